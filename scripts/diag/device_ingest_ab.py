"""One keyframe's inputs into a slot, two ways in one process, the legs alternating per repeat:

  host    nalo_frame_upload_raw from pinned host memory: sensor frame (1 B/px), mask (1 B/px) and colour (3 B/px) cross PCIe, then ingest + pyramid
  device  nalo_frame_ingest_device from torch tensors that are resident on the device: ingest_dev + frame_attach + pyramid, nothing crosses

at 1224x368 (from 1241x376) and at 1920x1072 (from 1944x1088), 8-bit, photometricCalibration 2, with a remap table. Each shape runs twice: the keyframe's
inputs (image + mask + colour) and the image alone - the like-for-like pair of the two ingest kernels, since ingest_kernel resizes mask and colour in its own pass
while the device route does that in frame_attach. Two passes per run: wall clock of call + drain with profiling off, then the kernels' own times
(dispatch-attached timestamps of the scopes ingest, ingest_dev, frame_attach, pyramid) with profiling on. The script checks that both routes leave the same
level 0, mask and colour in the slot. Prints a table and one JSON line per run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
from nalo_slam_amd import binding  # noqa: E402


def radial_remap(w, h, wo, ho, k1=-0.12):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    nx, ny = (x - w / 2) / (0.6 * w), (y - h / 2) / (0.6 * w)
    r2 = nx * nx + ny * ny
    rx = ((nx * (1 + k1 * r2)) * 0.6 * w + wo / 2).astype(np.float32)
    ry = ((ny * (1 + k1 * r2)) * 0.6 * w + ho / 2).astype(np.float32)
    bad = ~((rx >= 0) & (ry >= 0) & (rx < wo - 1) & (ry < ho - 1))
    rx[bad] = -1
    ry[bad] = -1
    return rx, ry


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": float(np.median(us)), "p95": float(np.percentile(us, 95)), "n": int(us.size)}


def one_shape(w, h, wo, ho, reps, planes):
    rng = np.random.RandomState(w)
    G = np.cumsum(rng.rand(256) + 0.05)
    G = (255.0 * (G - G[0]) / (G[-1] - G[0])).astype(np.float32)
    yy, xx = np.mgrid[0:ho, 0:wo]
    vinv = (1.0 / (1.0 - 0.4 * (((xx - wo / 2) / wo) ** 2 + ((yy - ho / 2) / ho) ** 2))).astype(np.float32)
    rx, ry = radial_remap(w, h, wo, ho)
    c = binding.Context(w, h, (0.52 * w, 0.52 * w, (w - 1) / 2.0, (h - 1) / 2.0), n_slots=2)
    c.undist_set(wo, ho, G, vinv, 2, rx, ry)
    raw, mask, bgr = c.pinned_array((ho, wo), np.uint8), c.pinned_array((ho, wo), np.uint8), c.pinned_array((ho, wo, 3), np.uint8)
    raw[:], mask[:], bgr[:] = rng.randint(0, 256, (ho, wo)), rng.randint(0, 200, (ho, wo)), rng.randint(0, 256, (ho, wo, 3))
    t_raw, t_mask, t_bgr = (torch.from_numpy(np.array(a)).cuda() for a in (raw, mask, bgr))
    torch.cuda.synchronize()

    def host():
        c.frame_upload_raw(0, raw, exposure=0.02, mask_org=mask if planes else None, bgr_org=bgr if planes else None)

    def device():
        c.frame_ingest(1, image=t_raw, mask=t_mask if planes else None, colour=t_bgr if planes else None, exposure=0.02)

    for _ in range(5):
        host(); device()
    c.sync()
    same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(c.frame_download(0, 0), c.frame_download(1, 0)))
    same = same and (not planes or all(np.array_equal(a, b) for a, b in zip(c.frame_download_mask(0), c.frame_download_mask(1))))
    wall = {"host": [], "device": []}
    for _ in range(reps):
        for name, leg in (("host", host), ("device", device)):
            c.sync()
            t0 = time.perf_counter()
            leg()
            c.sync()
            wall[name].append((time.perf_counter() - t0) * 1e6)
    c.profile_enable(True)
    c.profile_reset()
    for _ in range(reps):
        host(); c.sync()
        device(); c.sync()
    scopes = {s: stats(c.profile_samples(s)) for s in ("ingest", "ingest_dev", "frame_attach", "pyramid") if planes or s != "frame_attach"}
    c.profile_enable(False)
    res = {"shape": "%dx%d from %dx%d" % (w, h, wo, ho), "inputs": "image + mask + colour" if planes else "image", "same_result": bool(same), "reps": reps,
           "pcie_bytes_host_leg": int(wo * ho * (5 if planes else 1)),
           "wall_us": {k: stats(v) for k, v in wall.items()}, "kernel_us": scopes}
    c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    for w, h, wo, ho, planes in ((1224, 368, 1241, 376, True), (1224, 368, 1241, 376, False), (1920, 1072, 1944, 1088, True), (1920, 1072, 1944, 1088, False)):
        r = one_shape(w, h, wo, ho, a.reps, planes)
        print("%s, %s  same result: %s  PCIe bytes per frame (host leg): %d" % (r["shape"], r["inputs"], r["same_result"], r["pcie_bytes_host_leg"]))
        for k, v in r["wall_us"].items():
            print("  wall, call + drain   %-12s median %8.1f us  p95 %8.1f us  (n=%d)" % (k, v["median"], v["p95"], v["n"]))
        for k, v in r["kernel_us"].items():
            print("  kernel scope         %-12s median %8.2f us  p95 %8.2f us  (n=%d)" % (k, v["median"], v["p95"], v["n"]))
        print(json.dumps(r))


if __name__ == "__main__":
    main()
