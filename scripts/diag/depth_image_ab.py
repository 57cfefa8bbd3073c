"""The tracker's depth image of one keyframe (debugPlotIDepthMap -> pushDepthImage), two ways in one process, the legs alternating per keyframe: wall time from the
first call to the result on the host

  device    nalo_trk_depth_image: the radix select, the smoothing and the paint on the device, 3 B/px (+ a few scalars) up behind one wait
  readback  the route it replaces for a caller of the device chain: nalo_trk_get_depth(0) (4 B/px, and the weight sums the binding fetches with it) +
            nalo_frame_download(slot, 0) (16 B/px of {I, dx, dy, 0} on the bus; the binding also fetches absSquaredGrad) ...
  hostloops ... + the sort and the two image-wide loops, here as tests/depth_image_model.py's vectorised NumPy `fast` (a stand-in for the caller's C++ loops,
            which were NOT measured; reported apart from the transfers)

at 1224x368 and at 1920x1072, on a synthetic keyframe (nalo_trk_set_ref on points of the analytic scene, untimed, the stream drained before each leg). The pair
{minID, maxID} is carried from keyframe to keyframe in both legs. The script checks that both routes give the same bytes on every keyframe. The kernels' own
times: run this under rocprofv3 --kernel-trace --stats with --shapes WxH, one run per shape (rows di_*)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
import depth_image_model as model  # noqa: E402
from nalo_slam_amd import binding, synth  # noqa: E402


def one_shape(w, h, n_pts, keyframes):
    win = synth.make_window(w=w, h=h, W=2, P=8, seed=3, n_extra=0)
    rng = np.random.RandomState(1)
    c = binding.Context(w, h, win.K, n_slots=2)
    refs = []
    for i in range(2):
        c.frame_upload(i, win.images[i])
        Ku, Kv = rng.uniform(5, w - 6, n_pts).astype(np.float32), rng.uniform(5, h - 6, n_pts).astype(np.float32)
        d = win.depth[i][(Kv + 0.5).astype(int), (Ku + 0.5).astype(int)]
        ok = np.isfinite(d)
        refs.append((Ku[ok], Kv[ok], (1.0 / d[ok]).astype(np.float32), np.full(int(ok.sum()), 1e-4, np.float32)))
    box = {}

    def device(pair):
        box["dev"] = c.trk_depth_image(pair)

    def readback():
        box["rb"] = (c.trk_get_depth(0)[0], c.frame_download(box["slot"], 0)[0][:, 0])

    def hostloops(pair):
        box["model"] = model.fast(box["rb"][0], box["rb"][1], w, h, pair)

    legs = ["device", "readback", "hostloops"]
    ts = {k: [] for k in legs}
    pair = np.array([-1.0, -1.0], np.float32)
    same, npos = True, 0
    for i in range(keyframes + 1):                                             # keyframe 0 is the warm-up (first-use allocations), not timed
        box["slot"] = i % 2
        c.trk_set_ref(i % 2, *[a * np.float32(1.0 + 0.1 * (i % 3)) if k == 2 else a for k, a in enumerate(refs[i % 2])])
        c.sync()
        t = {}
        for k in (("device", "readback") if i % 2 == 0 else ("readback", "device")):
            t0 = time.perf_counter()
            (device(pair) if k == "device" else readback())
            t[k] = time.perf_counter() - t0
        t0 = time.perf_counter(); hostloops(pair); t["hostloops"] = time.perf_counter() - t0
        dev, mod = box["dev"], box["model"]
        same = same and np.array_equal(dev["bgr"], mod["bgr"]) and dev["minmax"].tobytes() == mod["minmax"].tobytes() and dev["n_positive"] == mod["n_positive"]
        pair, npos = dev["minmax"], dev["n_positive"]
        if i > 0:
            for k in legs:
                ts[k].append(t[k])
    print("depth_image_ab: %d x %d, %d positive pixels in the map, %d keyframes per leg; both routes give the same bytes: %s" % (w, h, npos, keyframes, same))
    med = {}
    for k in legs:
        a = np.array(ts[k]) * 1e6
        med[k] = np.median(a)
        print("  %-9s median %9.1f us   p10 %9.1f   p90 %9.1f" % (k, med[k], np.percentile(a, 10), np.percentile(a, 90)), flush=True)
    print("  read-back route, total  = readback + hostloops (NumPy): %9.1f us" % (med["readback"] + med["hostloops"]))
    c.close()
    return same


ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=40)
ap.add_argument("--shapes", default="1224x368,1920x1072", help="comma-separated WxH (one shape per profiler run keeps the kernel rows apart)")
args = ap.parse_args()
ok = True
for shape in args.shapes.split(","):
    w, h = [int(v) for v in shape.split("x")]
    ok = one_shape(w, h, 3000 if w * h < 1000000 else 12000, args.keyframes) and ok
sys.exit(0 if ok else 1)
