"""dense=1 step 6 of makeCoarseDepthL0 (CoarseTracker.cpp:540-666) two ways in one process, the routes alternating per keyframe: wall time from the first call to
a drained stream, medians with p10 / p90

  host    nalo_trk_get_pc read back, makeMaskDistMap in NumPy, the defined fit in NumPy (tests/plane_model.py), nalo_trk_append_plane_points per cluster: what
          a caller did before nalo_trk_fit_planes (with PCL in place of the NumPy fit)
  device  nalo_trk_fit_planes(append = 1)

at 1224x368 with the level-0 cloud trk_set_ref builds from ~2500 reference inputs, and at 1920x1072 with a 160 k-point injected cloud over 40 mask values. Every
keyframe starts from the same cloud (restored untimed). The script checks that both routes leave the same level-0 cloud (inverse depths to 1e-6). The kernels' own
times: run this under rocprofv3 --kernel-trace --stats (rows plane_*_kernel, trk_append_clusters_kernel and rocPRIM's sort)."""
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
import plane_cases as pc  # noqa: E402
import plane_model as pm  # noqa: E402
from nalo_slam_amd import binding, synth  # noqa: E402


def setup(name):
    if name == "kitti00":
        w, h = 1224, 368
        win = synth.make_window(w=w, h=h, W=3, P=300, seed=4)
        rng = np.random.RandomState(2)
        Ku, Kv = rng.uniform(5, w - 6, 2500).astype(np.float32), rng.uniform(5, h - 6, 2500).astype(np.float32)
        d = win.depth[win.W - 1][(Kv + 0.5).astype(int), (Ku + 0.5).astype(int)]
        ok = np.isfinite(d)
        mask = pc.six_region_mask(w, h)
        c = binding.Context(w, h, win.K, n_slots=1)
        c.frame_upload(0, win.images[win.W - 1], mask=mask)
        c.trk_set_ref(0, Ku[ok], Kv[ok], (1.0 / d[ok]).astype(np.float32), np.full(int(ok.sum()), 1e-4, np.float32))
        return c, c.trk_get_pc(0), mask, w, h, win.K
    sc = pc.large_scene()
    c = binding.Context(sc["w"], sc["h"], sc["K"], n_slots=1)
    c.frame_upload(0, np.random.RandomState(0).uniform(0, 255, (sc["h"], sc["w"])).astype(np.float32), mask=sc["mask"])
    cloud = (sc["u"], sc["v"], sc["idp"], np.full(len(sc["u"]), 100, np.float32))
    return c, cloud, sc["mask"], sc["w"], sc["h"], sc["K"]


def run(name, keyframes):
    c, cloud, mask, w, h, K = setup(name)
    draws = pm.make_draws(9)

    def host_leg():
        u, v, idp, _ = c.trk_get_pc(0)
        cl = pm.fit_planes(u, v, idp, mask, w, h, K, draws, fast=True)
        if len(cl) >= 4:
            for m in cl:
                if m["fitted"]:
                    c.trk_append_plane_points(m["plane"][:3], float(m["plane"][3]), int(m["mask_value"]), m["rect"])
        c.sync()

    def device_leg():
        c.trk_fit_planes(draws, append=1)
        c.sync()

    t = {"host": [], "device": []}
    result = {}
    for k in range(keyframes + 2):
        for leg, fn in (("host", host_leg), ("device", device_leg)) if k % 2 == 0 else (("device", device_leg), ("host", host_leg)):
            c.trk_set_pc(0, 0, *cloud)
            c.sync()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 2:
                t[leg].append(dt)
            result[leg] = c.trk_get_pc(0)
    # u, v, colour and the counts equal; the inverse depths to 1e-6: the NumPy fit sums the refinement sequentially, the device in tree order, so a plane
    # coefficient may differ in its last float bit
    ha, da = result["host"], result["device"]
    same = len(ha[0]) == len(da[0]) and all(np.array_equal(ha[i], da[i]) for i in (0, 1, 3)) and np.allclose(ha[2], da[2], rtol=1e-6, atol=0)
    print("%s: cloud %d -> %d points, both routes leave the same level-0 cloud: %s" % (name, len(cloud[0]), len(result["device"][0]), same))
    for leg in ("host", "device"):
        a = np.array(t[leg])
        print("  %-7s median %9.3f ms   p10 %9.3f   p90 %9.3f   (%d keyframes)" % (leg, np.median(a), np.percentile(a, 10), np.percentile(a, 90), len(a)))
    c.close()
    return same


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--shapes", default="kitti00,cloud160k")
    a = ap.parse_args()
    ok = all([run(s, a.keyframes) for s in a.shapes.split(",")])
    sys.exit(0 if ok else 1)
