"""DenseMapping::updateMap for one keyframe two ways in one process, the legs alternating per keyframe: wall time per call (from the first call to the vertex
arrays in host memory), medians with p10 / p90

  A  nalo_dense_fit_planes, then nalo_dense_make_map per fitted cluster with its read-backs (19 bytes per point), the accepted runs appended on the host, and the
     vertex arrays of refreshPC() built from them in NumPy: what a caller does without nalo_dense_update_map
  B  nalo_dense_update_map + nalo_map_dense_cloud (the archive is reset, untimed, before every call)

at 1224x368 and 1920x1072 with a mask of twelve values in irregular regions, some interleaved so that their boxes overlap (the ground in stripes and a
checkerboard, ellipses above the horizon). The script checks that both legs give the same points and the same vertices. The kernels of leg B alone:

  rocprofv3 --kernel-trace --stats -- python scripts/diag/dense_update_ab.py --only-b

(rows dense_boxes*_kernel, dense_*_batch_kernel, act_scan_kernel, dense_decide_kernel, dense_copy_kernel, map_dense_cloud_*_kernel)."""
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
import plane_model as pm  # noqa: E402
from nalo_slam_amd import binding  # noqa: E402

F = np.float32
FID = 1


def make_scene(w, h, seed=12):
    """twelve values: six on the ground plane Y = 1.65 below row 0.68 h (three bands, each split in two interleaved values), six walls in ellipses above 0.46 h"""
    fx = 718.856 * w / 1224.0
    K = (fx, fx, 607.19 * w / 1224.0, 185.2 * h / 368.0)
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    low, up = yy >= int(0.68 * h), yy < int(0.46 * h)
    mask = np.zeros((h, w), F)
    regions = []
    for i in range(3):
        band = low & (xx >= 10 + i * (w - 20) // 3) & (xx < 10 + (i + 1) * (w - 20) // 3 - 10)
        a = band & ((xx // 7 + yy // 5) % 2 == 0) if i == 1 else band & (xx % 10 < 5 + i)
        regions += [(30.0 + 2 * i, a, 260 - 20 * i, None), (31.0 + 2 * i, band & ~a, 150 - 10 * i, None)]
    for i, Z in enumerate([6.0, 9.0, 14.0, 200.0, 300.0, 25.0]):
        ell = up & (((xx - (100 + 200 * i) * w / 1224.0) / ((90.0 + 8 * i) * w / 1224.0)) ** 2 + ((yy - (80 + 5 * i) * h / 368.0) / ((50.0 + 6 * i) * h / 368.0)) ** 2 < 1)
        regions.append((40.0 + i, ell, 120 - 9 * i, Z))
    us, vs, ids = [], [], []
    for value, sel, n, Z in regions:
        mask[sel] = value
        s = sel.copy()
        s[:3] = s[h - 2:] = False
        s[:, :3] = s[:, w - 2:] = False
        ys, xs = np.nonzero(s)
        pick = rng.choice(len(xs), n, replace=False)
        x, y = xs[pick], ys[pick]
        depth = (Z + rng.uniform(-0.001, 0.001, n)) if Z else (1.65 + rng.uniform(-0.001, 0.001, n)) / ((y - K[3]) / K[1])
        us.append(x + 0.25); vs.append(y + 0.5); ids.append(1.0 / depth)
    u, v, idp = [np.concatenate(a).astype(F) for a in (us, vs, ids)]
    return dict(w=w, h=h, K=K, mask=mask, img=rng.uniform(5, 250, (h, w)).astype(F), bgr=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), u=u, v=v, idp=idp)


def context(sc):
    c = binding.Context(sc["w"], sc["h"], sc["K"], n_slots=2)
    for i in range(2):
        c.frame_upload(i, sc["img"], mask=sc["mask"], bgr=sc["bgr"])
    P = len(sc["u"])
    c.ba_set_window([0, 1], np.tile(np.eye(3, 4), (2, 1, 1)), frame_ids=[FID, FID + 1])
    c.ba_set_points(np.zeros(P, np.int32), sc["u"], sc["v"], sc["idp"], np.full((P, 8), 100, F), np.ones((P, 8), F))
    c.map_dense_enable(True)
    return c


def run(w, h, keyframes, only_b):
    sc = make_scene(w, h)
    c = context(sc)
    draws = pm.make_draws(12)
    c2w = np.concatenate([np.eye(3), np.array([[0.5], [0.1], [2.0]])], 1)
    cal = c.ba_get_frames()[2]
    fx, fy, cx, cy = [F(x) for x in cal]
    fxi, fyi, cxi, cyi = F(1) / fx, F(1) / fy, -cx / fx, -cy / fy
    cap = w * h

    def leg_a():
        recs, _ = c.dense_fit_planes(0, draws)
        parts = []
        for r in recs:
            if not r["fitted"]:
                continue
            d = c.dense_make_map(0, r["plane"], float(r["mask_value"]), c2w, cap=cap)
            if d["n"] > 0 and d["accept"]:
                parts.append(d)
        u, v = np.concatenate([p["u"] for p in parts]), np.concatenate([p["v"] for p in parts])
        idp, bgr = np.concatenate([p["idepth"] for p in parts]), np.concatenate([p["bgr"] for p in parts])
        keep = ~(idp < 0)
        depth = (F(1) / idp[keep]).astype(F)
        xyz = np.stack([(u[keep].astype(F) * fxi + cxi) * depth, (v[keep].astype(F) * fyi + cyi) * depth, depth], 1).astype(F)
        return dict(u=u, v=v, idepth=idp, bgr=bgr, xyz=xyz, rgb=bgr[keep][:, ::-1])

    def leg_b():
        c.dense_update_map(0, draws, c2w)
        g = c.map_dense_cloud(FID)
        return dict(xyz=g["xyz"], rgb=g["rgb"])

    legs = (("B", leg_b),) if only_b else (("A", leg_a), ("B", leg_b))
    t = {k: [] for k, _ in legs}
    res = {}
    for k in range(keyframes + 2):
        for name, fn in (legs if k % 2 == 0 else legs[::-1]):
            c.map_reset()
            c.sync()
            t0 = time.perf_counter()
            res[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 2:
                t[name].append(dt)
    same = True
    p = c.map_dense_get(FID)
    if not only_b:
        a = res["A"]
        same = (len(p) == len(a["u"]) and np.array_equal(p["u"], a["u"]) and np.array_equal(p["v"], a["v"]) and np.array_equal(p["idepth"].view(np.uint32), a["idepth"].view(np.uint32))
                and np.array_equal(p["bgr"], a["bgr"]) and np.array_equal(res["B"]["xyz"].view(np.uint32), a["xyz"].view(np.uint32)) and np.array_equal(res["B"]["rgb"], a["rgb"]))
    print("%dx%d: %d points appended, %d vertices, both legs give the same points and vertices: %s" % (w, h, len(p), len(res["B"]["xyz"]), same))
    for name, _ in legs:
        a = np.array(t[name])
        print("  leg %s median %9.3f ms   p10 %9.3f   p90 %9.3f   (%d keyframes)" % (name, np.median(a), np.percentile(a, 10), np.percentile(a, 90), len(a)))
    c.close()
    return same


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--shapes", default="1224x368,1920x1072")
    ap.add_argument("--only-b", action="store_true")
    a = ap.parse_args()
    ok = all([run(*[int(x) for x in s.split("x")], a.keyframes, a.only_b) for s in a.shapes.split(",")])
    sys.exit(0 if ok else 1)
