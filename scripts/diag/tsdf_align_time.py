"""nalo_tsdf_align_eval at the KITTI shape: the volume of tests/test_tsdf_gpu.py's chain (1224x368, W = 8, three keyframes fused into 256x64x256 voxels) and the
depth plane nalo_tsdf_raycast sees from the last keyframe's pose (1224x368, left on the device: nalo_tsdf_raycast_view), evaluated at that pose, step = 1, for
dof = 6 and dof = 7, with min_weight = 0: the chain's dense planes are sparse, its fused weights have holes, and at min_weight = 1 no pixel has all seven samples.
Per leg the whole call (wall clock: one launch, one wait, the 37 doubles and four counts from host-mapped memory) and the scope tsdf_align (the kernel, HIP
events), median and p95; and one whole nalo_tsdf_align_depth of twelve iterations from a start two voxels off.

The bytes an evaluation touches, counted from the states it reports: 4 B of the plane per visited pixel; a sample that passes the index test gathers eight
weights (32 B) and, when they are all valid, eight tsdf words (32 B) - one sample for a pixel whose S(q) is invalid, up to seven for the others, taken here as
the full 7 x 64 B for a used pixel and 64 B for the rest (an upper estimate of what the lanes ask for, not of what leaves HBM: the seven samples of a pixel
share most of a 4 x 4 x 4 neighbourhood and the volume, 34 MB, stays in the Infinity Cache across calls); and 336 B of partial record per workgroup, written
once and read once by the last one. There is no pass mark: nobody had measured this path, and the log is where the first number goes.

Prints a table and one JSON line; --log appends both to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
from tsdf_ab import stats  # noqa: E402  (loads the package)
from tsdf_raycast_time import chain_context  # noqa: E402

from nalo_slam_amd import binding  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    c, made, T, K, mn, mx = chain_context()
    w, h = 1224, 368
    nx, ny, nz = made.dims
    rc = c.tsdf_raycast(w, h, K, T, mn, mx, (mx - mn) / 250.0, 1.0, download=False)
    plane = c.tsdf_raycast_view()["depth"]
    copy_GBs, _ = c.hbm_calibrate(1 << 28, 10)
    kw = dict(min_depth=mn, max_depth=mx, min_weight=0.0, huber=0.5, step=1)
    wall, scope, sums = {}, {}, {}
    for dof in (6, 7):
        name = "dof%d" % dof
        wall[name] = []
        for k in range(a.warmup + a.reps):
            c.sync()
            t0 = time.perf_counter()
            sums[name] = c.tsdf_align_eval(plane, K, T, 1.0, dof=dof, **kw)
            if k >= a.warmup:
                wall[name].append((time.perf_counter() - t0) * 1e6)
    c.profile_enable(True)
    c.profile_select("tsdf_align")
    for dof in (6, 7):
        for k in range(a.warmup + a.reps):
            if k == a.warmup:
                c.sync()
                c.profile_reset()
            c.tsdf_align_eval(plane, K, T, 1.0, dof=dof, **kw)
        c.sync()
        scope["dof%d" % dof] = stats(np.asarray(c.profile_samples("tsdf_align"), np.float64))
    c.profile_enable(False)
    start = np.array(T, np.float64)
    start[:, 3] += 2.0 * float(made.voxel_size) / np.sqrt(3.0)
    loop_us = []
    for k in range(3 + 10):
        c.sync()
        t0 = time.perf_counter()
        lp = c.tsdf_align_depth(plane, K, start, 1.0, dof=7, max_iterations=12, min_used=100, eps=0.0, **kw)
        if k >= 3:
            loop_us.append((time.perf_counter() - t0) * 1e6)
    n = sums["dof7"]["count"]
    blocks = ((w + 15) // 16) * ((h + 15) // 16)
    touched = dict(plane=4 * w * h, gathers=7 * 64 * n[0] + 64 * (n[2] + n[3]), partial_records=2 * 336 * blocks)
    total = sum(touched.values())
    out = {"part": "tsdf_align", "plane": [w, h], "dims": [nx, ny, nz], "raycast_hits": rc["n_hit"], "count": n, "scope_us": scope, "call_us": {k: stats(v) for k, v in wall.items()},
           "bytes": touched, "copy_GBs": copy_GBs, "loop12_us": stats(loop_us), "loop": dict(status=lp["status"], iterations=lp["iterations"], evaluations=lp["evaluations"],
                                                                                            E_per_pixel=[lp["E_first"] / max(lp["n_first"], 1), lp["E_last"] / max(lp["n_last"], 1)])}
    lines = ["tsdf_align_eval %dx%d, step 1, against %dx%dx%d: used / no depth / S invalid / gradient invalid %s" % (w, h, nx, ny, nz, n),
             "  bytes asked for: plane %.2f MB, gathers %.1f MB (7 x 64 B a used pixel), partial records %.2f MB = %.1f MB; at the copy rate of %.0f GB/s that is %.1f us" % (
                 touched["plane"] * 1e-6, touched["gathers"] * 1e-6, touched["partial_records"] * 1e-6, total * 1e-6, copy_GBs, total / (copy_GBs * 1e3))]
    for name in ("dof6", "dof7"):
        s, cl = scope[name], stats(wall[name])
        lines.append("  %-6s scope median %.1f us (p95 %.1f) = %.0f GB/s of the bytes asked for; call with its wait median %.1f us (p95 %.1f)" % (
            name, s["median"], s["p95"], total / (s["median"] * 1e3), cl["median"], cl["p95"]))
    lines.append("  nalo_tsdf_align_depth, dof 7, 12 iterations from two voxels off: median %.1f us (%d evaluations), E per pixel %.3g -> %.3g" % (
        out["loop12_us"]["median"], lp["evaluations"], out["loop"]["E_per_pixel"][0], out["loop"]["E_per_pixel"][1]))
    lines.append(json.dumps(out))
    print("\n".join(lines))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
