"""What taking a fused plane back, and putting it in again at a corrected pose, costs in the TSDF volume (nalo_tsdf_replace_depth), on scripts/diag/tsdf_ab.py's
street (a 1224x368 frame, walls at 6 .. 12 m) and a 256x64x256 volume, without and with colour, in one process. The frame is a dense depth plane of the scene
(and its colour image) in device memory; the volume holds four other poses of it, so a removal divides and does not merely reset. Two contexts on the same
scene, their legs alternating inside every repetition:

  integrate   nalo_tsdf_integrate_depth[_color]: the scope tsdf_integrate, the yardstick (that kernel is the parent commit's)
  remove      nalo_tsdf_replace_depth, remove only                          (scope tsdf_replace)
  add         nalo_tsdf_replace_depth, add only
  fused       nalo_tsdf_replace_depth, remove at the old pose and add at one moved by about a voxel, ONE launch
  two calls   the same replacement on the twin context as remove, then add: two launches, their kernel times summed, one drain behind the second

Kernel times are the scopes' event brackets, call times a host clock around the call(s) and a drain. The whole volume (32 MiB, 80 MiB with colour) fits the
Infinity Cache and every leg runs over the same voxels: these are warm-cache times, as tsdf_ab.py's are. Prints a table and one JSON line per volume kind."""
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

F = np.float32
W, H, K = 1224, 368, (718.856, 718.856, 607.19, 185.21)
DIMS = (256, 64, 256)
MN, MX = 0.5, 20.0


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": float(np.median(us)), "p95": float(np.percentile(us, 95)), "n": int(us.size)}


def street(seed=0):
    """tsdf_ab.py's scene as a dense plane: four vertical bands, each a wall at its own depth, a millimetre of noise, and a colour image"""
    rng = np.random.RandomState(seed)
    depth = np.zeros((H, W), F)
    for b, Z in enumerate((6.0, 9.0, 12.0, 8.0)):
        depth[:, b * W // 4:(b + 1) * W // 4] = Z
    depth += rng.uniform(-0.002, 0.002, (H, W)).astype(F)
    return depth, rng.randint(0, 256, (H, W, 3)).astype(np.uint8)


def pose(dx, dz):
    return np.concatenate([np.eye(3), np.array([[dx], [0.0], [dz]])], 1)


def scene_context(colour, depth, bgr, vs):
    c = binding.Context(W, H, K, n_slots=1)
    c.tsdf_create((-0.5 * vs * DIMS[0], -0.5 * vs * DIMS[1], 1.0), vs, DIMS, 4 * vs, 64.0)
    if colour:
        c.tsdf_color_enable()
    d, b = torch.from_numpy(depth).cuda(), torch.from_numpy(bgr).cuda() if colour else None
    for k in range(1, 5):                                                      # the four other poses the volume holds throughout
        c.tsdf_integrate_depth(d, K, pose(0.05 * k, 0.1 * k), MN, MX, colour=b)
    side = lambda p: binding.tsdf_side(d, K, p, 1.0, MN, MX, colour=b)
    return c, d, b, side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    depth, bgr = street()
    vs = max(20.0 / DIMS[0], 6.0 / DIMS[1], 14.0 / DIMS[2])
    p0, p1 = pose(0.0, 0.0), pose(1.1 * vs, 0.7 * vs)                           # the correction: about a voxel
    for colour in (False, True):
        A, dA, bA, sideA = scene_context(colour, depth, bgr, vs)
        B, dB, bB, sideB = scene_context(colour, depth, bgr, vs)
        copy_GBs, _ = A.hbm_calibrate(1 << 28, 10)
        start = [x.tsdf_get()[1].tobytes() for x in (A, B)]
        for x in (A, B):
            x.profile_enable(True)
        wall = {k: [] for k in ("integrate", "remove", "add", "fused", "two_calls")}
        visited = {}

        def timed(c, name, fn, keep):
            c.sync()
            t0 = time.perf_counter()
            fn()
            c.sync()
            if keep:
                wall[name].append((time.perf_counter() - t0) * 1e6)

        def legs_A(keep):
            # + p0 | p0 -> p1 | p1 -> p0 | - p0 | + p0 | - p0: the volume ends every repetition as it began. tsdf_replace launches: fused, fused, remove, add, remove
            timed(A, "integrate", lambda: A.tsdf_integrate_depth(dA, K, p0, MN, MX, colour=bA), keep)
            timed(A, "fused", lambda: A.tsdf_replace_depth(remove=sideA(p0), add=sideA(p1)), keep)
            visited["fused"] = A.tsdf_last()["visited"]
            timed(A, "fused", lambda: A.tsdf_replace_depth(remove=sideA(p1), add=sideA(p0)), keep)
            timed(A, "remove", lambda: A.tsdf_replace_depth(remove=sideA(p0)), keep)
            visited["remove"] = A.tsdf_last()["visited"]
            timed(A, "add", lambda: A.tsdf_replace_depth(add=sideA(p0)), keep)
            A.tsdf_replace_depth(remove=sideA(p0))

        def two(old, new):
            B.tsdf_replace_depth(remove=sideB(old))
            B.tsdf_replace_depth(add=sideB(new))

        def legs_B(keep):
            # tsdf_replace launches: remove, add, remove, add, remove
            B.tsdf_integrate_depth(dB, K, p0, MN, MX, colour=bB)
            timed(B, "two_calls", lambda: two(p0, p1), keep)
            timed(B, "two_calls", lambda: two(p1, p0), keep)
            B.tsdf_replace_depth(remove=sideB(p0))

        for k in range(a.warmup + a.reps):
            if k == a.warmup:
                for x in (A, B):
                    x.sync()
                    x.profile_reset()
            for legs in ((legs_A, legs_B) if k % 2 == 0 else (legs_B, legs_A)):
                legs(k >= a.warmup)
        ki = np.asarray(A.profile_samples("tsdf_integrate"), np.float64)
        ka = np.asarray(A.profile_samples("tsdf_replace"), np.float64).reshape(-1, 5)
        kb = np.asarray(B.profile_samples("tsdf_replace"), np.float64).reshape(-1, 5)
        assert len(ki) == len(ka) == len(kb) == a.reps
        # removal and add are inverses only up to rounding: the weights, which count, must be back where they began
        assert [x.tsdf_get()[1].tobytes() for x in (A, B)] == start
        kern = {"integrate": stats(ki), "fused": stats(ka[:, :2].reshape(-1)), "remove": stats(ka[:, 2]), "add": stats(ka[:, 3]),
                "two_calls": stats(np.concatenate([kb[:, 0] + kb[:, 1], kb[:, 2] + kb[:, 3]]))}
        r = {"volume": "coloured" if colour else "plain", "dims": DIMS, "frame": [W, H], "copy_GBs": copy_GBs, "visited": visited,
             "kernel_us": kern, "call_us": {k: stats(v) for k, v in wall.items()},
             "fused_over_twice_integrate": kern["fused"]["median"] / (2 * kern["integrate"]["median"]), "fused_over_two_calls": kern["fused"]["median"] / kern["two_calls"]["median"]}
        print("%-8s volume %dx%dx%d, frame %dx%d, copy rate %.0f GB/s; kernel us median (p95) | call + drain us median (p95)" % ((r["volume"],) + DIMS + (W, H, copy_GBs)))
        for name in ("integrate", "remove", "add", "fused", "two_calls"):
            print("  %-10s %8.1f (%8.1f) | %8.1f (%8.1f)" % (name, kern[name]["median"], kern[name]["p95"], r["call_us"][name]["median"], r["call_us"][name]["p95"]))
        print("  fused / (2 x integrate) = %.2f   fused / two calls = %.2f   hull of the fused launch: %d voxels, of one side: %d" % (
            r["fused_over_twice_integrate"], r["fused_over_two_calls"], visited["fused"], visited["remove"]))
        print(json.dumps(r))
        A.close()
        B.close()


if __name__ == "__main__":
    main()
