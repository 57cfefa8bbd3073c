"""What re-fusing the window's keyframes costs in the TSDF volume: ONE nalo_tsdf_replace_frames launch (scope tsdf_replace_n) against the sum of the n
tsdf_replace launches of the loop of nalo_tsdf_replace_frame, on scripts/diag/tsdf_replace_ab.py's street (1224x368 frames, walls at 6 .. 12 m) and a 256x64x256
volume, without and with colour, for n = 2, 4, 7 and 15 frames along a forward walk, in one process.

The frames are dense depth planes of the street in device memory, one per frame, and go through the plane-level calls nalo_tsdf_replace_depth_n and
nalo_tsdf_replace_depth: these launch the same two kernels as nalo_tsdf_replace_frames and nalo_tsdf_replace_frame do behind their plane builds, which are the
same work on both routes and are not what is compared (a dense archive of fifteen full-size frames needs a device chain this script does not build). Two
contexts hold the same volume; in every repetition context A
moves all n frames from their current poses to perturbed ones in one launch and context B does the same with n launches, their kernel times summed; the next
repetition moves them back, and the order of A and B alternates. Kernel times are the scopes' event brackets, after a warm-up. The whole volume (32 MiB, 80 MiB
with colour) fits the Infinity Cache: these are warm-cache times, as tsdf_replace_ab.py's are. Prints a table and one JSON line per volume kind and n."""
import argparse
import json
import os
import sys

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
    """tsdf_replace_ab.py's scene as a dense plane: four vertical bands, each a wall at its own depth, a millimetre of noise, and a colour image"""
    rng = np.random.RandomState(seed)
    depth = np.zeros((H, W), F)
    for b, Z in enumerate((6.0, 9.0, 12.0, 8.0)):
        depth[:, b * W // 4:(b + 1) * W // 4] = Z
    depth += rng.uniform(-0.002, 0.002, (H, W)).astype(F)
    return depth, rng.randint(0, 256, (H, W, 3)).astype(np.uint8)


def pose(dx, dy, dz):
    return np.concatenate([np.eye(3), np.array([[dx], [dy], [dz]])], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    vs = max(20.0 / DIMS[0], 6.0 / DIMS[1], 14.0 / DIMS[2])
    rng = np.random.RandomState(3)
    for colour in (False, True):
        for n in (2, 4, 7, 15):
            # a forward walk of 0.1 m a frame, each frame with its own plane; the correction moves every frame by about a voxel and rescales it by 2 %
            planes = [street(k) for k in range(n)]
            walk = [pose(0.02 * k, 0.0, 0.1 * k) for k in range(n)]
            moved = [pose(0.02 * k + vs * rng.uniform(-1, 1), vs * rng.uniform(-0.5, 0.5), 0.1 * k + vs * rng.uniform(-1, 1)) for k in range(n)]
            ctxs = []
            for _ in range(2):
                c = binding.Context(W, H, K, n_slots=1)
                c.tsdf_create((-0.5 * vs * DIMS[0], -0.5 * vs * DIMS[1], 1.0), vs, DIMS, 4 * vs, 64.0)
                if colour:
                    c.tsdf_color_enable()
                dev = [(torch.from_numpy(d).cuda(), torch.from_numpy(b).cuda() if colour else None) for d, b in planes]
                side = lambda k, p, s, dev=dev: binding.tsdf_side(dev[k][0], K, p, s, MN, MX, colour=dev[k][1])
                c.tsdf_replace_depth_n([dict(add=side(k, walk[k], 1.0)) for k in range(n)])
                c.profile_enable(True)
                ctxs.append((c, side))
            (A, sideA), (B, sideB) = ctxs
            visited = {}

            def leg_A(old, new, s_old, s_new):
                A.tsdf_replace_depth_n([dict(remove=sideA(k, old[k], s_old), add=sideA(k, new[k], s_new)) for k in range(n)])
                visited["one_launch"] = A.tsdf_last()["visited"]

            def leg_B(old, new, s_old, s_new):
                v = 0
                for k in range(n):
                    B.tsdf_replace_depth(remove=sideB(k, old[k], s_old), add=sideB(k, new[k], s_new))
                    v += B.tsdf_last()["visited"]
                visited["n_launches"] = v

            for r in range(a.warmup + a.reps):
                if r == a.warmup:
                    for x in (A, B):
                        x.sync()
                        x.profile_reset()
                args = (walk, moved, 1.0, 1.02) if r % 2 == 0 else (moved, walk, 1.02, 1.0)
                for leg in ((leg_A, leg_B) if (r // 2) % 2 == 0 else (leg_B, leg_A)):
                    leg(*args)
            ka = np.asarray(A.profile_samples("tsdf_replace_n"), np.float64)
            kb = np.asarray(B.profile_samples("tsdf_replace"), np.float64).reshape(-1, n).sum(1)
            assert len(ka) == len(kb) == a.reps
            same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(A.tsdf_get(), B.tsdf_get()))
            assert same, "the one launch and the n launches left different volumes"
            res = {"volume": "coloured" if colour else "plain", "n": n, "dims": DIMS, "frame": [W, H], "visited": visited,
                   "kernel_us": {"one_launch": stats(ka), "n_launches_sum": stats(kb)}, "one_over_sum": float(np.median(ka) / np.median(kb))}
            print("%-8s n %2d: one launch %8.1f us (p95 %8.1f) | sum of %2d launches %8.1f us (p95 %8.1f) | ratio %.2f | hull %d voxels, the n hulls together %d" % (
                res["volume"], n, res["kernel_us"]["one_launch"]["median"], res["kernel_us"]["one_launch"]["p95"], n, res["kernel_us"]["n_launches_sum"]["median"],
                res["kernel_us"]["n_launches_sum"]["p95"], res["one_over_sum"], visited["one_launch"], visited["n_launches"]))
            print(json.dumps(res))
            A.close()
            B.close()


if __name__ == "__main__":
    main()
