"""The TSDF volume at the KITTI shape, in one process: 1224x368 frames into 256x128x256 voxels.

  (a) integrate   nalo_tsdf_integrate_frame of a frame of the dense archive, 60 calls after warm-up: the kernel alone (the scope tsdf_integrate) and the whole
                  call with a drain; the kernel's bytes (16 B per visited voxel plus the plane) over the copy rate nalo_hbm_calibrate reports in the same run, and
                  how many of the volume's voxels the culling box visited
  (b) surface     nalo_tsdf_surface_points of that volume: ONE library call with room for the last count plus a margin (count, scan, write, the copy up, one
                  wait), and the binding's two-call form that asks for n_needed first (wall clock of either), against the only other route to a fused
                  surface: nalo_map_dense_world_points of the same frames to the host (the CPU fusion behind it is NOT timed)

Prints a table and one JSON line per part."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
from nalo_slam_amd import binding  # noqa: E402

F = np.float32
W, H, K = 1224, 368, (718.856, 718.856, 607.19, 185.21)
DIMS = (256, 128, 256)
FID = 700


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": float(np.median(us)), "p95": float(np.percentile(us, 95)), "n": int(us.size)}


def street(seed=0):
    """four mask values in vertical bands, each a wall at its own depth (6 .. 12 m), 400 window points on each"""
    rng = np.random.RandomState(seed)
    mask = np.zeros((H, W), F)
    u, v, idp = [], [], []
    for b, Z in enumerate((6.0, 9.0, 12.0, 8.0)):
        x0, x1 = b * W // 4, (b + 1) * W // 4
        mask[:, x0:x1] = 2.0 + b
        x, y = rng.randint(x0 + 4, x1 - 4, 400), rng.randint(4, H - 4, 400)
        u.append(x + 0.25); v.append(y + 0.5); idp.append(1.0 / (Z + rng.uniform(-0.002, 0.002, 400)))
    img = rng.uniform(5, 250, (H, W)).astype(F)
    bgr = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    return mask, img, bgr, np.concatenate(u).astype(F), np.concatenate(v).astype(F), np.concatenate(idp).astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4, help="poses the frame is integrated from before the surface is read")
    a = ap.parse_args()
    mask, img, bgr, u, v, idp = street()
    c = binding.Context(W, H, K, n_slots=2)
    for s in range(2):
        c.frame_upload(s, img, mask=mask, bgr=bgr)
    c.ba_set_window([0, 1], np.tile(np.eye(3, 4), (2, 1, 1)), frame_ids=[FID, FID + 1])
    P = len(u)
    c.ba_set_points(np.zeros(P, np.int32), u, v, idp, np.full((P, 8), 100, F), np.ones((P, 8), F))
    c.map_dense_enable(True)
    draws = np.random.RandomState(1).randint(0, 2 ** 32, 150, dtype=np.uint64).astype(np.uint32)     # the plane fit's RANSAC draws, 50 samples
    poses = [np.concatenate([np.eye(3), np.array([[0.05 * k], [0.0], [0.1 * k]])], 1) for k in range(a.frames)]
    recs, runs, napp = c.dense_update_map(0, draws, poses[0])
    # 20 x 6 x 14 m in front of the first camera: voxels of 7.8 x 4.7 x 5.5 cm would not be cubes, so the largest sets the size
    vs = max(20.0 / DIMS[0], 6.0 / DIMS[1], 14.0 / DIMS[2])
    origin = (-0.5 * vs * DIMS[0], -0.5 * vs * DIMS[1], 1.0)
    c.tsdf_create(origin, vs, DIMS, 4 * vs, 64.0)
    copy_GBs, triad_GBs = c.hbm_calibrate(1 << 28, 10)
    c.profile_enable(True)
    c.profile_select("tsdf_integrate")
    wall = []
    for k in range(a.warmup + a.reps):
        if k == a.warmup:
            c.sync()
            c.profile_reset()
        c.sync()
        t0 = time.perf_counter()
        c.tsdf_integrate_frame(FID, poses[k % a.frames], K, 0.5, 20.0)
        c.sync()
        if k >= a.warmup:
            wall.append((time.perf_counter() - t0) * 1e6)
    st = c.tsdf_last()
    kern = np.asarray(c.profile_samples("tsdf_integrate"), np.float64)
    c.profile_enable(False)
    nbytes = 16 * st["visited"] + 4 * W * H
    ks = stats(kern)
    ra = {"part": "integrate", "dense_points": int(napp), "kernel_us": ks, "call_us": stats(wall), "visited": st["visited"], "updated": st["updated"],
          "visited_fraction": st["visited"] / float(np.prod(DIMS)), "bytes": nbytes, "GBs_at_median": nbytes / ks["median"] * 1e-3, "copy_GBs": copy_GBs,
          "fraction_of_copy_rate": nbytes / ks["median"] * 1e-3 / copy_GBs}
    surf, surf2, world = [], [], []
    n_pts = len(c.tsdf_surface_points(1.0))
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        pts = c.tsdf_surface_points(1.0, cap=n_pts + 1024)
        t1 = time.perf_counter()
        for p in poses:
            c.map_dense_world_points(FID, p)
        t2 = time.perf_counter()
        pts2 = c.tsdf_surface_points(1.0)
        t3 = time.perf_counter()
        assert len(pts) == len(pts2) == n_pts
        if k >= a.warmup:
            surf.append((t1 - t0) * 1e6)
            world.append((t2 - t1) * 1e6)
            surf2.append((t3 - t2) * 1e6)
    rb = {"part": "surface", "surface_points": n_pts, "surface_points_one_call_us": stats(surf), "surface_points_two_calls_us": stats(surf2),
          "world_points_of_%d_frames_us" % a.frames: stats(world),
          "bytes_up_surface": 12 * n_pts, "bytes_up_world_points": 24 * int(napp) * a.frames}
    print("tsdf_integrate  kernel median %.1f us (p95 %.1f), call %.1f us; %d of %d voxels visited (%.1f %%), %.0f GB/s = %.2f of the copy rate %.0f GB/s" % (
        ks["median"], ks["p95"], ra["call_us"]["median"], st["visited"], int(np.prod(DIMS)), 100 * ra["visited_fraction"], ra["GBs_at_median"], ra["fraction_of_copy_rate"], copy_GBs))
    print("tsdf_surface    %d points, one call median %.1f us (p95 %.1f), asking for n_needed first %.1f us (p95 %.1f); nalo_map_dense_world_points of the %d frames: %.1f us (p95 %.1f)" % (
        n_pts, stats(surf)["median"], stats(surf)["p95"], stats(surf2)["median"], stats(surf2)["p95"], a.frames, stats(world)["median"], stats(world)["p95"]))
    print(json.dumps(ra))
    print(json.dumps(rb))
    c.close()


if __name__ == "__main__":
    main()
