"""What colour in the TSDF volume costs, on scripts/diag/tsdf_ab.py's scene (the 1224x368 frame fused from four poses into 256x128x256 voxels), in one process:
two contexts on the same scene, one that never enables colour and one that does, their legs alternating inside every repetition.

  (a) integrate   nalo_tsdf_integrate_frame + drain and the scope tsdf_integrate (the kernel alone), without and with colour. The bytes colour adds by the plan:
                  3 planes x (16 B read + 16 B written) per lane that updated a voxel, plus the packed colour plane (4 B a pixel, written by the frame's colour
                  pass and the resolve pass, read where a voxel is updated)
  (b) mesh        nalo_tsdf_mesh against nalo_tsdf_mesh_color with the mesh left on the device (the scope tsdf_mesh and the call): 24 B read + 4 B written per
                  vertex by the plan

--root DIR measures another checkout's library instead (for instance the parent commit's, built there): where that tree has no colour only the uncoloured legs
run, which is how "colour costs nothing when it is off" is checked - this script on both trees, in alternating processes.
Prints a table and one JSON line per part."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), help="the checkout whose library is measured")
ap.add_argument("--tag", default="this tree")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
from nalo_slam_amd import binding  # noqa: E402

F = np.float32
W, H, K = 1224, 368, (718.856, 718.856, 607.19, 185.21)
DIMS = (256, 128, 256)
FID = 700
N_POSES = 4


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": float(np.median(us)), "p95": float(np.percentile(us, 95)), "n": int(us.size)}


def street(seed=0):
    """tsdf_ab.py's scene: four mask values in vertical bands, each a wall at its own depth (6 .. 12 m), 400 window points on each"""
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


def scene_context(colour):
    mask, img, bgr, u, v, idp = street()
    c = binding.Context(W, H, K, n_slots=2)
    for s in range(2):
        c.frame_upload(s, img, mask=mask, bgr=bgr)
    c.ba_set_window([0, 1], np.tile(np.eye(3, 4), (2, 1, 1)), frame_ids=[FID, FID + 1])
    P = len(u)
    c.ba_set_points(np.zeros(P, np.int32), u, v, idp, np.full((P, 8), 100, F), np.ones((P, 8), F))
    c.map_dense_enable(True)
    draws = np.random.RandomState(1).randint(0, 2 ** 32, 150, dtype=np.uint64).astype(np.uint32)
    poses = [np.concatenate([np.eye(3), np.array([[0.05 * k], [0.0], [0.1 * k]])], 1) for k in range(N_POSES)]
    recs, runs, napp = c.dense_update_map(0, draws, poses[0])
    vs = max(20.0 / DIMS[0], 6.0 / DIMS[1], 14.0 / DIMS[2])
    c.tsdf_create((-0.5 * vs * DIMS[0], -0.5 * vs * DIMS[1], 1.0), vs, DIMS, 4 * vs, 64.0)
    if colour:
        c.tsdf_color_enable()
    return c, poses, int(napp)


def main():
    a = ARGS
    has_colour = hasattr(binding.Context, "tsdf_color_enable")
    legs = [("plain", False)] + ([("colour", True)] if has_colour else [])
    ctxs = {}
    for name, colour in legs:
        ctxs[name] = scene_context(colour)
    c0, poses, napp = ctxs["plain"]
    copy_GBs, triad_GBs = c0.hbm_calibrate(1 << 28, 10)
    # the lanes (aligned groups of four voxels) that update a voxel, per pose: from the weights either side of one integration, while they still grow
    lanes, updated = [], []
    for p in poses:
        w0 = c0.tsdf_get()[1]
        c0.tsdf_integrate_frame(FID, p, K, 0.5, 20.0)
        up = (c0.tsdf_get()[1] != w0).reshape(-1, 4)
        lanes.append(int(up.any(1).sum()))
        updated.append(int(up.sum()))
        assert updated[-1] == c0.tsdf_last()["updated"]
    c0.tsdf_reset()
    # ---- (a) integration
    wall = {n: [] for n, _ in legs}
    for n, _ in legs:
        ctxs[n][0].profile_enable(True)
        ctxs[n][0].profile_select("tsdf_integrate")
    for k in range(a.warmup + a.reps):
        order = legs if k % 2 == 0 else legs[::-1]
        for n, _ in order:
            c = ctxs[n][0]
            if k == a.warmup:
                c.sync()
                c.profile_reset()
            c.sync()
            t0 = time.perf_counter()
            c.tsdf_integrate_frame(FID, poses[k % N_POSES], K, 0.5, 20.0)
            c.sync()
            if k >= a.warmup:
                wall[n].append((time.perf_counter() - t0) * 1e6)
    st = c0.tsdf_last()
    ra = {"part": "integrate", "tag": a.tag, "dense_points": napp, "visited": st["visited"], "updated_per_pose": updated, "lanes_with_an_update_per_pose": lanes,
          "copy_GBs": copy_GBs, "triad_GBs": triad_GBs}
    for n, _ in legs:
        c = ctxs[n][0]
        ra[n + "_kernel_us"] = stats(np.asarray(c.profile_samples("tsdf_integrate"), np.float64))
        ra[n + "_call_us"] = stats(wall[n])
        c.profile_enable(False)
    if has_colour:
        ra["colour_volume_bytes"] = 96 * float(np.mean(lanes))
        ra["colour_plane_bytes"] = 4 * W * H
        extra_us = ra["colour_kernel_us"]["median"] - ra["plain_kernel_us"]["median"]
        ra["extra_kernel_us"] = extra_us
        ra["colour_volume_GBs_at_extra"] = ra["colour_volume_bytes"] / extra_us * 1e-3 if extra_us > 0 else None
    # ---- (b) the mesh, left on the device
    wall = {n: [] for n, _ in legs}
    counts = {}
    for n, _ in legs:
        ctxs[n][0].profile_enable(True)
        ctxs[n][0].profile_select("tsdf_mesh")
    for k in range(a.warmup + a.reps):
        order = legs if k % 2 == 0 else legs[::-1]
        for n, colour in order:
            c = ctxs[n][0]
            if k == a.warmup:
                c.sync()
                c.profile_reset()
            c.sync()
            t0 = time.perf_counter()
            counts[n] = c.tsdf_mesh(1.0, download=False, colour=True) if colour else c.tsdf_mesh(1.0, download=False)
            if k >= a.warmup:
                wall[n].append((time.perf_counter() - t0) * 1e6)
    rb = {"part": "mesh", "tag": a.tag, "vertices": counts["plain"][0], "triangles": counts["plain"][1], "copy_GBs": copy_GBs}
    for n, _ in legs:
        c = ctxs[n][0]
        rb[n + "_kernel_us"] = stats(np.asarray(c.profile_samples("tsdf_mesh"), np.float64))
        rb[n + "_call_us"] = stats(wall[n])
        c.profile_enable(False)
    if has_colour:
        assert counts["colour"] == counts["plain"]
        rb["colour_bytes"] = 28 * counts["plain"][0]
        extra_us = rb["colour_kernel_us"]["median"] - rb["plain_kernel_us"]["median"]
        rb["extra_kernel_us"] = extra_us
        rb["colour_GBs_at_extra"] = rb["colour_bytes"] / extra_us * 1e-3 if extra_us > 0 else None
    for r, what in ((ra, "tsdf_integrate"), (rb, "tsdf_mesh     ")):
        for n, _ in legs:
            print("%s %-6s [%s] kernel median %.1f us (p95 %.1f), call median %.1f us (p95 %.1f)" % (
                what, n, a.tag, r[n + "_kernel_us"]["median"], r[n + "_kernel_us"]["p95"], r[n + "_call_us"]["median"], r[n + "_call_us"]["p95"]))
    print("copy rate %.0f GB/s; %d voxels visited, %s updated in %s lanes per pose; mesh %d vertices, %d triangles" % (
        copy_GBs, st["visited"], updated, lanes, counts["plain"][0], counts["plain"][1]))
    print(json.dumps(ra))
    print(json.dumps(rb))
    for n, _ in legs:
        ctxs[n][0].close()


if __name__ == "__main__":
    main()
