"""nalo_tsdf_mesh at the KITTI shape, on scripts/diag/tsdf_ab.py's scene: the 1224x368 frame fused from four poses into 256x128x256 voxels. One process, the
legs alternating inside every repetition (wall clock of each, drained):

  mesh            nalo_tsdf_mesh with no host array: the mesh stays on the device (classify, two scans, vertices, triangles, one wait for the two totals)
  mesh + download ONE call with host arrays sized from the last counts plus a margin: the same, then the copy up and a second wait
  surface points  nalo_tsdf_surface_points with a cap: what the library published before the mesh
  read-back       nalo_tsdf_get of the whole volume, the route the mesh replaces: the TRANSFER ONLY - the CPU meshing that would follow it is NOT timed

and the scope tsdf_mesh (the four kernels of a call, HIP events) against the bytes the plan moves - 8 B per voxel read in each of the two passes over the volume,
5 B per voxel of scratch written and read, the output - over the rate nalo_hbm_calibrate copies at in the same run. The 67 MB volume and its 42 MB of scratch fit
the Infinity Cache and repeated calls keep them warm: the fraction says how the kernels compare with a streaming copy, not what HBM delivers. --big adds the scope on
a 640x256x512 volume (671 MB, beyond the cache) holding the same kind of surface.

Prints a table and one JSON line; --log appends both to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tsdf_ab import DIMS, FID, H, K, W, F, stats, street  # noqa: E402  (loads the package)

from nalo_slam_amd import binding  # noqa: E402


def mesh_call(c, min_weight, capv, capt, xyz, tri):
    a = binding.TsdfMeshArgs()
    a.min_weight = min_weight
    a.cap_vertices, a.cap_triangles = capv, capt
    a.xyz = None if xyz is None else xyz.ctypes.data_as(binding.c_fp)
    a.tri = None if tri is None else tri.ctypes.data_as(binding.c_ip)
    rc = c.L.nalo_tsdf_mesh(c.h_, C.byref(a))
    assert rc == 0, rc
    return int(a.n_vertices), int(a.n_triangles)


def scope(c, reps, warmup, min_weight):
    c.profile_enable(True)
    c.profile_select("tsdf_mesh")
    for k in range(warmup + reps):
        if k == warmup:
            c.sync()
            c.profile_reset()
        counts = c.tsdf_mesh(min_weight, download=False)
    c.sync()
    us = np.asarray(c.profile_samples("tsdf_mesh"), np.float64)
    c.profile_enable(False)
    return stats(us), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    mask, img, bgr, u, v, idp = street()
    c = binding.Context(W, H, K, n_slots=2)
    for s in range(2):
        c.frame_upload(s, img, mask=mask, bgr=bgr)
    c.ba_set_window([0, 1], np.tile(np.eye(3, 4), (2, 1, 1)), frame_ids=[FID, FID + 1])
    P = len(u)
    c.ba_set_points(np.zeros(P, np.int32), u, v, idp, np.full((P, 8), 100, F), np.ones((P, 8), F))
    c.map_dense_enable(True)
    draws = np.random.RandomState(1).randint(0, 2 ** 32, 150, dtype=np.uint64).astype(np.uint32)
    poses = [np.concatenate([np.eye(3), np.array([[0.05 * k], [0.0], [0.1 * k]])], 1) for k in range(a.frames)]
    c.dense_update_map(0, draws, poses[0])
    vs = max(20.0 / DIMS[0], 6.0 / DIMS[1], 14.0 / DIMS[2])
    c.tsdf_create((-0.5 * vs * DIMS[0], -0.5 * vs * DIMS[1], 1.0), vs, DIMS, 4 * vs, 64.0)
    for p in poses:
        c.tsdf_integrate_frame(FID, p, K, 0.5, 20.0)
    copy_GBs, _ = c.hbm_calibrate(1 << 28, 10)
    nvox = int(np.prod(DIMS))
    nv, nt = c.tsdf_mesh(1.0, download=False)
    n_pts = len(c.tsdf_surface_points(1.0))
    xyz, tri = np.zeros((nv + 1024, 3), F), np.zeros((nt + 1024, 3), np.int32)
    legs = {"mesh": [], "mesh_download": [], "surface_points": [], "get_volume": []}
    for k in range(a.warmup + a.reps):
        c.sync()
        t0 = time.perf_counter()
        assert c.tsdf_mesh(1.0, download=False) == (nv, nt)
        t1 = time.perf_counter()
        assert mesh_call(c, 1.0, len(xyz), len(tri), xyz, tri) == (nv, nt)
        t2 = time.perf_counter()
        assert len(c.tsdf_surface_points(1.0, cap=n_pts + 1024)) == n_pts
        t3 = time.perf_counter()
        c.tsdf_get()
        t4 = time.perf_counter()
        if k >= a.warmup:
            for name, dt in zip(legs, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                legs[name].append(dt * 1e6)
    ks, _ = scope(c, a.reps, a.warmup, 1.0)
    nbytes = (16 + 10) * nvox + 12 * nv + 12 * nt
    r = {"part": "tsdf_mesh", "dims": list(DIMS), "vertices": nv, "triangles": nt, "surface_points": n_pts, "kernels_us": ks,
         "call_us": {name: stats(v) for name, v in legs.items()}, "bytes_planned": nbytes, "GBs_at_median": nbytes / ks["median"] * 1e-3, "copy_GBs": copy_GBs,
         "fraction_of_copy_rate": nbytes / ks["median"] * 1e-3 / copy_GBs, "bytes_up_mesh": 12 * (nv + nt), "bytes_up_volume": 8 * nvox}
    lines = ["tsdf_mesh %dx%dx%d: %d vertices, %d triangles (%d surface points)" % (DIMS + (nv, nt, n_pts)),
             "  scope tsdf_mesh      median %.1f us (p95 %.1f): %.1f MB planned = %.0f GB/s = %.2f of the copy rate %.0f GB/s (volume and scratch warm in the Infinity Cache)" % (
                 ks["median"], ks["p95"], nbytes * 1e-6, r["GBs_at_median"], r["fraction_of_copy_rate"], copy_GBs)]
    for name, label in (("mesh", "mesh, left on the device"), ("mesh_download", "mesh + download, one call"), ("surface_points", "surface points, with a cap"),
                        ("get_volume", "nalo_tsdf_get, whole volume (transfer only; the CPU meshing behind it is not timed)")):
        s = stats(legs[name])
        lines.append("  %-16s median %.1f us (p95 %.1f)   %s" % (name, s["median"], s["p95"], label))
    if a.big:
        bd = (640, 256, 512)
        c.tsdf_create((-0.5 * vs * bd[0], -0.5 * vs * bd[1], 1.0), vs, bd, 4 * vs, 64.0)
        for p in poses:
            c.tsdf_integrate_frame(FID, p, K, 0.5, 20.0)
        kb, (bv, bt) = scope(c, max(a.reps // 3, 5), 2, 1.0)
        bvox = int(np.prod(bd))
        bbytes = 26 * bvox + 12 * bv + 12 * bt
        r["big"] = {"dims": list(bd), "vertices": bv, "triangles": bt, "kernels_us": kb, "bytes_planned": bbytes, "GBs_at_median": bbytes / kb["median"] * 1e-3,
                    "fraction_of_copy_rate": bbytes / kb["median"] * 1e-3 / copy_GBs}
        lines.append("  scope tsdf_mesh at %dx%dx%d (%.0f MB of volume, beyond the cache): median %.1f us (p95 %.1f), %d vertices, %d triangles: %.0f GB/s = %.2f of the copy rate" % (
            bd + (8e-6 * bvox, kb["median"], kb["p95"], bv, bt, r["big"]["GBs_at_median"], r["big"]["fraction_of_copy_rate"])))
    lines.append(json.dumps(r))
    print("\n".join(lines))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
