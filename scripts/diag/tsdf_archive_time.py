"""nalo_tsdf_archive_mesh for the boxes of one shift, beside what a caller does today, on scripts/diag/tsdf_ab.py's scene: the 1224x368 frame fused with colour
from three poses into 256x128x256 voxels, and a shift whose x and z seam planes lie at the median voxel of the fused surface, so that every box of the shift
holds a part of it. One process, the legs alternating inside every repetition (wall clock of each, drained):

  archive         nalo_tsdf_archive_reset, then nalo_tsdf_archive_mesh of every box with no host array: mesh and append, everything stays on the device
  mesh            nalo_tsdf_mesh_color of the same boxes with no host array: the mesh part of the leg above; archive - mesh is the append part
  today           nalo_tsdf_mesh_color of the same boxes with all three host arrays given (sized from the counts plus a margin): the download the archive replaces;
                  the concatenation on the host that would follow is NOT timed, and it would leave the seams open

and, in a loop of their own, the scopes tsdf_mesh and tsdf_archive (the kernels of the mesh, and the key pass with the four append passes; HIP events), summed
over the boxes of a repetition. The table's load after the boxes is vertices over slots; probe lengths are not reported: the library keeps no counters, and a
diagnostic build with them was not made.

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


def cutting_shift(c):
    """a shift whose x and z seam planes lie at the median voxel of the fused surface (five voxels back in y)"""
    geo = c.tsdf_geometry()
    idx = np.floor((c.tsdf_surface_points(1.0).astype(np.float64) - geo["origin"].astype(np.float64)) / np.float64(geo["voxel_size"]))
    med = np.median(idx, axis=0)
    return (int(min(max(med[0], 1), DIMS[0] - 2)), -5, int(min(max(med[2], 1), DIMS[2] - 2)))


def mesh_color_call(c, box, min_weight, xyz, tri, rgba):
    a, cc = binding.TsdfMeshArgs(), binding.TsdfMeshColorArgs()
    a.use_box = 1
    a.lo[:], a.size[:] = box[0], box[1]
    a.min_weight = min_weight
    if xyz is not None:
        a.cap_vertices, a.cap_triangles, a.xyz, a.tri = len(xyz), len(tri), xyz.ctypes.data_as(binding.c_fp), tri.ctypes.data_as(binding.c_ip)
        cc.cap, cc.rgba = len(rgba), rgba.ctypes.data_as(binding.c_u8p)
    rc = c.L.nalo_tsdf_mesh_color(c.h_, C.byref(a), C.byref(cc))
    assert rc == 0, rc
    return int(a.n_vertices), int(a.n_triangles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--frames", type=int, default=3)
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
    c.tsdf_color_enable()
    c.tsdf_archive_enable()
    for p in poses:
        c.tsdf_integrate_frame(FID, p, K, 0.5, 20.0)
    SHIFT = cutting_shift(c)
    boxes = binding.tsdf_shift_boxes(DIMS, SHIFT)["boxes"]
    counts = [mesh_color_call(c, b, 1.0, None, None, None) for b in boxes]
    host = [(np.zeros((nv + 1024, 3), F), np.zeros((nt + 1024, 3), np.int32), np.zeros((nv + 1024, 4), np.uint8)) for nv, nt in counts]
    legs = {"archive": [], "mesh": [], "today": []}
    st = None
    for k in range(a.warmup + a.reps):
        c.tsdf_archive_reset()
        c.sync()
        t0 = time.perf_counter()
        for b in boxes:
            st = c.tsdf_archive_mesh(1.0, b)
        t1 = time.perf_counter()
        for b in boxes:
            mesh_color_call(c, b, 1.0, None, None, None)
        t2 = time.perf_counter()
        for b, (xyz, tri, rgba) in zip(boxes, host):
            mesh_color_call(c, b, 1.0, xyz, tri, rgba)
        t3 = time.perf_counter()
        if k >= a.warmup:
            for name, dt in zip(legs, (t1 - t0, t2 - t1, t3 - t2)):
                legs[name].append(dt * 1e6)
    scopes = {}
    for name in ("tsdf_mesh", "tsdf_archive"):
        c.profile_enable(True)
        c.profile_select(name)
        per_rep = []
        for k in range(a.warmup + a.reps):
            c.tsdf_archive_reset()
            c.sync()
            c.profile_reset()
            for b in boxes:
                c.tsdf_archive_mesh(1.0, b)
            c.sync()
            if k >= a.warmup:
                per_rep.append(float(np.sum(c.profile_samples(name))))
        c.profile_enable(False)
        scopes[name] = stats(per_rep)
    call = {name: stats(x) for name, x in legs.items()}
    append = stats(np.asarray(legs["archive"]) - np.asarray(legs["mesh"]))
    nv, nt = sum(n for n, _ in counts), sum(n for _, n in counts)
    r = {"part": "tsdf_archive", "dims": list(DIMS), "shift": list(SHIFT), "boxes": [[list(b[0]), list(b[1])] for b in boxes], "piece_vertices": nv, "piece_triangles": nt,
         "archive_vertices": st["n_vertices"], "archive_triangles": st["n_triangles"], "table_slots": st["table_slots"], "table_load": st["n_vertices"] / st["table_slots"],
         "call_us": call, "append_us": append, "kernels_us": scopes, "bytes_down_today": 12 * nv + 12 * nt + 4 * nv}
    lines = ["tsdf_archive %dx%dx%d, shift %s: %d boxes, %d piece vertices, %d triangles; the archive holds %d vertices behind them (%d welded), table load %.3f of %d slots" % (
        DIMS + (SHIFT, len(boxes), nv, nt, st["n_vertices"], nv - st["n_vertices"], r["table_load"], st["table_slots"]))]
    for name, label in (("archive", "nalo_tsdf_archive_mesh of every box, nothing leaves the device"), ("mesh", "nalo_tsdf_mesh_color of every box, no host array: the mesh part"),
                        ("today", "nalo_tsdf_mesh_color of every box with xyz, tri and rgba downloaded (%.2f MB)" % (r["bytes_down_today"] * 1e-6))):
        lines.append("  %-8s median %.1f us (p95 %.1f)   %s" % (name, call[name]["median"], call[name]["p95"], label))
    lines.append("  %-8s median %.1f us (p95 %.1f)   archive - mesh, repetition by repetition: the append part (key pass, lookup, scan, insert, triangles, one wait a box)" % (
        "append", append["median"], append["p95"]))
    lines.append("  %-8s median %.1f us (p95 %.1f)   today - mesh: the download part the append replaces" % (
        "download", *[stats(np.asarray(legs["today"]) - np.asarray(legs["mesh"]))[q] for q in ("median", "p95")]))
    for name in scopes:
        lines.append("  scope %-13s median %.1f us (p95 %.1f) summed over the boxes" % (name, scopes[name]["median"], scopes[name]["p95"]))
    lines.append(json.dumps(r))
    print("\n".join(lines))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
