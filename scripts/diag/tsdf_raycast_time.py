"""nalo_tsdf_raycast at the KITTI shape: the volume of tests/test_tsdf_gpu.py's chain (1224x368, W = 8, three keyframes fused into 256x64x256 voxels) seen from
the last keyframe's pose in a 1224x368 view, N = 251 samples a ray over the chain's depth range. One process, the legs alternating inside every repetition:

  depth                      nalo_tsdf_raycast with the depth image downloaded
  depth + normals            the same with the normal image
  depth + normals + colour   the same with the colour image (colour is enabled behind the chain, so the planes hold zeros: the loads are the same)
  mesh + download            nalo_tsdf_mesh with both host arrays, one call: the only other route to an image of the model - the TRANSFER ONLY, the CPU
                             rasterisation that would follow it is NOT timed

Per leg the whole call (wall clock, with the download) and the scope tsdf_raycast (the kernel, HIP events), median and p95. Beside them: the samples the rays
visit per second (from the conservative interval's start to the hit, or the whole interval for a ray that misses; the interval is worked out here in numpy as the
kernel works it out), and the floor the kernel cannot beat - the bytes of tsdf and weight inside the view's frustum box (nalo_tsdf_frustum_box) over the rate
nalo_hbm_calibrate copies at in the same run. The volume (34 MB) fits the Infinity Cache and repeated calls keep it warm.

Prints a table and one JSON line; --log appends both to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
from tsdf_ab import F, stats  # noqa: E402  (loads the package)

from nalo_slam_amd import binding  # noqa: E402


def chain_context():
    """run the chain with its context kept open: (context, the volume's descriptor, pose, K, min_depth, max_depth of the last keyframe's integration)"""
    import test_tsdf_gpu as tg
    got = {}
    close, integrate, create = binding.Context.close, binding.Context.tsdf_integrate_frame, binding.Context.tsdf_create

    def create_and_note(self, origin, voxel_size, dims, trunc, max_weight):
        got["desc"] = binding.tsdf_desc(origin, voxel_size, dims, trunc, max_weight)
        return create(self, origin, voxel_size, dims, trunc, max_weight)

    def integrate_and_note(self, fid, T, K, mn, mx):
        got.update(c=self, T=np.asarray(T, np.float64), K=tuple(float(k) for k in K), mn=float(mn), mx=float(mx))
        return integrate(self, fid, T, K, mn, mx)

    binding.Context.close, binding.Context.tsdf_integrate_frame, binding.Context.tsdf_create = (lambda self: None), integrate_and_note, create_and_note
    try:
        tg.run_chain(True)
    finally:
        binding.Context.close, binding.Context.tsdf_integrate_frame, binding.Context.tsdf_create = close, integrate, create
    return got["c"], got["desc"], got["T"], got["K"], got["mn"], got["mx"]


def interval(desc, w, h, K, T, mn, st, N):
    """the kernel's conservative interval [n0, n1] per pixel (n0 > n1: empty), in float64 as the kernel computes it"""
    R, t = T[:, :3].astype(F), T[:, 3].astype(F)
    fx, fy, cx, cy = (F(k) for k in K)
    vv, uu = np.mgrid[0:h, 0:w]
    rx, ry = (uu.astype(F) - cx) / fx, (vv.astype(F) - cy) / fy
    zl = float(F(mn)) + (N - 1) * float(F(st))
    zlo, zhi = np.full((h, w), -1e300), np.full((h, w), 1e300)
    for a in range(3):
        d = ((R[a, 0] * rx + R[a, 1] * ry) + R[a, 2]).astype(np.float64)
        o, g, vs, n = float(t[a]), float(desc.origin[a]), float(desc.voxel_size), desc.dims[a]
        m = vs + 1e-5 * (abs(o) + abs(g) + np.abs(d) * zl + n * vs)
        lo, hi = g + 0.5 * vs - m, g + (n - 0.5) * vs + m
        with np.errstate(all="ignore"):
            z1, z2 = (lo - o) / d, (hi - o) / d
        zlo, zhi = np.maximum(zlo, np.minimum(z1, z2)), np.minimum(zhi, np.maximum(z1, z2))
    n0 = np.clip(np.floor((zlo - mn) / st) - 2, 0, None)
    n1 = np.clip(np.ceil((zhi - mn) / st) + 2, None, N - 1)
    return n0, n1


def mesh_call(c, capv, capt, xyz, tri):
    a = binding.TsdfMeshArgs()
    a.min_weight, a.cap_vertices, a.cap_triangles = 1.0, capv, capt
    a.xyz, a.tri = xyz.ctypes.data_as(binding.c_fp), tri.ctypes.data_as(binding.c_ip)
    assert c.L.nalo_tsdf_mesh(c.h_, C.byref(a)) == 0
    return int(a.n_vertices), int(a.n_triangles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    c, made, T, K, mn, mx = chain_context()
    c.tsdf_color_enable()
    w, h = 1224, 368
    st = (mx - mn) / 250.0
    N = binding.tsdf_raycast_steps(mn, mx, st)
    nx, ny, nz = made.dims
    copy_GBs, _ = c.hbm_calibrate(1 << 28, 10)
    legs = [("depth", False, False), ("depth_normals", True, False), ("depth_normals_colour", True, True)]
    nv, nt = c.tsdf_mesh(1.0, download=False)
    xyz, tri = np.zeros((nv + 1024, 3), F), np.zeros((nt + 1024, 3), np.int32)
    wall = {name: [] for name, _, _ in legs}
    wall["mesh_download"] = []
    counts = {}
    for k in range(a.warmup + a.reps):
        for name, nrm, col in legs:
            c.sync()
            t0 = time.perf_counter()
            r = c.tsdf_raycast(w, h, K, T, mn, mx, st, 1.0, nrm, col)
            dt = time.perf_counter() - t0
            counts[name] = (r["n_hit"], r["n_back"], r["n_normal"])
            if k >= a.warmup:
                wall[name].append(dt * 1e6)
        c.sync()
        t0 = time.perf_counter()
        assert mesh_call(c, len(xyz), len(tri), xyz, tri) == (nv, nt)
        if k >= a.warmup:
            wall["mesh_download"].append((time.perf_counter() - t0) * 1e6)
    scope = {}
    c.profile_enable(True)
    c.profile_select("tsdf_raycast")
    for name, nrm, col in legs:
        for k in range(a.warmup + a.reps):
            if k == a.warmup:
                c.sync()
                c.profile_reset()
            c.tsdf_raycast(w, h, K, T, mn, mx, st, 1.0, nrm, col, download=False)
        c.sync()
        scope[name] = stats(np.asarray(c.profile_samples("tsdf_raycast"), np.float64))
    c.profile_enable(False)
    # the samples the rays visit, and the floor
    depth = r["depth"]
    n0, n1 = interval(made, w, h, K, T, mn, st, N)
    with np.errstate(all="ignore"):
        n_hit = np.ceil((depth.astype(np.float64) - mn) / st)
    last = np.where(depth > 0, np.minimum(n_hit, n1), n1)
    visited = float(np.clip(last - n0 + 1, 0, None).sum())
    lo, hi = binding.tsdf_frustum_box(made, w, h, K, T, mx)
    box_vox = int(np.prod([hi[k] - lo[k] for k in range(3)]))
    floor_us = 8.0 * box_vox / (copy_GBs * 1e3)
    out = {"part": "tsdf_raycast", "view": [w, h], "dims": [nx, ny, nz], "N": N, "counts": counts, "scope_us": scope, "call_us": {k: stats(v) for k, v in wall.items()},
           "samples_visited": visited, "Gsamples_per_s": {k: visited / s["median"] * 1e-3 for k, s in scope.items()}, "copy_GBs": copy_GBs, "frustum_box_voxels": box_vox,
           "floor_us": floor_us, "mesh": [nv, nt]}
    lines = ["tsdf_raycast %dx%d over %dx%dx%d, N = %d: hit / back / normal %s" % (w, h, nx, ny, nz, N, counts["depth_normals"]),
             "  copy rate %.0f GB/s; tsdf + weight inside the frustum box: %d voxels = %.1f MB -> floor %.1f us; samples visited %.3g a call" % (
                 copy_GBs, box_vox, 8e-6 * box_vox, floor_us, visited)]
    for name, _, _ in legs:
        s, cl = scope[name], stats(wall[name])
        lines.append("  %-22s scope median %.1f us (p95 %.1f) = %.2f G samples/s, %.1f x the floor; call with the download median %.1f us (p95 %.1f)" % (
            name, s["median"], s["p95"], out["Gsamples_per_s"][name], s["median"] / floor_us, cl["median"], cl["p95"]))
    m = stats(wall["mesh_download"])
    lines.append("  %-22s nalo_tsdf_mesh with both host arrays (%d vertices, %d triangles), transfer only, the CPU rasterisation is not timed: median %.1f us (p95 %.1f)" % (
        "mesh_download", nv, nt, m["median"], m["p95"]))
    lines.append(json.dumps(out))
    print("\n".join(lines))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
