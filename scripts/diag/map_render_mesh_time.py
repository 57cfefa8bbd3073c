"""nalo_map_render_mesh on the state tests/test_map_render_mesh_gpu.py builds for its chain case (three keyframes at 1224x368 fused into a coloured 256x64x256
volume that follows the camera, the leaving boxes in the welded archive, the grid's coloured mesh on the device), measured in one process:

  call      wall time of the whole call (archive + live mesh, no points) from the first enqueue to the picture on the host, at 306x92 and at 1224x368
  pass      the triangle pass alone: the profile scope map_render_tris (device events around the launch), per source and for all sources in ONE launch against the
            sum of one launch per source (three calls with one source each) - the choice "one launch over a small source table"; and for two caller's meshes
            that fill the view, a sheet of 1024 x 512 vertices (1.05 M triangles of a pixel or less: the lane path) and one of 33 x 17 (1024 triangles with
            boxes of hundreds of pixels: the wave path)
  route     what the call replaces: nalo_tsdf_archive_get plus the download of the device mesh (xyz, tri, rgba), wall time and bytes; the rasterisation on the CPU
            would come on top and is NOT measured
  bytes     the pass' compulsory bytes (12 per triangle of indices, 16 per vertex of position and colour, 8 per candidate's atomic) per second against
            nalo_hbm_calibrate's copy rate from the same run

--lib PATH loads another build of the library (a kMrLaneBox variant) for the threshold comparison; the picture must not depend on it, so its bytes are hashed."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--lib", default=None)
args = ap.parse_args()
from nalo_slam_amd import binding  # noqa: E402

if args.lib:
    binding.lib_path = lambda: os.path.abspath(args.lib)
import torch  # noqa: E402

import render_model as rm  # noqa: E402
import test_map_render_mesh_gpu as t  # noqa: E402


def med(name, a, unit="us"):
    a = np.asarray(a, np.float64)
    print("  %-44s median %10.1f %s   p95 %10.1f   (n = %d)" % (name, np.median(a), unit, np.percentile(a, 95), len(a)), flush=True)
    return float(np.median(a))


def wall(fn, n):
    out = []
    for i in range(n + 1):                                                      # call 0 is the warm-up (first-use allocations), not timed
        c.sync()
        t0 = time.perf_counter()
        fn()
        if i:
            out.append((time.perf_counter() - t0) * 1e6)
    return out


state = None
gen = t.chain_keyframes()
for state in gen:
    if state[0] == 2:                                                           # the last keyframe: the generator stays suspended, its context open
        break
kf, c, view, frames = state
print("map_render_mesh_time: library %s" % binding.lib_path())
st = c.tsdf_archive_stats()
mv = c.tsdf_mesh_view()
nv_live, nt_live = mv[0].shape[0], mv[1].shape[0]
print("  archive %d vertices %d triangles; live mesh (the whole 256x64x256 grid) %d vertices %d triangles" % (st["n_vertices"], st["n_triangles"], nv_live, nt_live))
copy_rate, _ = c.hbm_calibrate()
print("  nalo_hbm_calibrate: copy %.0f GB/s" % copy_rate)
user = tuple(torch.as_tensor(v, device="cuda").clone() for v in mv + (c.tsdf_mesh_color_view(),))      # the live mesh again as a caller's mesh: a third source of the same size


def sheet(nx, ny, f, vw, vh):
    """a slanted height field of nx x ny vertices that fills the view (world coordinates; 2 (nx - 1) (ny - 1) triangles), as a caller's mesh on the device"""
    V = np.asarray(view, np.float64).reshape(3, 4)
    u, v = np.meshgrid(np.linspace(1.0, vw - 2.0, nx), np.linspace(1.0, vh - 2.0, ny))
    z = 2.0 + 3.0 * v / vh + 0.05 * np.sin(0.7 * u) * np.cos(0.9 * v)
    p = np.stack([(u - vw / 2) / f * z, (v - vh / 2) / f * z, z], -1).reshape(-1, 3)
    xyz = ((p - V[:, 3]) @ V[:, :3]).astype(np.float32)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1)
    tri = np.concatenate([np.stack([i, i + 1, i + nx + 1], 1), np.stack([i, i + nx + 1, i + nx], 1)]).astype(np.int32)
    rgba = np.random.RandomState(1).randint(0, 256, (len(xyz), 4)).astype(np.uint8)
    return tuple(torch.from_numpy(a).cuda() for a in (xyz, tri, rgba)), len(xyz)



c.profile_enable(True)
c.profile_select("map_render_tris")
digest = hashlib.sha256()
for vw, vh, f in ((306, 92, 110.0), (1224, 368, 440.0)):
    kw = dict(fx=f, fy=f, display_mode=3)
    print(" view %d x %d" % (vw, vh))
    res = {}
    fine, nv_fine = sheet(1024, 512, f, vw, vh)                                # 1.05 M triangles of about a pixel (1224x368) or less (306x92): every box stays with its lane
    coarse, nv_coarse = sheet(33, 17, f, vw, vh)                               # 1024 triangles with boxes of hundreds of pixels: every box goes to the wave
    for name, src, nv in (("archive", dict(archive=True), st["n_vertices"]), ("live mesh", dict(live=True), nv_live), ("user (the live mesh's arrays)", dict(mesh=user), nv_live),
                          ("archive + live mesh", dict(archive=True, live=True), st["n_vertices"] + nv_live),
                          ("all three in one launch", dict(archive=True, live=True, mesh=user), st["n_vertices"] + 2 * nv_live),
                          ("a sheet of 1024 x 512 vertices", dict(mesh=fine), nv_fine), ("a sheet of 33 x 17 vertices", dict(mesh=coarse), nv_coarse)):
        for mode in (0, 1):
            c.profile_reset()
            box = {}

            def run():
                box["g"] = c.map_render_mesh(vw, vh, view, colour_mode=mode, **src, **kw)

            w = wall(run, args.calls)
            g = box["g"]
            digest.update(g["rgb"].tobytes() + g["depth"].tobytes())
            print("  %s, colour_mode %d: %d triangles, %d candidates; near %d guard %d degenerate %d large %d" %
                  (name, mode, g["n_triangles"], g["n_tri_pixels"], g["n_tri_near"], g["n_tri_guard"], g["n_tri_degenerate"], g["n_tri_large"]))
            med("whole call (wall)", w)
            p = med("map_render_tris (device)", c.profile_samples("map_render_tris")[1:])
            res[(name, mode)] = p
            nbytes = 12 * g["n_triangles"] + 16 * nv + 8 * g["n_tri_pixels"]
            print("  %-44s %.1f MB compulsory -> %.1f GB/s = %.1f %% of the copy rate; %.2f G triangles/s" %
                  ("", nbytes * 1e-6, nbytes / p * 1e-3, 100.0 * nbytes / p * 1e-3 / copy_rate, g["n_triangles"] / p * 1e-3))
    for mode in (0, 1):
        one = res[("all three in one launch", mode)]
        three = res[("archive", mode)] + res[("live mesh", mode)] + res[("user (the live mesh's arrays)", mode)]
        print("  colour_mode %d: one launch over the source table %.1f us, one launch per source %.1f us (sum of the three)" % (mode, one, three))
c.profile_enable(False)
print(" the route the call replaces")


def route():
    c.tsdf_archive_get()
    [torch.as_tensor(v, device="cuda").cpu() for v in c.tsdf_mesh_view() + (c.tsdf_mesh_color_view(),)]


med("nalo_tsdf_archive_get + mesh download (wall)", wall(route, max(args.calls // 4, 5)))
print("  bytes up: %d (archive xyz, tri, rgba) + %d (device mesh); the call's: %d at 306x92, %d at 1224x368 (rgb + depth)" %
      (16 * st["n_vertices"] + 12 * st["n_triangles"], 16 * nv_live + 12 * nt_live, 7 * 306 * 92, 7 * 1224 * 368))
print(" sha256 of every picture above: %s" % digest.hexdigest())
gen.close()
