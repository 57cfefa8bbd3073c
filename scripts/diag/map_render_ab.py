"""The viewer's 3-D panel of one session state, two ways in one process, the legs alternating per call: wall time from the first call to the result on the host

  render   nalo_map_render: everything switched on (points of all listed frames, dense clouds, cameras, constraints, trajectories), a 640x480 RGB image and its
           depth up behind one wait (plus nalo_map_graph's count and wait for the constraints)
  clouds   the only route to the same vertices without it: one nalo_map_frame_cloud plus one nalo_map_dense_cloud per listed frame (15 bytes per vertex up, one
           wait each); the rasterisation on the CPU would come on top and is NOT measured

on the state tests/test_map_render_gpu.py builds for its full-size case: three keyframes of the device chain at 1224x368, W = 8, the archive, the dense archive and the
graph on, 10 listed frames. A second pass runs with the library's profile brackets on and prints the scopes map_render_points / map_render_lines / map_render_resolve
(device events around each launch) three times: with the start view; with the same view and the principal point moved far off the image, where every vertex still
goes through the depth range, the two divisions and the viewport test but none is drawn, so the point pass issues no atomic; and with a view that looks away from the
map, where a vertex already fails the depth range, before the divisions. The differences between the three point passes are the atomics and the projection."""
import argparse
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
import render_model as rm  # noqa: E402
import test_map_render_gpu as t  # noqa: E402


def stats(name, a):
    a = np.asarray(a)
    if not len(a):                                                             # a scope without a launch (no segment with a sample: no line kernel)
        print("  %-22s no launch" % name, flush=True)
        return float("nan")
    print("  %-22s median %9.1f us   p95 %9.1f   (n = %d)" % (name, np.median(a), np.percentile(a, 95), len(a)), flush=True)
    return float(np.median(a))


ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=60)
args = ap.parse_args()
(c,), win, frames, recs, dense, conn = t.chain(1224, 368, 8, 3, 8000, 6000)
frames = [(f, np.concatenate([m[:, :3], m[:, 3:] * 2000], 1)) for f, m in frames]        # the corridor's cameras are 3e-4 apart: spread them as the test does
view = rm.look_at((1.0, -3.0, -8.0), (0, 0, 4.0), (0, -1, 0))
away = rm.look_at((1.0, -3.0, -8.0), (2.0, -6.0, -20.0), (0, -1, 0))
poses = np.stack([m[:, 3] for _, m in frames]).astype(np.float32)
kw = dict(display_mode=1, with_dense=True, show_kf_cams=True, current_cam=frames[-1][1], show_active_constraints=True, show_all_constraints=True, show_trajectory=True,
          all_poses=poses)
box = {}


def render():
    box["r"] = c.map_render(640, 480, view, frames, **kw)


def clouds():
    n = 0
    for f, _ in frames:
        n += len(c.map_frame_cloud(f, 1, 1e10, 1e10, 0.0)["xyz"])
        if f in dense:
            n += len(c.map_dense_cloud(f)["xyz"])
    box["n"] = n


ts = {"render": [], "clouds": []}
for i in range(args.calls + 1):                                                # call 0 is the warm-up (first-use allocations), not timed
    c.sync()
    for k in (("render", "clouds") if i % 2 == 0 else ("clouds", "render")):
        t0 = time.perf_counter()
        (render() if k == "render" else clouds())
        if i > 0:
            ts[k].append((time.perf_counter() - t0) * 1e6)
r = box["r"]
n_rec = sum(len(v) for v in recs.values()) + sum(len(v) for v in dense.values())
# the virtual list the point pass walks: the resident immature set once, the window's point slots, every archive run twice (once per status), the dense pieces
n_list = 6000 + len(c.ba_get_points()["idepth"]) + 2 * sum(len(c.map_get_frame(f)) for f, _ in frames) + sum(len(v) for v in dense.values())
print("map_render_ab: 1224 x 368, W = 8, 3 keyframes, %d listed frames, %d records (%d dense), view 640 x 480, %d calls per leg" %
      (len(frames), n_rec, sum(len(v) for v in dense.values()), args.calls))
print("  the point pass' list: %d entries, %d workgroups of 256 lanes" % (n_list, (n_list + 255) // 256))
print("  vertices %d (the clouds route fetched %d), drawn %d, segments %d, line samples %d" % (r["n_vertices"], box["n"], r["n_drawn_points"], r["n_segments"], r["n_line_samples"]))
print("  bytes up, render: %d (rgb) + %d (depth) + 32 (counts); clouds: %d (15 per vertex)" % (3 * 640 * 480, 4 * 640 * 480, 15 * box["n"]))
stats("render", ts["render"])
stats("clouds", ts["clouds"])
c.profile_enable(True)
pts = {}
for name, v, extra in (("start view", view, {}), ("start view, principal point off the image", view, dict(cx=1e6)), ("view looking away", away, {})):
    c.profile_reset()
    for i in range(args.calls):
        g = c.map_render(640, 480, v, frames, **dict(kw, **extra))
    c.sync()
    print(" %s: drawn %d of %d vertices, %d line samples" % (name, g["n_drawn_points"], g["n_vertices"], g["n_line_samples"]))
    med = {s: stats(s, c.profile_samples(s)) for s in ("map_render_points", "map_render_lines", "map_render_resolve")}
    pts[name] = med["map_render_points"]
    print("  point pass: %.2f G list entries/s, %.2f G vertices/s" % (n_list / med["map_render_points"] * 1e-3, g["n_vertices"] / med["map_render_points"] * 1e-3))
a, b, d = (pts[k] for k in ("start view", "start view, principal point off the image", "view looking away"))
print(" point pass, start view minus principal point off the image (the %d atomics of 8 bytes): %.1f us = %.2f G atomics/s" % (r["n_drawn_points"], a - b, r["n_drawn_points"] / max(a - b, 1e-9) * 1e-3))
print(" point pass, principal point off the image minus looking away (two divisions, the projection and the viewport test per vertex): %.1f us" % (b - d))
c.profile_enable(False)
ok = r["n_vertices"] == box["n"]
print("  both routes count the same vertices: %s" % ok)
c.close()
sys.exit(0 if ok else 1)
