"""setCoarseTrackingRef on the headline window, three ways in one process, alternating per keyframe: wall time per call + drain (medians)

  (a) nalo_trk_set_ref              the four input arrays in host memory (pinned staging + one H2D copy per call)
  (b) nalo_trk_set_ref_resident     the same arrays uploaded once before the loop (nalo_trk_ref_upload)
  (c) nalo_trk_set_ref_from_window  the inputs gathered on the device from the optimised window (no arrays at all)

Every keyframe is the headline step (bench.GpuJob.step: snapshot restore, three tracked frames, optimize(6)), which ends with the window's linearizeAll(true);
the three legs then run in a rotated order. The arrays of (a) and (b) are the window's own inputs in the reference's order, read back once, so all three legs
build the same reference (checked bit for bit at the end). The producer kernel's own time: run this under rocprofv3 --kernel-trace --stats."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=240)
args = ap.parse_args()

win, st6, trk = bench.make_inputs("kitti00_8kf")
job = bench.GpuJob(win, st6, trk, 0)
for _ in range(10):
    job.step(True)
c, L, W = job.ctx, job.ctx.L, win.W
# the window's inputs of makeCoarseDepthL0: IN residuals to frame W-1 in (host, submission) order
st, _, _, _, cp = c.ba_get_residuals()
hdi = c.ba_get_points()["HdiF"]
idx = np.nonzero(st[:, W - 1] == 0)[0]
idx = idx[np.argsort(win.host[idx], kind="stable")]
ref = [np.ascontiguousarray(a, np.float32) for a in (cp[idx, W - 1, 0], cp[idx, W - 1, 1], cp[idx, W - 1, 2], hdi[idx])]
import ctypes as C  # noqa: E402
ref_args = tuple(a.ctypes.data_as(C.POINTER(C.c_float)) for a in ref)
c.trk_ref_upload(*ref)
legs = {
    "a host arrays": lambda: L.nalo_trk_set_ref(c.h_, W - 1, len(ref[0]), *ref_args),
    "b resident": lambda: L.nalo_trk_set_ref_resident(c.h_, W - 1),
    "c from window": lambda: L.nalo_trk_set_ref_from_window(c.h_),
}
names = list(legs)
ts = {k: [] for k in names}
for i in range(args.keyframes):
    job.step(True)
    for j in range(3):
        k = names[(i + j) % 3]
        c.sync()
        t0 = time.perf_counter()
        c._ck(legs[k]())
        c.sync()
        ts[k].append(time.perf_counter() - t0)
print("headline window: %d inputs (%d points), %d keyframes, call + drain:" % (len(ref[0]), len(win.host), args.keyframes))
for k in names:
    t = np.array(ts[k]) * 1e6
    print("  %-14s median %6.1f us   p10 %6.1f   p90 %6.1f" % (k, np.median(t), np.percentile(t, 10), np.percentile(t, 90)), flush=True)
out = {}
for k in names:
    c._ck(legs[k]())
    out[k] = [c.trk_get_pc(l) + list(c.trk_get_depth(l)) for l in range(c.levels)]
same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for k in names[1:] for g, h in zip(out[names[0]], out[k]) for a, b in zip(g, h))
print("the three legs build the same reference bit for bit: %s" % same)
