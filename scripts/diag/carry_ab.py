"""The keyframe turnover - the oldest frame leaves, the new keyframe enters - two ways in one process, the routes alternating per keyframe: wall time from the
first call of the turnover to a drained stream, medians and spread

  reissue  nalo_ba_get_points + nalo_ba_get_idepth_zero + nalo_ba_get_residuals (W x P states) read back, nalo_ba_marginalize_frame, nalo_ba_get_point_history +
           nalo_ba_get_frames, the residual graph and the history shifted in NumPy, nalo_ba_set_window + nalo_ba_set_points + nalo_ba_set_residuals +
           nalo_ba_set_point_history: what a caller did before nalo_ba_carry_window (tests/test_point_lifecycle_gpu.py's five-keyframe loop)
  carry    nalo_ba_marginalize_frame + nalo_ba_carry_window(entering)

on the headline window (1224x368, W = 8, 2000 points) and the 250 k-point window (1920x1072, W = 8). Every keyframe starts from the same state, built untimed: the
window issued from the host arrays (the oldest frame hosts no point, so it can leave at once), a history, one linearizeAll(true). The script checks that both
routes leave a window that linearises to the same energy, bit for bit. The carry kernel's own time: run this under rocprofv3 --kernel-trace --stats (row
ba_carry_kernel)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
from nalo_slam_amd import binding, synth  # noqa: E402

SHAPES = {"kitti00_8kf": dict(w=1224, h=368, W=8, P=2000), "stress250k": dict(w=1920, h=1072, W=8, P=250000)}


def run(name, keyframes):
    s = SHAPES[name]
    win = synth.make_window(w=s["w"], h=s["h"], W=s["W"], P=s["P"], seed=7, n_extra=1)
    st6 = synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)
    W = win.W
    keep = win.host != 0                                          # the frame that leaves hosts no point any more (they were marginalised or dropped before)
    host, u, v, idepth0, color, weights, exists0 = [np.ascontiguousarray(a[keep]) for a in (win.host, win.u, win.v, win.idepth, win.color, win.weights, win.exists)]
    P = len(host)
    c = binding.Context(win.w, win.h, win.K, n_slots=W + 1)
    for i in range(W + 1):
        c.frame_upload(i, win.images[i])
    entering = c.frame_state(W, win.world_to_cam[W], frame_id=W)
    host_new = (host - 1).astype(np.int32)
    L, h = c.L, c.h_
    i8 = C.POINTER(C.c_int8)
    st, idepth, idz = np.zeros((P, W), np.int8), np.zeros(P, np.float32), np.zeros(P, np.float32)
    ng, lt, ls = np.zeros(P, np.int32), np.zeros((P, 2), np.int8), np.zeros((P, 2), np.int8)
    ex = np.ones((P, W), np.uint8)
    cal = np.asarray(c.K, np.float64)

    def prep():
        c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=st6)
        c.ba_set_points(host, u, v, idepth0, color, weights)
        c.ba_set_residuals(exists0)
        c.ba_set_point_history()
        c.ba_linearize(True)
        c.ba_get_points()                                         # the accumulation of that pass, which a read-back would otherwise run on demand inside the timed leg
        c.sync()

    def reissue_leg():
        c._ck(L.nalo_ba_get_points(h, binding._f(idepth), None, None, None, None, None, None, None))
        c._ck(L.nalo_ba_get_idepth_zero(h, binding._f(idz)))
        c._ck(L.nalo_ba_get_residuals(h, st.ctypes.data_as(i8), None, None, None, None))
        c.ba_marginalize_frame(0)
        c._ck(L.nalo_ba_get_point_history(h, binding._i(ng), lt.ctypes.data_as(i8), ls.ctypes.data_as(i8)))
        frames = (binding.FrameState * W)()
        c._ck(L.nalo_ba_get_frames(h, frames, None, None))
        frames[W - 1] = entering
        ex[:, :W - 1] = st[:, 1:] >= 0                            # the residuals to the frames that remain; the column of the new keyframe stays 1
        lt[:, 1], ls[:, 1] = lt[:, 0], ls[:, 0]                  # FullSystem.cpp:1344-1345
        lt[:, 0], ls[:, 0] = W - 1, 0
        c._ck(L.nalo_ba_set_window(h, W, frames, binding._d(cal), binding._d(cal)))
        c.W = W
        c._ck(L.nalo_ba_set_points(h, P, binding._i(host_new), binding._f(u), binding._f(v), binding._f(idepth), binding._f(idz), binding._f(color), binding._f(weights), None))
        c._ck(L.nalo_ba_set_residuals(h, binding._u8(ex)))
        c._ck(L.nalo_ba_set_point_history(h, binding._i(ng), lt.ctypes.data_as(i8), ls.ctypes.data_as(i8)))

    def carry_leg():
        c.ba_marginalize_frame(0)
        c._ck(L.nalo_ba_carry_window(h, C.byref(entering), 0))
        c.W = W
    legs = {"reissue": reissue_leg, "carry": carry_leg}
    names = list(legs)
    for k in names:
        for _ in range(3):
            prep(); legs[k](); c.sync()
    ts = {k: [] for k in names}
    for i in range(keyframes):
        for j in range(2):
            k = names[(i + j) % 2]
            prep()
            t0 = time.perf_counter()
            legs[k]()
            c.sync()
            ts[k].append(time.perf_counter() - t0)
    E = {}
    for k in names:
        prep(); legs[k]()
        E[k] = (c.ba_linearize(False), c.ba_get_point_history()[1].tobytes(), c.ba_launch_config())
    same = np.float64(E["reissue"][0]).tobytes() == np.float64(E["carry"][0]).tobytes() and E["reissue"][1:] == E["carry"][1:]
    print("%s: %d points, %d keyframes per route; both routes leave the same window (energy bit for bit %.6e, history, launch configuration): %s"
          % (name, P, keyframes, E["carry"][0], same))
    for k in names:
        t = np.array(ts[k]) * 1e6
        print("  %-7s median %9.1f us   p10 %9.1f   p90 %9.1f" % (k, np.median(t), np.percentile(t, 10), np.percentile(t, 90)), flush=True)
    c.close()
    return same


ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=100)
ap.add_argument("--shapes", default="kitti00_8kf,stress250k")
args = ap.parse_args()
ok = all([run(s, args.keyframes) for s in args.shapes.split(",")])
sys.exit(0 if ok else 1)
