"""The keyframe tail between optimize() and marginalizeFrame two ways in one process, the legs alternating per keyframe: wall time, medians and spread

  host     nalo_ba_get_residuals (W x P states) + nalo_ba_get_points (idepth, HdiF, Hdd) read back, flagPointsForRemoval in NumPy (vectorised, with the caller's
           own copy of numGoodResiduals / lastResiduals), nalo_ba_marginalize_points(flags) - which downloads, edits and uploads the [W][Ppad] state array
  device   nalo_ba_flag_points (per-host counts back, decisions resident) + nalo_ba_marginalize_flagged

on the headline window (1224x368, W = 8, 2000 points) and the 250 k-point window (1920x1072, W = 8). Every keyframe starts from the same state: snapshot restore,
linearizeAll(true) and its accumulation, untimed. The NumPy decision is measurement scaffolding (the tests compare against tests/lifecycle_model.py); the script
checks that both legs take the same decisions. Kernel by kernel: run this under rocprofv3 --kernel-trace --stats."""
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


def numpy_decision(host, st, idepth, Hdd, HdiF, prior, ff, ng, ls):
    n = (st >= 0).sum(1)
    vis = ((st == 0) & (ff[None, :] != 0)).sum(1)
    H = np.where(HdiF == 0, np.float32(0), np.maximum(Hdd + prior, np.float32(1e-10))).astype(np.float32)
    oob = ((n >= 3) & (ng > 14) & (n - vis < 3)) | (ls[:, 0] == 1) | ((n >= 2) & (ls[:, 0] == 2) & (ls[:, 1] == 2))
    nores = (idepth < 0) | (n == 0)
    out = (oob | (ff[host] != 0)) & ~nores
    marg = out & (n >= 3) & (ng >= 4) & (H > 50)
    return np.where(nores, 1, np.where(marg, 3, np.where(out, 2, 0))).astype(np.uint8)


def run(name, keyframes):
    s = SHAPES[name]
    win = synth.make_window(w=s["w"], h=s["h"], W=s["W"], P=s["P"], seed=7, n_extra=0)
    st6 = synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)
    W, P = win.W, len(win.host)
    c = binding.Context(win.w, win.h, win.K, n_slots=W)
    for i in range(W):
        c.frame_upload(i, win.images[i])
    c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=st6)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(win.exists)
    rng = np.random.RandomState(3)
    ng0 = rng.randint(0, 21, P).astype(np.int32)
    ls0 = rng.choice([0, 0, 0, 1, 2], (P, 2)).astype(np.int8)
    lt0 = np.tile(np.array([W - 1, W - 2], np.int8), (P, 1))
    c.ba_set_point_history(ng0, lt0, ls0)
    c.ba_optimize(6)
    c.ba_snapshot()
    ff = np.zeros(W, np.uint8); ff[[1, W - 2]] = 1
    prior = np.zeros(P, np.float32)
    st, idepth, HdiF, Hdd = np.zeros((P, W), np.int8), np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    cnt = np.zeros((W, 4), np.int32)
    i8, u8, F, I = C.POINTER(C.c_int8), binding._u8, binding._f, binding._i
    L, h = c.L, c.h_
    hist = {}

    def prep():
        c.ba_restore()
        c.ba_linearize(True)
        c.ba_get_points()
        hist["h"] = c.ba_get_point_history()                      # the host leg's own copy of the history (a running caller keeps it up to date itself)
        c.sync()

    def host_leg():
        c._ck(L.nalo_ba_get_residuals(h, st.ctypes.data_as(i8), None, None, None, None))
        c._ck(L.nalo_ba_get_points(h, F(idepth), None, F(HdiF), None, F(Hdd), None, None, None))
        dec = numpy_decision(win.host, st, idepth, Hdd, HdiF, prior, ff, hist["h"][0], hist["h"][2])
        c._ck(L.nalo_ba_marginalize_points(h, u8(np.ascontiguousarray(dec == 3, np.uint8)), None, None, None, None))
        return dec

    def device_leg():
        c._ck(L.nalo_ba_flag_points(h, u8(ff), None, None, I(cnt)))
        c._ck(L.nalo_ba_marginalize_flagged(h, None, None, None, None))
        return cnt.copy()
    legs = {"host": host_leg, "device": device_leg}
    names = list(legs)
    for k in names:
        for _ in range(3):
            prep(); legs[k]()
    ts = {k: [] for k in names}
    for i in range(keyframes):
        for j in range(2):
            k = names[(i + j) % 2]
            prep()
            t0 = time.perf_counter()
            legs[k]()
            c.sync()
            ts[k].append(time.perf_counter() - t0)
    prep()
    dec_h = host_leg()
    prior_h = c.ba_get_prior()
    prep()
    dec_d = c.ba_flag_points(ff)[0]
    cnt_d = device_leg()
    prior_d = c.ba_get_prior()
    same = np.array_equal(dec_h, dec_d) and np.array_equal(prior_h[0], prior_d[0]) and np.array_equal(np.bincount(dec_h, minlength=4), cnt_d.sum(0))
    print("%s: %d points, %d keyframes; decisions {keep, drop_nores, drop, marg} %s; both legs agree (decisions, HM bit for bit): %s"
          % (name, P, keyframes, np.bincount(dec_d, minlength=4).tolist(), same))
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
