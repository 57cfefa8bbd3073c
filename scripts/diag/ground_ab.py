"""The ground choice of setCoarseTrackingRef (CoarseTracker.cpp:582-625, 669-693) two ways in one process, the legs alternating call by call: wall time of a leg
from its first call to its last byte on the host, medians with p10 / p90 over --calls calls per leg

  device  nalo_trk_fit_ground (with the marking of the window's points where there is a window)
  host    what a caller did before that call: nalo_trk_fit_planes + nalo_plane_fit_members + nalo_trk_get_pc (+ nalo_ba_get_residuals and
          nalo_ba_get_point_history for the marking) + the choice and the marking in NumPy (tests/ground_model.py, its vectorised forms)

at 1224x368 on the level-0 cloud nalo_trk_set_ref_from_window builds from a 7-frame window (with marking), and on the 160 k-point cloud of
plane_cases.large_scene at 1920x1072 (no window: the choice alone; the ordered mid_z sum of its largest cluster is the serial part). append = 0, so every call
sees the same cloud. Both legs must give the same pick and flags. Then the ground pass' own time: the "ground_pass" scope of nalo_profile_* (score + choice +
paint + mark + clear, one bracket), over 50 more calls."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
import ground_model as gm  # noqa: E402
import plane_cases as pc  # noqa: E402
import plane_model as pm  # noqa: E402
from nalo_slam_amd import binding, synth  # noqa: E402

F = np.float32


def setup(name):
    if name == "kitti00":
        w, h, W = 1224, 368, 7
        win = synth.make_window(w=w, h=h, W=W, P=2000, seed=41)
        mask = pc.block_mask(w, h, 3, 2, [210.0, 7.0, 3.0, 255.0, 220.0, 230.0])
        c = binding.Context(w, h, win.K, n_slots=W)
        for i in range(W):
            c.frame_upload(i, win.images[i], mask=mask if i == W - 1 else None)
        c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003))
        c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
        c.ba_set_residuals(win.exists)
        c.ba_set_point_history()
        c.ba_optimize(4)
        c.trk_set_ref_from_window()
        return c, win.K, len(win.host)
    sc = pc.large_scene()
    c = binding.Context(sc["w"], sc["h"], sc["K"], n_slots=1)
    c.frame_upload(0, np.random.RandomState(0).uniform(0, 255, (sc["h"], sc["w"])).astype(F), mask=sc["mask"])
    c.trk_set_pc(0, 0, sc["u"], sc["v"], sc["idp"], np.full(len(sc["u"]), 100, F))
    return c, sc["K"], 0


def run(name, calls):
    c, K, P = setup(name)
    draws = pm.make_draws(9)
    mark = P > 0

    def device_leg():
        recs, n, pick, scores, on = c.trk_fit_ground(draws, mark=mark, n_points=P)
        return (pick.ran, pick.cluster, list(pick.gp_raw), pick.ground_height, pick.n_ground_points), on

    def host_leg():
        recs, n = c.trk_fit_planes(draws, min_points=20)
        u, v, idp, _ = c.trk_get_pc(0)
        _, order = c.plane_fit_members(len(u), int(recs["n"].sum()))
        clusters, off = [], 0
        for r in recs:
            mem = order[off:off + r["n"]].astype(np.int64)
            off += r["n"]
            clusters.append(dict(members=mem, xx=u[mem].astype(np.int64), yy=v[mem].astype(np.int64), mask_value=r["mask_value"], n=int(r["n"]), n_cloud=int(r["n_cloud"]),
                                 fitted=int(r["fitted"]), plane=r["plane"]))
        want = gm.choose(clusters, idp, K, fast=True)
        on, num = None, 0
        if mark:
            st, _, _, _, cp = c.ba_get_residuals()
            _, lt, ls = c.ba_get_point_history()
            W = c.W
            tested = (lt[:, 0] == W - 1) & (ls[:, 0] == 0) & (st[:, W - 1] == 0)
            on, num = gm.mark_fast(want["g_u"], want["g_v"], tested, cp[:, W - 1, 0], cp[:, W - 1, 1])
        gh = want["ground_height"]
        return (want["ran"], want["cluster"], [float(x) for x in want["gp_raw"]], float(gh) if gh is not None else None, num), on

    t = {"host": [], "device": []}
    out = {}
    for k in range(calls + 2):
        for leg, fn in (("host", host_leg), ("device", device_leg)) if k % 2 == 0 else (("device", device_leg), ("host", host_leg)):
            c.sync()
            t0 = time.perf_counter()
            out[leg] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 2:
                t[leg].append(dt)
    assert out["host"][0] == out["device"][0], (out["host"][0], out["device"][0])
    assert (out["host"][1] is None and out["device"][1] is None) or np.array_equal(out["host"][1], out["device"][1])
    recs, _ = c.trk_fit_planes(draws, min_points=20)
    u = c.trk_get_pc(0)[0]
    print("%s: cloud %d points, %d clusters (largest %d), %d window points, pick %s" % (name, len(u), len(recs), int(recs["n"].max()), P, out["device"][0]))
    for leg in ("host", "device"):
        a = np.array(t[leg])
        print("  %-6s median %8.3f ms  p10 %8.3f  p90 %8.3f  (%d calls)" % (leg, np.median(a), np.percentile(a, 10), np.percentile(a, 90), len(a)))
    tp = []
    for _ in range(calls):
        t0 = time.perf_counter()
        c.trk_fit_planes(draws, min_points=20)
        tp.append((time.perf_counter() - t0) * 1e3)
    print("  nalo_trk_fit_planes alone: median %8.3f ms" % np.median(tp))
    c.profile_enable(True)
    c.profile_select("ground_pass")
    c.profile_reset()
    for _ in range(50):
        device_leg()
    c.sync()
    s = c.profile_samples("ground_pass")
    print("  ground_pass scope (score + choice%s): median %8.1f us  p10 %8.1f  p90 %8.1f  (%d brackets)" %
          (" + paint + mark + clear" if mark else "", np.median(s), np.percentile(s, 10), np.percentile(s, 90), len(s)))
    c.profile_enable(False)
    c.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    for name in ("kitti00", "cloud160k"):
        if a.only in (None, name):
            run(name, a.calls)
