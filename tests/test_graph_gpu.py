"""The keyframe graph of the device chain - nalo_map_graph_enable / nalo_map_graph / nalo_map_graph_connections, EnergyFunctional::connectivityMap as
publishGraph receives it - against the literal model of tests/graph_model.py and against the library's own public read-backs. Every comparison is an
integer equality over ALL entries.

  1  live counts at the kernel's borders: W = 4 with hosts of 1, 65, 257 and 513 points (a wave border, a block border, several blocks per host, padding in
     every host's last block), a pair without a residual, a pair with exactly one, a host without any; W = 2; W = 16 with 40 points per host
  2  every way a residual disappears - the fix pass, the removal of all three classes of flagged points, a frame that leaves from the middle - and appears -
     the carry with an entering frame, the insertion of activated points, the window issued from the initialiser -, each against the count from nalo_ba_get_residuals; the refusal before any window
  3  marg against an independent route: a twin context evaluates every residual once more at the same state and the same resident frameEnergyTH, and
     nalo_ba_get_residuals' `active` of that pass is what marginalizePointsF's isActive() reads; both routes (before and after the fix pass), a second
     marginalisation that adds, nalo_ba_marginalize_points against nalo_ba_marginalize_flagged
  4  three keyframes of the device chain (W = 5, 1500 points, frame 0 leaves every keyframe, 5 + 3 frames seen), the model driven by read-backs and by one
     twin per keyframe (a replay of the chain up to that keyframe's publish point); nalo_map_reset
  5  the read-back route: the same session re-issued with nalo_ba_set_window + set_points + set_residuals and nalo_ba_marginalize_points gives the chain's graph
  6  opt-in without side effects, and the refusals

Case 5's route removes only the marginalised points in nalo_ba_marginalize_points; the caller drops the other two classes by re-issuing the window without
them, so its publish point is the re-issued window."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import graph_model as gm
import lifecycle_model as lm
import lifecycle_scenes as sc
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
LOW = 3e-4                                                      # the low-parallax corridor of tests/lifecycle_scenes.py


# ------------------------------------------------------------------------------------------------ helpers
def entries(c):
    return [tuple(int(x) for x in e) for e in c.map_graph()]


def connections(c):
    return [tuple(int(x) for x in e) for e in c.map_graph_connections()]


def act_of(c):
    return {(h, t): a for h, t, a, _ in entries(c)}


def marg_of(c):
    return {(h, t): m for h, t, _, m in entries(c)}


def readback_act(c, fids, host):
    """residual objects per (host frame_id, target frame_id) of the window, counted from nalo_ba_get_residuals (state >= 0: the residual exists)"""
    n = gm.live_counts(host, c.ba_get_residuals()[0], len(fids))
    return {(fids[h], fids[t]): int(n[h, t]) for h in range(len(fids)) for t in range(len(fids))}


def sync_live(g, live):
    for (h, t), n in live.items():
        g.set_live(h, t, n)


def assert_graph(c, g, what):
    got, want = entries(c), g.entries()
    assert len(got) == len(want), (what, len(got), len(want))
    assert got == want, (what, [(a, b) for a, b in zip(got, want) if a != b][:8])
    assert [e[:2] for e in got] == sorted(e[:2] for e in got), (what, "key order")
    assert connections(c) == g.connections(), what


def upload(win, n_slots=None):
    c = binding.Context(win.w, win.h, win.K, n_slots=n_slots or win.images.shape[0])
    for i in range(win.images.shape[0]):
        c.frame_upload(i, win.images[i])
    return c


def take(win, idx):
    return dataclasses.replace(win, host=win.host[idx], u=win.u[idx], v=win.v[idx], idepth=win.idepth[idx], idepth_true=win.idepth_true[idx], color=win.color[idx],
                               weights=win.weights[idx], exists=win.exists[idx])


# ------------------------------------------------------------------------------------------------ 1: the kernel's borders
SIZES = [1, 65, 257, 513]


@functools.lru_cache(None)
def border_window(full_graph):
    win = synth.make_window(w=640, h=480, W=4, P=4 * 513, seed=sc.SEED, n_extra=1, step_z=0.8 * LOW, step_x=0.03 * LOW, full_graph=full_graph)
    return take(win, np.concatenate([np.nonzero(win.host == h)[0][:n] for h, n in enumerate(SIZES)]))


def test_live_counts_at_the_kernels_borders():
    win = border_window(True)
    assert np.bincount(win.host).tolist() == SIZES
    exists = win.exists.copy()
    exists[win.host == 0] = [0, 0, 1, 0]                        # the pairs (0, 1), (0, 3): no residual; (0, 2): exactly one
    exists[win.host == 1] = 0                                   # a host without any residual
    exists[win.host == 2, 3] = 0                                # one more pair without
    fids = [40, 10, 30, 20]                                     # window order is not key order
    c = upload(win)
    c.ba_set_window(list(range(4)), win.world_to_cam[:4], frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(exists)
    assert c.ba_launch_config()["nblocks"] == 1 + 1 + 2 + 3
    c.map_graph_enable()                                        # on a standing window: its pairs are created here
    e = entries(c)
    want = readback_act(c, fids, win.host)
    assert len(e) == 16 and [x[:2] for x in e] == sorted(want)
    assert {x[:2]: x[2] for x in e} == want and all(x[3] == 0 for x in e)
    assert all(want[(f, f)] == 0 for f in fids)
    assert want[(40, 10)] == 0 and want[(40, 20)] == 0 and want[(40, 30)] == 1 and want[(30, 20)] == 0 and all(want[(10, f)] == 0 for f in fids)
    assert want[(20, 40)] == 513 and want[(30, 40)] == 257 and want[(20, 30)] == 513
    con = connections(c)
    assert [x[:2] for x in con] == [(10, 20), (10, 30), (10, 40), (20, 30), (20, 40), (30, 40)]
    assert con[3] == (20, 30, 513, 0, 0, 0) and con[5] == (30, 40, 257, 1, 0, 0) and con[0] == (10, 20, 0, 513, 0, 0)
    c.close()


@pytest.mark.parametrize("W,per_host", [(2, 150), (16, 40)])
def test_live_counts_smallest_and_largest_window(W, per_host):
    win = synth.make_window(w=320, h=240, W=W, P=W * per_host, seed=sc.SEED, n_extra=0, full_graph=False)
    fids = [3 * i + 1 for i in range(W)]
    c = upload(win)
    c.map_graph_enable()
    c.ba_set_window(list(range(W)), win.world_to_cam[:W], frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(win.exists)
    e = entries(c)
    want = readback_act(c, fids, win.host)
    assert len(e) == W * W and {x[:2]: x[2] for x in e} == want and all(x[3] == 0 for x in e)
    assert sum(want.values()) == int(win.exists.sum()) and min(want[(fids[h], fids[t])] for h in range(W) for t in range(W) if h != t) >= 1
    assert len(connections(c)) == W * (W - 1) // 2
    c.close()


# ------------------------------------------------------------------------------------------------ 2: every way a residual disappears or appears
def test_every_way_a_residual_disappears():
    win = border_window(False)
    P, W = len(win.host), 4
    rng = np.random.RandomState(sc.SEED + 1)
    idepth = win.idepth.copy()
    neg = rng.rand(P) < 0.02
    idepth[neg] = -idepth[neg]
    st6 = np.zeros((W + 1, 6))
    st6[1:, :3] = 0.004 * rng.randn(W, 3) / 0.5
    st6[1:, 3:] = 0.0004 * rng.randn(W, 3)
    fids = [100 + i for i in range(W)]
    c = upload(win)
    c.map_graph_enable()
    c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=st6[:W], frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, idepth, win.color, win.weights, has_prior=(win.host == 0).astype(np.int32))
    c.ba_set_residuals(win.exists)
    c.ba_set_point_history(*sc.plant_history(P, W))
    assert act_of(c) == readback_act(c, fids, win.host)
    # the fix pass's removals
    c.ba_linearize(False)
    st1 = c.ba_get_residuals()[0]
    assert act_of(c) == readback_act(c, fids, win.host)         # a pass that removes nothing changes nothing
    c.ba_linearize(True)
    st2 = c.ba_get_residuals()[0]
    removed = int(((st1 >= 0) & (st2 < 0)).sum())
    print("GRAPH fix pass removed %d of %d residuals" % (removed, int((st1 >= 0).sum())))
    assert removed >= 20
    assert act_of(c) == readback_act(c, fids, win.host)
    # the removal of the flagged points, all three classes; frame 1 (65 points) is flagged and loses every point
    ff = np.zeros(W, np.uint8); ff[1] = 1
    dec = c.ba_flag_points(ff)[0]
    print("GRAPH decisions", np.bincount(dec, minlength=4).tolist())
    assert all((dec == d).sum() >= 1 for d in (lm.DROP_NORES, lm.DROP, lm.MARGINALIZE)) and (dec[win.host == 1] != lm.KEEP).all()
    c.ba_marginalize_flagged()
    before = readback_act(c, fids, win.host)
    st3 = c.ba_get_residuals()[0]
    assert (st3[dec != lm.KEEP] < 0).all() and act_of(c) == before
    assert sum(marg_of(c).values()) == c.ba_counts()[2] > 0
    # a frame leaves from the middle: every pair with it reads 0, the others are unchanged
    c.ba_marginalize_frame(1)
    after = act_of(c)
    assert len(after) == 16 and sum(before[k] for k in before if 101 in k) > 0
    assert all(after[k] == (0 if 101 in k else before[k]) for k in before)
    assert [x[:2] for x in connections(c)] == [(100, 101), (100, 102), (100, 103), (101, 102), (101, 103), (102, 103)]
    # the carry with an entering frame: every carried point has one residual to it
    c.ba_carry_window(c.frame_state(W, win.world_to_cam[W], frame_id=104, state6=st6[W]))
    m = c.ba_carry_map()
    assert np.array_equal(m, np.nonzero(dec == lm.KEEP)[0])
    host = win.host[m] - (win.host[m] > 1)
    fids2 = [100, 102, 103, 104]
    live = readback_act(c, fids2, host)
    got = act_of(c)
    assert len(got) == 16 + 7 and all(got[k] == live.get(k, 0) for k in got)
    assert all(got[(fids2[h], 104)] == int((host == h).sum()) for h in range(3)) and got[(100, 104)] + got[(102, 104)] + got[(103, 104)] == len(m)
    assert all(got[k] == after[k] for k in after)               # the old pairs as they were, the departed frame's at 0
    c.close()


def test_the_graph_of_a_context_without_a_window_is_refused():
    c = binding.Context(320, 240, (160.0, 160.0, 159.5, 119.5), n_slots=2)
    c.map_graph_enable()
    for fn, dt in ((c.L.nalo_map_graph, binding.GRAPH_EDGE_DTYPE), (c.L.nalo_map_graph_connections, binding.GRAPH_CONNECTION_DTYPE)):
        out, n = np.full(4, -7, dt), C.c_int(-7)
        assert fn(c.h_, out.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == ERR_STATE
        assert n.value == -7 and (out == np.full(4, -7, dt)).all()
    c.close()


def test_the_window_from_the_initialiser_creates_its_pairs():
    """nalo_ba_window_from_initializer: the pairs of {firstFrame, newFrame}, one residual from every kept point to the new frame; a negative id is refused"""
    from test_init_window_gpu import EYE, Pair
    p = Pair(640, 480)
    a = p.a
    a.map_graph_enable()
    draws = p.draws()
    args = a.init_window_args(a.frame_state(0, EYE, frame_id=7), a.frame_state(3, EYE, frame_id=-9), draws)
    assert a.L.nalo_ba_window_from_initializer(a.h_, C.byref(args)) == ERR_ARG
    out, n = np.full(8, -7, binding.GRAPH_EDGE_DTYPE), C.c_int(-7)
    assert a.L.nalo_map_graph(a.h_, out.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == ERR_STATE and n.value == -7      # still no window
    a.ba_window_from_initializer(a.frame_state(0, EYE, frame_id=9), a.frame_state(3, EYE, frame_id=7), draws)
    assert a.P >= 500
    assert entries(a) == [(7, 7, 0, 0), (7, 9, 0, 0), (9, 7, a.P, 0), (9, 9, 0, 0)]
    assert act_of(a) == readback_act(a, [9, 7], np.zeros(a.P, np.int32))
    assert connections(a) == [(7, 9, 0, a.P, 0, 0)]
    p.close()


def test_after_the_insertion_of_activated_points():
    """the set-up of tests/test_ba_carry_gpu.py::test_insertion_of_the_activated_points on one context (its helpers by import)"""
    from imm_helpers import host_to_new
    from test_imm_activate_gpu import level1_maps
    from test_imm_large_gpu import CASES, Case, fresh_state
    cs = Case("K")
    W, s = cs.W, CASES["K"]
    wp = synth.make_window(w=s["w"], h=s["h"], W=W, P=W * 250, seed=9, n_extra=2, step_z=s["step_z"], yaw_deg=s["yaw"])
    st6 = synth.perturbed_poses(wp, sigma_t=0.002, sigma_r=0.0002)
    first = wp.host < W - 1
    a = cs.c
    a.map_graph_enable()
    fids = list(range(W))
    a.ba_set_window([int(x) for x in cs.slot[:W - 1]], wp.world_to_cam[:W - 1], aff=cs.aff[:W - 1], exposure=cs.exposure[:W - 1], state6=st6[:W - 1], frame_ids=fids[:W - 1])
    a.ba_set_points(wp.host[first], wp.u[first], wp.v[first], wp.idepth[first], wp.color[first], wp.weights[first])
    a.ba_set_residuals(wp.exists[first][:, :W - 1])
    a.ba_set_point_history()
    a.ba_carry_window(a.frame_state(int(cs.slot[W - 1]), wp.world_to_cam[W - 1], frame_id=W - 1, aff=cs.aff[W - 1], exposure=cs.exposure[W - 1], state6=st6[W - 1]))
    host0 = wp.host[first]
    before = readback_act(a, fids, host0)
    assert act_of(a) == before
    uu, vv, hh = cs.points(CASES["K"]["per_host"], seed=4, margin=3)
    color, weights, gradH, eth = cs.create(uu, vv, hh)
    p = np.random.RandomState(4 + 7).permutation(len(uu))
    u, v, host, color, weights, gradH, eth = [x[p] for x in (uu.astype(np.float32), vv.astype(np.float32), hh, color, weights, gradH, eth)]
    fs = fresh_state(len(u))
    a.imm_resident_set(u, v, color, weights, gradH, eth, host, fs["idmin"], fs["idmax"], fs["status"], fs["quality"])
    for new_frame in (W, W + 1):
        a.imm_resident_trace(int(cs.slot[new_frame]), *host_to_new(cs.win, new_frame, cs.aff, cs.exposure))
    idmin, idmax, status, quality = a.imm_resident_get()[:4]
    a.imm_resident_set(u, v, color, weights, gradH, eth, host, idmin, idmax, status, quality)
    a.imm_resident_set_type(np.random.RandomState(4 + 8).choice([1.0, 2.0, 4.0], len(u)).astype(np.float32))
    KRKi, Kt = level1_maps(cs.win, W - 1, yaw_deg=2.5)
    flagged = np.zeros(W, np.int32); flagged[1] = 1
    fate, sel, (result, idp, rin) = a.imm_resident_activate(W - 1, KRKi, Kt, flagged, 0.3, 3)
    assert (result == 1).sum() >= 100
    a.ba_carry_window(None, insert_activated=True)
    m = a.ba_carry_map()
    new_host = np.where(m >= 0, host0[np.maximum(m, 0)], host[sel[np.maximum(-m - 1, 0)]])
    live = readback_act(a, fids, new_host)
    got = act_of(a)
    assert got == live and sum(live.values()) > sum(before.values())
    want_in = {(fids[h], fids[t]): 0 for h in range(W) for t in range(W)}
    for k in np.nonzero(result == 1)[0]:
        for t in range(W):
            want_in[(fids[host[sel[k]]], fids[t])] += int(rin[k][t] != 0)
    assert all(got[k] == before[k] + want_in[k] for k in got)   # the residuals that ended the point's optimisation IN, and nothing else
    a.close()


# ------------------------------------------------------------------------------------------------ 3: marg against an independent route
@functools.lru_cache(None)
def marg_scene():
    """W = 5, 2500 points of the low-parallax corridor: a third of the graph missing, 2 % negative inverse depths, 1 % of the points without a residual"""
    W, P = 5, 2500
    win = synth.make_window(w=640, h=480, W=W, P=P, seed=sc.SEED, n_extra=0, step_z=0.8 * LOW, step_x=0.03 * LOW, full_graph=False)
    rng = np.random.RandomState(sc.SEED + 1)
    idepth = win.idepth.copy()
    neg = rng.rand(P) < 0.02
    idepth[neg] = -idepth[neg]
    exists = win.exists.copy()
    exists[rng.rand(P) < 0.01] = 0
    return dict(win=win, idepth=idepth, exists=exists, st6=synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004), fids=[100 + i for i in range(W)],
                hist=sc.plant_history(P, W), ff=sc.flag_sets(W)[2])


def marg_ctx(S, graph):
    win = S["win"]
    c = upload(win)
    if graph:
        c.map_graph_enable()
    c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=S["st6"], frame_ids=S["fids"])
    c.ba_set_points(win.host, win.u, win.v, S["idepth"], win.color, win.weights, has_prior=(win.host == 0).astype(np.int32))
    c.ba_set_residuals(S["exists"])
    c.ba_set_point_history(*S["hist"])
    return c


def same_state(a, t, th=True):
    """the twin's premise: no step was taken, poses and inverse depths are equal bit for bit - and, before the twin's extra pass, the frames' energy thresholds
    (that pass leaves the newest frame a threshold of its own, which nothing reads before the comparison is over)"""
    fa, ft = a.ba_get_frames(), t.ba_get_frames()
    if th:
        assert bytes(fa[0]) == bytes(ft[0])
    for x, y in zip(fa[0], ft[0]):
        assert x.frame_id == y.frame_id and bytes(x.worldToCam_evalPT) == bytes(y.worldToCam_evalPT) and bytes(x.state) == bytes(y.state) and bytes(x.state_zero) == bytes(y.state_zero)
    assert np.array_equal(fa[1].view(np.uint64), ft[1].view(np.uint64)) and np.array_equal(fa[2].view(np.uint64), ft[2].view(np.uint64))
    assert np.array_equal(a.ba_get_points()["idepth"].view(np.uint32), t.ba_get_points()["idepth"].view(np.uint32))


def expected_marg(fids, host, dec, st, active):
    """marg(h, t) = #{p : dec[p] == MARGINALIZE, the residual exists, it is active after the re-linearisation}"""
    hit = (dec == lm.MARGINALIZE)[:, None] & (st >= 0) & (active != 0)
    W = len(fids)
    return {(fids[h], fids[t]): int(hit[host == h][:, t].sum()) for h in range(W) for t in range(W)}


@pytest.mark.parametrize("route", ["before the fix pass", "after the fix pass"])
def test_marg_equals_the_twins_active_residuals(route):
    S = marg_scene()
    win, fids, fix = S["win"], S["fids"], route == "after the fix pass"
    A, T = marg_ctx(S, True), marg_ctx(S, False)
    for c in (A, T):
        c.ba_linearize(False)
        if fix:
            c.ba_linearize(True)
    dec = A.ba_flag_points(S["ff"])[0]
    st = A.ba_get_residuals()[0]
    if fix:
        assert np.isin(T.ba_get_residuals()[0], (-1, lm.IN)).all()          # every residual the fix pass left is IN
    same_state(A, T)
    T.ba_linearize(False)                                       # every residual once more, at the same state and the same resident frameEnergyTH
    active = T.ba_get_residuals()[1]
    same_state(A, T, th=False)
    n_marg = int((dec == lm.MARGINALIZE).sum())
    inactive = int(((dec == lm.MARGINALIZE)[:, None] & (st >= 0) & (active == 0)).sum())
    hosts = np.unique(win.host[dec == lm.MARGINALIZE])
    print("GRAPH marg %s: %d marginalised points of hosts %s, %d existing residuals of them inactive" % (route, n_marg, hosts.tolist(), inactive))
    assert n_marg >= 100 and len(hosts) >= 3
    if not fix:
        assert inactive >= 20                                   # marg is not a plain count of existing residuals
    m0 = A.ba_counts()[2]
    A.ba_marginalize_flagged()
    want = expected_marg(fids, win.host, dec, st, active)
    got = marg_of(A)
    assert got == want, [(k, got[k], want[k]) for k in want if got[k] != want[k]][:8]
    assert sum(got.values()) == A.ba_counts()[2] - m0 > 0
    assert all(got[(f, f)] == 0 for f in fids)
    if fix:
        # a second marginalisation on a later keyframe ADDS; nalo_ba_marginalize_points with host flags gives the first one's increments
        B = marg_ctx(S, True)
        B.ba_linearize(False)
        B.ba_linearize(True)
        decB = B.ba_flag_points(S["ff"])[0]
        assert np.array_equal(decB, dec)
        B.ba_marginalize_points((decB == lm.MARGINALIZE).astype(np.uint8))
        assert marg_of(B) == got and B.ba_counts()[2] == A.ba_counts()[2]
        B.close()
        A.ba_linearize(False)
        A.ba_linearize(True)
        ff2 = np.zeros(win.W, np.uint8); ff2[2] = 1
        dec2 = A.ba_flag_points(ff2)[0]
        m1 = A.ba_counts()[2]
        A.ba_marginalize_flagged()
        got2 = marg_of(A)
        print("GRAPH marg second keyframe: %d marginalised points, marg %d -> %d" % (int((dec2 == lm.MARGINALIZE).sum()), sum(got.values()), sum(got2.values())))
        assert all(got2[k] >= got[k] for k in got) and sum(got2.values()) - sum(got.values()) == A.ba_counts()[2] - m1 > 0
    A.close(); T.close()


# ------------------------------------------------------------------------------------------------ 4 - 6: the device chain
WW, KF = 5, 3


@functools.lru_cache(None)
def chain_data():
    win = synth.make_window(w=640, h=480, W=WW, P=1500, seed=sc.SEED, n_extra=KF, step_z=0.8 * LOW, step_x=0.03 * LOW, full_graph=False)
    F = WW + KF
    rng = np.random.RandomState(sc.SEED + 3)
    st6 = np.zeros((F, 6))
    st6[1:, :3] = 0.004 * rng.randn(F - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * rng.randn(F - 1, 3)
    ng0, lt0, ls0 = lm.default_history(win.exists)
    ls0[win.host == WW - 1, 0] = lm.IN
    return dict(win=win, st6=st6, hist=(ng0, lt0, ls0))


class Chain:
    """the loop of tests/test_map_gpu.py::test_three_keyframes_of_the_device_chain, step by step: frame 0 is flagged and leaves every keyframe"""

    def __init__(self, graph, archive=False):
        d = chain_data()
        self.win, self.st6 = d["win"], d["st6"]
        self.c = c = upload(self.win)
        c.ba_set_prior_carry(True)
        if graph:
            c.map_graph_enable()
        self.fids = [200 + i for i in range(WW)]
        c.ba_set_window(list(range(WW)), self.win.world_to_cam[:WW], state6=self.st6[:WW], frame_ids=self.fids)
        c.ba_set_points(self.win.host, self.win.u, self.win.v, self.win.idepth, self.win.color, self.win.weights)
        c.ba_set_residuals(self.win.exists)
        c.ba_set_point_history(*d["hist"])
        if archive:
            c.map_enable(chunk_points=300)
        self.host, self.entered = self.win.host.copy(), 0

    def entering(self):
        i = WW + self.entered
        return self.c.frame_state(i, self.win.world_to_cam[i], frame_id=200 + i, state6=self.st6[i])

    def fix(self):
        self.c.ba_linearize(False)
        self.c.ba_linearize(True)

    def flag(self):
        ff = np.zeros(WW, np.uint8); ff[0] = 1
        return self.c.ba_flag_points(ff)[0]

    def leave(self):
        self.c.ba_marginalize_frame(0)
        self.fids = self.fids[1:]

    def enter(self):
        e = self.entering()
        self.c.ba_carry_window(e)
        self.host = self.host[self.c.ba_carry_map()] - 1
        self.fids = self.fids + [200 + WW + self.entered]
        self.entered += 1

    def replay(self, n):
        for _ in range(n):
            self.fix(); self.flag()
            self.c.ba_marginalize_flagged()
            self.leave(); self.enter()

    def live(self):
        return readback_act(self.c, self.fids, self.host)


def twin_active(a, kf):
    """`active` of every residual after one more evaluation at the state A's marginalisation pass re-linearises at: a replay of the chain up to this keyframe"""
    t = Chain(False)
    t.replay(kf)
    t.fix()
    assert np.isin(t.c.ba_get_residuals()[0], (-1, lm.IN)).all()
    same_state(a.c, t.c)
    t.c.ba_linearize(False)
    active = t.c.ba_get_residuals()[1]
    t.c.close()
    return active


@pytest.fixture(scope="module")
def chain():
    """the chain's graph at every publish point, after every departure and after every carry: what cases 4 and 5 compare against -> dict(graphs, decs, model)"""
    a = Chain(True, archive=True)
    g = gm.Graph()
    for f in a.fids:
        g.insert_frame(f)
    sync_live(g, a.live())
    assert_graph(a.c, g, "the first window")
    graphs, decs = {("issue", 0): (entries(a.c), connections(a.c))}, []
    total_marg = 0
    for kf in range(KF):
        a.fix()
        dec = a.flag()
        st = a.c.ba_get_residuals()[0]
        active = twin_active(a, kf)
        a.c.ba_marginalize_flagged()
        for (h, t), n in expected_marg(a.fids, a.host, dec, st, active).items():
            g.marginalize(h, t, n)
            total_marg += n
        sync_live(g, a.live())                                  # the fix pass's removals, removePoint of the three classes
        assert_graph(a.c, g, "publish point of keyframe %d" % kf)
        graphs[("publish", kf)] = (entries(a.c), connections(a.c))
        print("GRAPH chain keyframe %d: decisions %s, entries %d, act %d, marg %d" % (kf, np.bincount(dec, minlength=4).tolist(), len(g.m), sum(v[0] for v in g.m.values()), total_marg))
        gone = a.fids[0]
        for f in a.fids:                                        # FullSystem::marginalizeFrame: every residual that targets the leaving frame
            g.set_live(f, gone, 0)
            assert g.m[gm.key(gone, f)][0] == 0                 # its own points went with the flagged host
        g.frame_leaves(gone)
        a.leave()
        assert_graph(a.c, g, "frame %d left" % gone)
        graphs[("left", kf)] = (entries(a.c), connections(a.c))
        g.insert_frame(200 + WW + a.entered)
        a.enter()
        sync_live(g, a.live())                                  # one residual from every carried point to the new frame
        assert_graph(a.c, g, "frame %d entered" % a.fids[-1])
        graphs[("issue", kf + 1)] = (entries(a.c), connections(a.c))
        decs.append(dec)
    r = dict(a=a, g=g, graphs=graphs, decs=decs, total_marg=total_marg)
    yield r
    a.c.close()


def test_three_keyframes_of_the_device_chain(chain):
    a, g = chain["a"], chain["g"]
    e = entries(a.c)
    seen = sorted({x[0] for x in e})
    assert seen == [200 + i for i in range(WW + KF)]            # 5 + 3 frames
    assert len(e) == len(g.m) == WW * WW + KF * (2 * WW - 1)
    gone = [200, 201, 202]
    assert all(x[2] == 0 for x in e if x[0] in gone or x[1] in gone)
    assert sum(x[3] for x in e if x[0] in gone or x[1] in gone) > 0 and chain["total_marg"] == sum(x[3] for x in e) == a.c.ba_counts()[2]
    by = {x[:2]: x for x in e}
    con = connections(a.c)
    assert len(con) == (len(e) - (WW + KF)) // 2 and [x[:2] for x in con] == sorted(k for k in by if k[0] < k[1])
    for f, t, fa, ba, fm, bm in con:                            # the forward and backward pairing
        assert (fa, fm) == by[(f, t)][2:] and (ba, bm) == by[(t, f)][2:]
    assert any(x[4] != x[5] for x in con) and any(x[2] != x[3] for x in con)


def test_reset_empties_the_graph(chain):
    a = chain["a"]
    a.c.map_reset()
    e = entries(a.c)
    live = a.live()
    assert len(e) == WW * WW and {x[:2]: x[2] for x in e} == live and all(x[3] == 0 for x in e) and sum(live.values()) > 0
    assert len(connections(a.c)) == WW * (WW - 1) // 2


# ------------------------------------------------------------------------------------------------ 5: the read-back route
def test_the_read_back_route_gives_the_same_graph(chain):
    from test_ba_carry_gpu import Pts, read_points, reissue
    d = chain_data()
    win, st6 = d["win"], d["st6"]
    r = upload(win)
    r.ba_set_prior_carry(True)
    r.map_graph_enable()
    r.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=st6[:WW], frame_ids=[200 + i for i in range(WW)])
    r.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    r.ba_set_residuals(win.exists)
    r.ba_set_point_history(*d["hist"])
    pts = Pts(win.host, win.u, win.v, win.color, win.weights, np.zeros(len(win.host), np.int32))
    graphs = chain["graphs"]
    assert (entries(r), connections(r)) == graphs[("issue", 0)]
    for kf in range(KF):
        r.ba_linearize(False)
        r.ba_linearize(True)
        ff = np.zeros(WW, np.uint8); ff[0] = 1
        dec = r.ba_flag_points(ff)[0]
        assert np.array_equal(dec, chain["decs"][kf])
        pre = read_points(r)
        r.ba_marginalize_points((dec == lm.MARGINALIZE).astype(np.uint8))
        assert {x[:2]: x[3] for x in entries(r)} == {x[:2]: x[3] for x in graphs[("publish", kf)][0]}      # marg at once; act once the dropped points are gone too
        valid = dec == lm.KEEP
        pts, _ = reissue(r, pts, pre, valid, list(range(WW)), None, r.ba_get_prior(), r.ba_get_point_history())
        assert (entries(r), connections(r)) == graphs[("publish", kf)], "publish point of keyframe %d" % kf
        pre = read_points(r)
        r.ba_marginalize_frame(0)
        assert (entries(r), connections(r)) == graphs[("left", kf)], "keyframe %d, the frame left" % kf
        i = WW + kf
        entering = r.frame_state(i, win.world_to_cam[i], frame_id=200 + i, state6=st6[i])
        pts, _ = reissue(r, pts, pre, np.ones(len(pts.host), bool), list(range(1, WW)), entering, r.ba_get_prior(), r.ba_get_point_history())
        assert (entries(r), connections(r)) == graphs[("issue", kf + 1)], "keyframe %d issued" % (kf + 1)
    r.close()


# ------------------------------------------------------------------------------------------------ 6: opt-in, no side effects, refusals
def readbacks(c):
    out = list(c.ba_get_points().values()) + list(c.ba_get_residuals()) + list(c.ba_get_prior()) + list(c.ba_get_point_history())
    return [np.ascontiguousarray(x).view(np.uint8) for x in out]


def test_opt_in_without_side_effects_and_refusals():
    g, n = Chain(True), Chain(False)
    for x in (g, n):
        x.fix(); x.flag()
        if x is g:
            entries(g.c)
        x.c.ba_marginalize_flagged()
    e1, c1 = entries(g.c), connections(g.c)
    rg, rn = readbacks(g.c), readbacks(n.c)
    assert len(rg) == len(rn) and all(np.array_equal(x, y) for x, y in zip(rg, rn))
    assert g.c.ba_counts() == n.c.ba_counts()
    assert entries(g.c) == e1 and connections(g.c) == c1        # twice in a row: equal, and nothing read back has changed
    assert all(np.array_equal(x, y) for x, y in zip(readbacks(g.c), rg))
    # graph off: NALO_ERR_STATE, outputs untouched
    for fn, dt in ((n.c.L.nalo_map_graph, binding.GRAPH_EDGE_DTYPE), (n.c.L.nalo_map_graph_connections, binding.GRAPH_CONNECTION_DTYPE)):
        out, k = np.full(64, -7, dt), C.c_int(-7)
        assert fn(n.c.h_, out.ctypes.data_as(C.c_void_p), 64, C.byref(k)) == ERR_STATE
        assert k.value == -7 and (out == np.full(64, -7, dt)).all()
    # cap too small: NALO_ERR_ARG with *n set, outputs untouched
    for fn, dt, want in ((g.c.L.nalo_map_graph, binding.GRAPH_EDGE_DTYPE, len(e1)), (g.c.L.nalo_map_graph_connections, binding.GRAPH_CONNECTION_DTYPE, len(c1))):
        out, k = np.full(64, -7, dt), C.c_int(-7)
        assert fn(g.c.h_, out.ctypes.data_as(C.c_void_p), want - 1, C.byref(k)) == ERR_ARG
        assert k.value == want and (out == np.full(64, -7, dt)).all()
    assert len(e1) == WW * WW and len(c1) == WW * (WW - 1) // 2
    # a negative frame_id while on: NALO_ERR_ARG by the call that would enter it, the window as it was
    frames = g.c.ba_get_frames()
    was = bytes(frames[0])
    bad = g.entering()
    bad.frame_id = -3
    assert g.c.L.nalo_ba_carry_window(g.c.h_, C.byref(bad), 0) == ERR_ARG
    arr = (binding.FrameState * WW).from_buffer_copy(was)
    arr[2].frame_id = -1
    cal = np.asarray(g.c.K, np.float64)
    assert g.c.L.nalo_ba_set_window(g.c.h_, WW, arr, binding._d(cal), binding._d(cal)) == ERR_ARG
    assert bytes(g.c.ba_get_frames()[0]) == was and entries(g.c) == e1
    assert all(np.array_equal(x, y) for x, y in zip(readbacks(g.c), rg))
    assert n.c.L.nalo_ba_carry_window(n.c.h_, C.byref(bad), 0) == 0      # ... and accepted while off
    # a sharded window: NALO_ERR_STATE
    n2 = Chain(False)
    n2.c.ba_set_allreduce(lambda ptr, k: None)
    assert n2.c.L.nalo_map_graph_enable(n2.c.h_, 1) == ERR_STATE
    assert n2.c.L.nalo_map_graph_enable(n2.c.h_, 0) == 0
    for x in (g, n, n2):
        x.c.close()
