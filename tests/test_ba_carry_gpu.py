"""nalo_ba_carry_window - the BA window re-issued from what is resident - against the re-issue it replaces.

Every comparison runs two contexts on the same inputs: A carries the window; B reads its own window back (nalo_ba_get_*), puts it through the literal model of
tests/carry_model.py and re-issues it with nalo_ba_set_window / set_points / set_residuals / set_point_history, with nalo_ba_set_prior from A's prior before the
carry (extended by the model for an entering frame). "Equal" is bit for bit: the launch configuration, the frames, the prior, idepth and idepth_zero, the residual
states, the history, and - after nalo_ba_linearize(0) on both - the energy, the 13x13 accumulators, H_A / b_A, the Schur complement and the x of the solve.
nalo_ba_optimize is not compared bitwise (a rare unexplained bit-level difference on its gated path); where a test needs an optimisation step it takes
it through the step API.

  1  a frame leaves from the middle and one enters (W = 6, ~3000 points)
  2  two frames leave and none enters, then one enters in a second carry
  2b hosts of 517, 517, 0, 256, 257 and 1 points (kBlk = 256: an empty host, a one-point block, an exactly full block, a block plus one): one enters, then one leaves
  3  insertion of an activation's points (the scene and immature points of test_imm_activate_gpu.py's smallest shape)
  4  four keyframes of a sliding window of five frames, A never re-issuing after keyframe 0
  5  W = 16, and the refusal of a 17th frame
  6  errors and hygiene"""
import ctypes as C

import numpy as np
import pytest

import carry_model as cm
import lifecycle_model as lm
import lifecycle_scenes as sc
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
BLK = 256


# ------------------------------------------------------------------------------------------------ the two routes
class Pts:
    """what a caller keeps about its points, in submission order (the library has no getter for them)"""

    def __init__(self, host, u, v, color, weights, has_prior):
        self.host, self.u, self.v, self.color, self.weights = [np.ascontiguousarray(a) for a in (host, u, v, color, weights)]
        self.has_prior = np.ascontiguousarray(has_prior, np.int32)

    def take(self, idx):
        return Pts(self.host[idx], self.u[idx], self.v[idx], self.color[idx], self.weights[idx], self.has_prior[idx])


def copy_fs(fs):
    out = binding.FrameState()
    C.memmove(C.byref(out), C.byref(fs), C.sizeof(binding.FrameState))
    return out


def set_window_raw(c, frames):
    """nalo_ba_set_window from nalo_frame_state records as they are (the calibration the context was created with)"""
    W = len(frames)
    arr = (binding.FrameState * W)(*frames)
    cal = np.asarray(c.K, np.float64)
    c._ck(c.L.nalo_ba_set_window(c.h_, W, arr, binding._d(cal), binding._d(cal)))
    c.W = W


def read_points(c):
    """what has to be read while the points are still set (before a nalo_ba_marginalize_frame)"""
    return dict(idepth=c.ba_get_points()["idepth"], idz=c.ba_get_idepth_zero(c.P), st=c.ba_get_residuals()[0])


def reissue(b, pts, pre, valid, rows, entering, prior, hist, ins=None):
    """B's route. pts / pre: the caller's arrays and the read-backs of the window that is being replaced; rows[t_new] = old index; prior = A's (HM, bM) before
    its carry; hist: B's history read after the frames left, or None; ins = (result, idepth_out, res_in, sel, resident arrays dict) for an insertion.
    -> (the new Pts, the model's window)"""
    frames = [copy_fs(f) for f in b.ba_get_frames()[0]]
    m = cm.carry(pts.host, valid, pre["st"], hist, rows, entering is not None)
    keep = m["old_p"]
    new = pts.take(keep)
    new.host = m["host"]
    idepth, idz = pre["idepth"][keep], pre["idz"][keep]
    HM, bM = prior
    if entering is not None:
        frames.append(copy_fs(entering))
        HM, bM = cm.extend_prior(HM, bM)
    if ins is not None:
        result, idp, rin, sel, res = ins
        m = cm.insert(m, result, rin, res["host"], sel)
        k = m["from_k"][m["from_k"] >= 0]
        i = sel[k]
        new = Pts(m["host"], np.concatenate([new.u, res["u"][i]]), np.concatenate([new.v, res["v"][i]]), np.concatenate([new.color, res["color"][i]]),
                  np.concatenate([new.weights, res["weights"][i]]), np.concatenate([new.has_prior, np.zeros(len(k), np.int32)]))
        idepth, idz = np.concatenate([idepth, idp[k]]), np.concatenate([idz, idp[k]])     # setIdepth / setIdepthZero(currentIdepth)
    set_window_raw(b, frames)
    b.ba_set_prior(HM, bM)
    b.ba_set_points(new.host, new.u, new.v, idepth, new.color, new.weights, has_prior=new.has_prior, idepth_zero=idz)
    b.ba_set_residuals(m["exists"])
    if m["hist"] is not None:
        b.ba_set_point_history(*m["hist"])
    return new, m


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_equal_windows(a, b, what, hist=True):
    assert a.W == b.W and a.P == b.P, (what, a.W, b.W, a.P, b.P)
    assert a.ba_launch_config() == b.ba_launch_config(), (what, a.ba_launch_config(), b.ba_launch_config())
    fa, fb = a.ba_get_frames(), b.ba_get_frames()
    assert bytes(fa[0]) == bytes(fb[0]), (what, "frames")
    assert np.array_equal(u64(fa[1]), u64(fb[1])) and np.array_equal(u64(fa[2]), u64(fb[2])), (what, "PRE_worldToCam / calib")
    for x, y, n in zip(a.ba_get_prior(), b.ba_get_prior(), ("HM", "bM")):
        assert x.shape == y.shape and np.array_equal(u64(x), u64(y)), (what, n)
    for x, y, n in ((a.ba_get_points()["idepth"], b.ba_get_points()["idepth"], "idepth"), (a.ba_get_idepth_zero(a.P), b.ba_get_idepth_zero(b.P), "idepth_zero")):
        bad = np.nonzero(u32(x) != u32(y))[0]
        assert bad.size == 0, (what, n, bad.size, bad[:8], x[bad[:8]], y[bad[:8]])
    sa, sb = a.ba_get_residuals()[:2], b.ba_get_residuals()[:2]
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), (what, "residual states", int((sa[0] != sb[0]).sum()))
    if hist:
        for x, y, n in zip(a.ba_get_point_history(), b.ba_get_point_history(), ("numGood", "last_target", "last_state")):
            assert np.array_equal(x, y), (what, n, int((x != y).sum()))
    assert_equal_linearisation(a, b, what)


def assert_equal_linearisation(a, b, what):
    ea, eb = a.ba_linearize(False), b.ba_linearize(False)
    assert np.array_equal(u64([ea]), u64([eb])) and ea > 0, (what, "energy", ea, eb)
    assert np.array_equal(u64(a.ba_get_acc13()), u64(b.ba_get_acc13())), (what, "acc13")
    for x, y, n in zip(a.ba_accumulate(0) + a.ba_accumulate_sc(True), b.ba_accumulate(0) + b.ba_accumulate_sc(True), ("H_A", "b_A", "H_sc", "b_sc")):
        assert np.array_equal(u64(x), u64(y)), (what, n, np.abs(x - y).max())
    xa, xb = a.ba_solve_system(0), b.ba_solve_system(0)
    assert np.array_equal(u64(xa), u64(xb)) and np.abs(xa).max() > 0, (what, "x", np.abs(xa - xb).max())


def blocks_per_host(host, W):
    return (np.bincount(host, minlength=W) + BLK - 1) // BLK


# ------------------------------------------------------------------------------------------------ the scene of tests 1 and 2
W6 = 6


def scene6():
    """1224x368, six keyframes + one that enters, ~3000 points of the low-parallax corridor (tests/lifecycle_scenes.py); 517 points per host = three blocks, of
    which the removals take one"""
    s = sc.SCENES["kitti"]
    win = synth.make_window(w=s["w"], h=s["h"], W=W6, P=3100, seed=sc.SEED, n_extra=1, step_z=0.8 * s["scale"], step_x=0.03 * s["scale"], full_graph=False)
    rng = np.random.RandomState(sc.SEED + 1)
    P = len(win.host)
    idepth = win.idepth.copy()
    neg = rng.rand(P) < 0.02
    idepth[neg] = -idepth[neg]
    exists = win.exists.copy()
    exists[rng.rand(P) < 0.01] = 0
    st6 = np.zeros((W6 + 1, 6))
    st6[1:, :3] = 0.004 * rng.randn(W6, 3) / 0.5
    st6[1:, 3:] = 0.0004 * rng.randn(W6, 3)
    return win, idepth, exists, st6, (win.host == 0).astype(np.int32)


def make_pair6(idx=None):
    """idx: the points of the scene the window is built from (all of them when None)"""
    win, idepth, exists, st6, has_prior = scene6()
    if idx is not None:
        idepth, exists, has_prior = idepth[idx], exists[idx], has_prior[idx]
        for n in ("host", "u", "v", "color", "weights"):
            setattr(win, n, np.ascontiguousarray(getattr(win, n)[idx]))
    pair = []
    for _ in range(2):
        c = binding.Context(win.w, win.h, win.K, n_slots=W6 + 1)
        for i in range(W6 + 1):
            c.frame_upload(i, win.images[i])
        c.ba_set_window(list(range(W6)), win.world_to_cam[:W6], state6=st6[:W6])
        c.ba_set_points(win.host, win.u, win.v, idepth, win.color, win.weights, has_prior=has_prior)
        c.ba_set_residuals(exists)
        c.ba_set_point_history()
        pair.append(c)
    pts = Pts(win.host, win.u, win.v, win.color, win.weights, has_prior)
    entering = pair[0].frame_state(W6, win.world_to_cam[W6], frame_id=W6, state6=st6[W6])
    return win, pair[0], pair[1], pts, entering


def fix_flag_remove(cs, flagged):
    """linearizeAll(false), the fix pass, flagPointsForRemoval, the removal: on every context alike -> the decisions (asserted equal)"""
    decs = []
    for c in cs:
        c.ba_linearize(False)
        c.ba_linearize(True)
        ff = np.zeros(c.W, np.uint8); ff[list(flagged)] = 1
        decs.append(c.ba_flag_points(ff))
    for d in decs[1:]:
        assert np.array_equal(d[0], decs[0][0]) and np.array_equal(d[2], decs[0][2]) and np.array_equal(u32(d[1]), u32(decs[0][1]))
    pre = [read_points(c) for c in cs]
    for c in cs:
        c.ba_marginalize_flagged()
    return decs[0][0], pre


def test_a_frame_leaves_from_the_middle_and_one_enters():
    win, a, b, pts, entering = make_pair6()
    dec, (pre_a, pre_b) = fix_flag_remove((a, b), [2])
    valid = dec == lm.KEEP
    assert (dec != lm.KEEP).sum() >= 500 and valid.sum() >= 1000 and not valid[pts.host == 2].any()
    hist_before = a.ba_get_point_history()
    for c in (a, b):
        c.ba_marginalize_frame(2)
    prior = a.ba_get_prior()
    stats = a.ba_carry_window(entering)
    rows = [0, 1, 3, 4, 5]
    new, m = reissue(b, pts, pre_b, valid, rows, entering, prior, b.ba_get_point_history())
    assert stats == (int(valid.sum()), 0, int(valid.sum()), a.ba_launch_config()["Ppad"])
    assert np.array_equal(a.ba_carry_map(), m["old_p"])
    assert_equal_windows(a, b, "a frame left, one entered")
    # the shapes the case is about
    before, after = blocks_per_host(pts.host, W6), blocks_per_host(new.host, W6)
    shrank = [h for t, h in enumerate(rows) if after[t] < before[h]]
    print("CARRY blocks per host before", before.tolist(), "after", after.tolist(), "carried", stats[0], "of", len(valid))
    assert shrank and a.ba_launch_config()["nblocks"] == int(after.sum())
    st = a.ba_get_residuals()[0]
    assert (st[:, W6 - 1] >= 0).all()                                         # every carried point has the residual to the new frame (read after a linearisation: in any state)
    old = pre_a["st"][valid]
    assert np.array_equal(st[:, 2:5] >= 0, old[:, 3:6] >= 0) and np.array_equal(st[:, :2] >= 0, old[:, :2] >= 0) and (old[:, 3:6] >= 0).sum() >= 500
    ng, lt, ls = a.ba_get_point_history()
    h1 = lm.remap_at_frame_marginalization(hist_before[1], 2)[valid]
    want_t, want_s = lm.shift_at_insertion(h1, hist_before[2][valid], np.ones(len(h1), bool), W6 - 1)
    assert np.array_equal(lt, want_t) and np.array_equal(ls, want_s) and np.array_equal(ng, hist_before[0][valid]) and (ng > 0).sum() >= 500
    a.close(); b.close()


def test_two_frames_leave_then_one_enters_in_a_second_carry():
    win, a, b, pts, entering = make_pair6()
    dec, (pre_a, pre_b) = fix_flag_remove((a, b), [1, 3])
    valid = dec == lm.KEEP
    for c in (a, b):
        c.ba_marginalize_frame(1)
        c.ba_marginalize_frame(2)                                             # the old frame 3
    prior = a.ba_get_prior()
    h_b = b.ba_get_point_history()
    assert a.ba_carry_window() == (int(valid.sum()), 0, int(valid.sum()), a.ba_launch_config()["Ppad"]) and a.W == 4
    new, m = reissue(b, pts, pre_b, valid, [0, 2, 4, 5], None, prior, h_b)
    assert np.array_equal(h_b[1][valid], m["hist"][1]) and (h_b[1][valid] >= 0).sum() >= 500      # remapped once per frame, not again by the carry
    assert_equal_windows(a, b, "two frames left")
    assert a.ba_get_prior()[0].shape == (36, 36)
    # ... and the next keyframe enters in a carry of its own, on the window the first one made
    prior = a.ba_get_prior()
    pre_b = read_points(b)
    a.ba_carry_window(entering)
    reissue(b, new, pre_b, np.ones(len(new.host), bool), [0, 1, 2, 3], entering, prior, b.ba_get_point_history())
    assert a.W == 5 and np.array_equal(a.ba_carry_map(), np.arange(a.P))
    assert_equal_windows(a, b, "then one entered")
    a.close(); b.close()


def test_block_edges_one_enters_then_a_frame_leaves():
    host = scene6()[0].host
    counts = [517, 517, 0, BLK, BLK + 1, 1]                                   # (the scene's last two hosts hold 516 points)
    idx = np.concatenate([np.nonzero(host == h)[0][:n] for h, n in enumerate(counts)])
    win, a, b, pts, entering = make_pair6(idx)
    assert np.bincount(pts.host, minlength=W6).tolist() == counts and a.ba_launch_config()["nblocks"] == 3 + 3 + 0 + 1 + 2 + 1
    # the new keyframe enters, nothing leaves: the block edges as they are
    prior, pre_b = a.ba_get_prior(), read_points(b)
    stats = a.ba_carry_window(entering)
    new, m = reissue(b, pts, pre_b, np.ones(len(pts.host), bool), list(range(W6)), entering, prior, b.ba_get_point_history())
    assert stats == (len(idx), 0, len(idx), 10 * BLK) and a.W == W6 + 1 and np.array_equal(a.ba_carry_map(), np.arange(len(idx)))
    assert_equal_windows(a, b, "block edges, one entered")
    # the host of the exactly full block is marginalised: its points go, the frame leaves, the hosts behind it move down a row
    dec, (pre_a, pre_b) = fix_flag_remove((a, b), [3])
    valid = dec == lm.KEEP
    assert not valid[new.host == 3].any() and valid[new.host == 4].sum() > 0
    for c in (a, b):
        c.ba_marginalize_frame(3)
    prior = a.ba_get_prior()
    assert a.ba_carry_window()[:3] == (int(valid.sum()), 0, int(valid.sum())) and a.W == W6
    reissue(b, new, pre_b, valid, [0, 1, 2, 4, 5, 6], None, prior, b.ba_get_point_history())
    assert_equal_windows(a, b, "block edges, a frame left")
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 3: insertion
def test_insertion_of_the_activated_points():
    from imm_helpers import host_to_new
    from test_imm_activate_gpu import level1_maps
    from test_imm_large_gpu import CASES, Case, fresh_state
    from test_trk_ref_window_gpu import assert_same_ref, expected_inputs, hilbert_device_rank, tracker_ref
    cs = Case("K")
    W, F, s = cs.W, cs.F, CASES["K"]
    # the window's own points: 250 per host (one block each, six slots short of a second), on the frames of the case
    wp = synth.make_window(w=s["w"], h=s["h"], W=W, P=W * 250, seed=9, n_extra=2, step_z=s["step_z"], yaw_deg=s["yaw"])
    assert np.array_equal(wp.world_to_cam, cs.win.world_to_cam)
    st6 = synth.perturbed_poses(wp, sigma_t=0.002, sigma_r=0.0002)
    first = wp.host < W - 1
    pts = Pts(wp.host[first], wp.u[first], wp.v[first], wp.color[first], wp.weights[first], np.zeros(first.sum(), np.int32))
    a = cs.c
    b = binding.Context(cs.w, cs.h, wp.K, n_slots=F)
    for i in range(F):
        b.frame_upload(int(cs.slot[i]), cs.win.images[i])
    for c in (a, b):
        c.ba_set_window([int(x) for x in cs.slot[:W - 1]], wp.world_to_cam[:W - 1], aff=cs.aff[:W - 1], exposure=cs.exposure[:W - 1], state6=st6[:W - 1])
        c.ba_set_points(pts.host, pts.u, pts.v, wp.idepth[first], pts.color, pts.weights)
        c.ba_set_residuals(wp.exists[first][:, :W - 1])
        c.ba_set_point_history()
    entering = a.frame_state(int(cs.slot[W - 1]), wp.world_to_cam[W - 1], frame_id=W - 1, aff=cs.aff[W - 1], exposure=cs.exposure[W - 1], state6=st6[W - 1])
    prior = a.ba_get_prior()
    a.ba_carry_window(entering)
    pts, m = reissue(b, pts, read_points(b), np.ones(len(pts.host), bool), list(range(W - 1)), entering, prior, b.ba_get_point_history())
    assert_equal_windows(a, b, "the keyframe entered")
    # activation on A: the resident set of the case, shuffled so that hosts interleave, traced over the two later frames; then every 37th point loses its
    # pattern weights (Hdd = 0 < setting_minIdepthH_act: optimizeImmaturePoint returns the null pointer for it, result 0) - the selection does not read them
    uu, vv, hh = cs.points(CASES["K"]["per_host"], seed=4, margin=3)
    color, weights, gradH, eth = cs.create(uu, vv, hh)
    p = np.random.RandomState(4 + 7).permutation(len(uu))
    u, v, host, color, weights, gradH, eth = [x[p] for x in (uu.astype(np.float32), vv.astype(np.float32), hh, color, weights, gradH, eth)]
    n = len(u)
    fs = fresh_state(n)
    a.imm_resident_set(u, v, color, weights, gradH, eth, host, fs["idmin"], fs["idmax"], fs["status"], fs["quality"])
    for new_frame in (W, W + 1):
        a.imm_resident_trace(int(cs.slot[new_frame]), *host_to_new(cs.win, new_frame, cs.aff, cs.exposure))
    idmin, idmax, status, quality = a.imm_resident_get()[:4]
    weights = weights.copy()
    weights[::37] = 0
    a.imm_resident_set(u, v, color, weights, gradH, eth, host, idmin, idmax, status, quality)
    a.imm_resident_set_type(np.random.RandomState(4 + 8).choice([1.0, 2.0, 4.0], n).astype(np.float32))
    state0 = a.imm_resident_get()
    res = dict(u=u, v=v, host=host, color=color, weights=weights)
    KRKi, Kt = level1_maps(cs.win, W - 1, yaw_deg=2.5)
    flagged = np.zeros(W, np.int32); flagged[1] = 1
    fate, sel, (result, idp, rin) = a.imm_resident_activate(W - 1, KRKi, Kt, flagged, 0.3, 3)
    print("CARRY activation: selected %d, result 1 / 0 / -1: %d / %d / %d" % (len(sel), (result == 1).sum(), (result == 0).sum(), (result == -1).sum()))
    assert (result == 1).sum() >= 100 and (result == 0).sum() >= 1 and (result == -1).sum() >= 1
    prior = a.ba_get_prior()
    pre_b = read_points(b)
    n_before = a.P
    stats = a.ba_carry_window(None, insert_activated=True)
    new, m = reissue(b, pts, pre_b, np.ones(n_before, bool), list(range(W)), None, prior, b.ba_get_point_history(), ins=(result, idp, rin, sel, res))
    assert stats[:3] == (n_before, int((result == 1).sum()), n_before + int((result == 1).sum()))
    assert np.array_equal(a.ba_carry_map(), m["old_p"]) and (m["old_p"] < 0).sum() == stats[1]
    for x, y in zip(a.imm_resident_get(), state0):
        assert np.array_equal(x, y, equal_nan=True)                           # the resident immature set is not modified
    # what the input reaches (on the model's point list): a host grows across a block boundary, and a new point is merged between carried ones
    before, after = blocks_per_host(pts.host, W), blocks_per_host(new.host, W)
    print("CARRY insertion: blocks per host before", before.tolist(), "after", after.tolist())
    assert ((before >= 1) & (after > before)).any() and a.ba_launch_config()["nblocks"] == int(after.sum())      # 250 + the inserted ones: across 256
    rank = hilbert_device_rank(new.host, new.u, new.v, cs.w, cs.h)
    inserted = m["old_p"] < 0
    between = 0
    for h in range(W):
        r_c, r_i = rank[(new.host == h) & ~inserted], rank[(new.host == h) & inserted]
        if len(r_c) and len(r_i):
            between += int(((r_i > r_c.min()) & (r_i < r_c.max())).sum())
    assert between >= 1, "no inserted point lies between two carried points of its host"
    assert_equal_windows(a, b, "the activated points inserted")
    # one Gauss-Newton step through the step API and the fix pass, then the tracking reference: A's from the window (the k -> d map rebuilt for the new
    # layout), B's from the arrays a caller would collect
    for c in (a, b):
        c.ba_linearize(False)
        c.ba_backup_state()
        c.ba_solve_system(0)
        c.ba_do_step(1.0)
        c.ba_linearize(True)
    a.trk_set_ref_from_window()
    idx, inp = expected_inputs(b, new.host)
    assert len(idx) >= 500 and (m["old_p"][idx] < 0).sum() >= 50              # inserted points take part in the reference
    b.trk_set_ref(int(cs.slot[W - 1]), *inp)
    assert_same_ref(tracker_ref(a), tracker_ref(b))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4: the sliding window
def test_four_keyframes_of_a_sliding_window():
    WW, KF = 5, 4
    s = sc.SCENES["kitti"]
    win = synth.make_window(w=s["w"], h=s["h"], W=WW, P=3600, seed=sc.SEED, n_extra=KF, step_z=0.8 * s["scale"], step_x=0.03 * s["scale"], full_graph=False)
    F = WW + KF
    rng = np.random.RandomState(sc.SEED + 3)
    st6 = np.zeros((F, 6))
    st6[1:, :3] = 0.004 * rng.randn(F - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * rng.randn(F - 1, 3)
    a, b = [binding.Context(win.w, win.h, win.K, n_slots=F) for _ in range(2)]
    for c in (a, b):
        for i in range(F):
            c.frame_upload(i, win.images[i])
        c.ba_set_prior_carry(True)
        c.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=st6[:WW], frame_ids=list(range(WW)))
        c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
        c.ba_set_residuals(win.exists)
        # the history of a running system: the defaults of a fresh point, but the newest keyframe's own points are not OOB on their first day (a point is not
        # activated on the newest frame; here it stands for the points the later keyframes would bring, which this test does not insert)
        ng0, lt0, ls0 = lm.default_history(win.exists)
        ls0[win.host == WW - 1, 0] = lm.IN
        c.ba_set_point_history(ng0, lt0, ls0)
    pts = Pts(win.host, win.u, win.v, win.color, win.weights, np.zeros(len(win.host), np.int32))
    carried_good, removed = 0, 0
    for k in range(KF + 1):
        if k > 0:
            entering = a.frame_state(WW - 1 + k, win.world_to_cam[WW - 1 + k], frame_id=WW - 1 + k, state6=st6[WW - 1 + k])
            a.ba_carry_window(entering)
            pts, m = reissue(b, pts, pre_b, valid, [1, 2, 3, 4], entering, prior, hist_b)
            assert np.array_equal(a.ba_carry_map(), m["old_p"])
            carried_good += int((a.ba_get_point_history()[0] > 0).sum())
            print("CARRY keyframe %d: %d points carried" % (k, a.P))
            assert_equal_windows(a, b, "keyframe %d" % k)
            if k == KF:
                break
        dec, (_, pre_b) = fix_flag_remove((a, b), [0])                        # asserts that A's decisions are B's
        valid = dec == lm.KEEP
        removed += int((~valid).sum())
        print("CARRY keyframe %d: decisions %s" % (k, np.bincount(dec, minlength=4).tolist()))
        for c in (a, b):
            c.ba_marginalize_frame(0)
        prior = a.ba_get_prior()
        hist_b = b.ba_get_point_history()
    a.close(); b.close()
    print("CARRY sliding window: carried histories with numGood > 0: %d, points removed: %d" % (carried_good, removed))
    assert carried_good >= 1000 and removed >= 1000


# ------------------------------------------------------------------------------------------------ 5: the largest window
def test_sixteen_frames():
    win, st6, has_prior = sc.make_scene("w16", every=4)
    W = win.W
    assert W == 16
    a, b = [binding.Context(win.w, win.h, win.K, n_slots=W + 1) for _ in range(2)]
    for c in (a, b):
        for i in range(W):
            c.frame_upload(i, win.images[i])
        c.frame_upload(W, win.images[0])                                      # the frame that leaves comes back as the newest keyframe: its own image and pose
        c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=st6)
        c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights, has_prior=has_prior)
        c.ba_set_residuals(win.exists)
        c.ba_set_point_history()
    pts = Pts(win.host, win.u, win.v, win.color, win.weights, has_prior)
    dec, (_, pre_b) = fix_flag_remove((a, b), [0])
    valid = dec == lm.KEEP
    for c in (a, b):
        c.ba_marginalize_frame(0)
    prior = a.ba_get_prior()
    entering = a.frame_state(W, win.world_to_cam[0], frame_id=W, state6=st6[0] + 1e-4)
    a.ba_carry_window(entering)
    reissue(b, pts, pre_b, valid, list(range(1, W)), entering, prior, b.ba_get_point_history())
    assert a.W == 16 and (a.ba_get_point_history()[1] >= 8).sum() >= 100       # targets beyond the 3-bit range survive the shift
    assert_equal_windows(a, b, "back to sixteen frames")
    # a 17th frame is refused, and the window is as usable as before
    assert a.L.nalo_ba_carry_window(a.h_, C.byref(entering), 0) == ERR_ARG
    assert b"NALO_MAX_WINDOW" in a.L.nalo_last_error(a.h_)
    assert a.W == 16 and a.ba_launch_config() == b.ba_launch_config()
    assert_equal_linearisation(a, b, "after the refusal")
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 6: errors and hygiene
def small_pair():
    """320x240, four keyframes + one later frame, 400 points; a resident immature set of 300 points around the true depth, typed"""
    from test_imm_activate_gpu import level1_maps
    win = synth.make_window(w=320, h=240, W=4, P=400, seed=5, n_extra=1)
    st6 = synth.perturbed_poses(win, sigma_t=0.002, sigma_r=0.0002)
    rng = np.random.RandomState(2)
    n = 300
    host = rng.randint(0, 4, n).astype(np.int32)
    u, v = rng.randint(8, win.w - 8, n), rng.randint(8, win.h - 8, n)
    ok = np.isfinite(win.depth[host, v, u])
    host, u, v = host[ok], u[ok].astype(np.int32), v[ok].astype(np.int32)
    idt = (1.0 / win.depth[host, v, u]).astype(np.float32)
    cs = []
    for _ in range(2):
        c = binding.Context(win.w, win.h, win.K, n_slots=win.W + 1)
        for i in range(win.W + 1):
            c.frame_upload(i, win.images[i])
        c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=st6)
        c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
        c.ba_set_residuals(win.exists)
        c.ba_set_point_history()
        cs.append(c)
    n = len(u)
    color, weights, gradH, eth = [np.zeros((n, k), np.float32) for k in (8, 8, 3)] + [np.zeros(n, np.float32)]
    for h in range(win.W):
        mk = host == h
        color[mk], weights[mk], gradH[mk], eth[mk] = cs[0].imm_create(h, u[mk], v[mk])
    imm = (u.astype(np.float32), v.astype(np.float32), color, weights, gradH, eth, host, (0.8 * idt).astype(np.float32), (1.2 * idt).astype(np.float32),
           np.zeros(n, np.int32), np.full(n, 10, np.float32))
    KRKi, Kt = level1_maps(win, win.W - 1)
    entering = cs[0].frame_state(win.W, win.world_to_cam[win.W], frame_id=win.W)
    return win, cs[0], cs[1], imm, (KRKi, Kt), entering


def refused(c, entering, insert, code=ERR_STATE):
    cfg, frames = c.ba_launch_config(), bytes(c.ba_get_frames()[0])
    rc = c.L.nalo_ba_carry_window(c.h_, None if entering is None else C.byref(entering), insert)
    msg = c.L.nalo_last_error(c.h_)
    assert rc == code and msg.startswith(b"nalo_ba_carry_window"), (rc, msg)
    assert c.ba_launch_config() == cfg and bytes(c.ba_get_frames()[0]) == frames
    return msg


def test_refusals_leave_the_window_intact():
    win, a, b, imm, (KRKi, Kt), entering = small_pair()
    W = win.W

    def activate():
        a.imm_resident_set(*imm)
        a.imm_resident_set_type(np.ones(len(imm[0]), np.float32))
        return a.imm_resident_activate(W - 1, KRKi, Kt, np.zeros(W, np.int32), 0.5, 2)

    assert b"pending" in refused(a, None, 1)                                  # nothing pending
    fate, sel, (result, idp, rin) = activate()
    assert len(sel) >= 1
    assert b"second call" in refused(a, entering, 1)                          # together with an entering frame
    a.imm_resident_set(*imm)                                                  # a new resident set drops the pending result
    a.imm_resident_set_type(np.ones(len(imm[0]), np.float32))
    assert b"pending" in refused(a, None, 1)
    a.imm_resident_activate(W - 1, KRKi, Kt, np.zeros(W, np.int32), 0.5)      # a later activation without outputs drops it too
    assert b"pending" in refused(a, None, 1)
    # after all the refusals A is the window B still is
    assert_equal_windows(a, b, "after the refusals")
    # the frames change between the activation and the insertion
    activate()
    prior = a.ba_get_prior()
    a.ba_carry_window(entering)
    assert b"changed" in refused(a, None, 1)
    pts = Pts(win.host, win.u, win.v, win.color, win.weights, np.zeros(len(win.host), np.int32))
    reissue(b, pts, read_points(b), np.ones(len(win.host), bool), list(range(W)), entering, prior, b.ba_get_point_history())
    assert_equal_windows(a, b, "after the refused insertion")
    # nalo_ba_restore after a carry: the snapshot is of arrays that are gone
    a.ba_snapshot()
    a.ba_carry_window()
    rc = a.L.nalo_ba_restore(a.h_)
    assert rc == ERR_STATE and b"snapshot" in a.L.nalo_last_error(a.h_)
    assert_equal_linearisation(a, b, "after the refused restore")
    # a sharded window is not carried
    a.ba_set_allreduce(lambda ptr, n: None)
    assert b"sharded" in refused(a, None, 0)
    # before there is anything to carry
    c = binding.Context(win.w, win.h, win.K, n_slots=2)
    assert c.L.nalo_ba_carry_window(c.h_, None, 0) == ERR_STATE and c.L.nalo_ba_carry_map(c.h_, None) == ERR_STATE
    st = np.zeros(4, np.int32)
    assert c.L.nalo_ba_carry_last(c.h_, binding._i(st)) == ERR_STATE
    c.close(); a.close(); b.close()
