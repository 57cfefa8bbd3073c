"""The point lifecycle on the device - the resident history (nalo_ba_set_point_history), flagPointsForRemoval as a kernel (nalo_ba_flag_points) and the
marginalisation / removal from its resident decisions (nalo_ba_marginalize_flagged) - against the literal model of tests/lifecycle_model.py.

Every comparison is over ALL points and is an equality: decisions, per-host counts and the history as integers, idepth_hessian bit for bit. The model works on the
library's public read-backs (nalo_ba_get_residuals, nalo_ba_get_points, the prior flag); the state of a residual a fix pass removed is derived from a
linearizeAll(false) made just before it (lifecycle_model.removed_states). The scenes and their coverage (every class, every clause of isOOB, H on both sides of 50)
are those of tests/lifecycle_scenes.py, which tests/test_point_lifecycle_cpu.py checks with the fp32 oracle alone.

  1  decisions at four window shapes (KITTI-shaped W = 8, W = 12, W = 16 with targets >= 8, 250 k points) with planted histories and 0, 1, 2 flagged frames
  2  the hand-built cases of the CPU test planted into a real window (H = 50 itself cannot be planted through the ABI: those two cases are realised by the side of H)
  3  two fix passes move the history exactly twice
  4  nalo_ba_optimize on its routes (gated pre-launch, plain, setting_forceAceptStep = false, a window with an all-reduce hook)
  5  nalo_ba_marginalize_flagged against nalo_ba_marginalize_points(decision == 3) on the restored snapshot, bit for bit, and the frame marginalisation behind it
  6  five keyframes of a sliding window that carry the history through get / set
  7  error cases; a context without a history reports the launch configuration it always did"""
import numpy as np
import pytest

import lifecycle_model as lm
import lifecycle_scenes as sc
from nalo_slam_amd import binding, synth
from test_point_lifecycle_cpu import CASES

pytestmark = pytest.mark.gpu

NALO_ERR_STATE = -4


def make_ctx(win, st6, has_prior=None):
    c = binding.Context(win.w, win.h, win.K, n_slots=win.W + 1)
    for i in range(win.W):
        c.frame_upload(i, win.images[i])
    c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=st6)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights, has_prior=has_prior)
    c.ba_set_residuals(win.exists)
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_history(got, want, what):
    for g, w, n in zip(got, want, ("numGood", "last_target", "last_state")):
        bad = np.nonzero(np.asarray(g, np.int64).reshape(len(g), -1) != np.asarray(w, np.int64).reshape(len(g), -1))[0]
        assert bad.size == 0, (what, n, bad[:10], np.asarray(g)[bad[:10]], np.asarray(w)[bad[:10]])


def device_route(c, win, planted):
    """plant, linearizeAll(false), linearizeAll(true), accumulate, flagPointsForRemoval for the three flag sets -> read-backs and device outputs"""
    c.ba_set_point_history(*planted)
    r = dict(before=c.ba_get_point_history())
    c.ba_linearize(False)
    r["st1"] = c.ba_get_residuals()[0]
    c.ba_linearize(True)
    r["st2"], r["ac2"] = c.ba_get_residuals()[:2]
    r["after"] = c.ba_get_point_history()
    r["pts"] = c.ba_get_points()                                   # runs the accumulation of the fix pass: the H the decisions read
    r["flags"] = [c.ba_flag_points(ff) for ff in sc.flag_sets(win.W)]
    return r


def assert_flags(dev, mod, what):
    dec, H, counts = dev
    print(what, "decisions", np.bincount(mod["dec"], minlength=4).tolist(), "mismatches", int((dec != mod["dec"]).sum()))
    bad = np.nonzero(dec != mod["dec"])[0]
    assert bad.size == 0, (what, bad[:10], dec[bad[:10]], mod["dec"][bad[:10]])
    assert np.array_equal(counts, mod["counts"]), (what, counts, mod["counts"])
    return H


@pytest.mark.parametrize("name", ["kitti", "w12", "w16", "stress250k"])
def test_decisions_equal_the_model(name):
    win, st6, has_prior = sc.make_scene(name)
    planted = sc.plant_history(len(win.host), win.W)
    c = make_ctx(win, st6, has_prior)
    r = device_route(c, win, planted)
    c.close()
    assert_history(r["before"], planted, "read-back of the planted history")
    m = sc.model_route(win, has_prior, planted, r["st1"], r["st2"], r["ac2"], r["pts"])
    assert_history(r["after"], (m["ng"], m["lt"], m["ls"]), "history after the fix pass")
    for dev, mod in zip(r["flags"], m["flags"]):
        H = assert_flags(dev, mod, "%s flagged %s" % (name, np.nonzero(mod["ff"])[0].tolist()))
        assert np.array_equal(bits(H), bits(m["H"])), ("idepth_hessian", np.nonzero(bits(H) != bits(m["H"]))[0][:10])
    sc.assert_coverage(name, m)
    if name == "w16":
        assert (r["after"][1] >= 8).sum() >= sc.SCENES[name]["min_points"]


def test_planted_cases_take_the_decision_of_the_table():
    win, st6, has_prior, hist, rows = sc.plant_cases(CASES)
    c = make_ctx(win, st6, has_prior)
    c.ba_set_point_history(*hist)
    c.ba_linearize(False)
    st = c.ba_get_residuals()[0]
    pts = c.ba_get_points()
    H = lm.idepth_hessian(pts["Hdd"], pts["HdiF"], has_prior)
    assert_history(c.ba_get_point_history(), hist, "a linearizeAll(false) leaves the history alone")
    n_real = [0] * len(CASES)
    for flagged in sorted({tuple(cs["flagged"]) for cs in CASES}):
        ff = np.array([i in flagged for i in range(win.W)], np.uint8)
        dec, Hd, counts = c.ba_flag_points(ff)
        mdec, mcounts, _, _ = lm.flag_points(win.host, st, pts["idepth"], H, ff, hist[0], hist[2])
        assert np.array_equal(dec, mdec) and np.array_equal(counts, mcounts) and np.array_equal(bits(Hd), bits(H))
        for ci, p in rows:
            cs = CASES[ci]
            if tuple(cs["flagged"]) == flagged and sc.realised(cs, st[p], H[p], pts["idepth"][p]):
                n_real[ci] += 1
                assert dec[p] == cs["dec"], (cs["name"], p, dec[p], st[p], H[p])
    c.close()
    print("replicas that realise their case:", [(cs["name"], n) for cs, n in zip(CASES, n_real)])
    assert min(n_real) >= 1, [(cs["name"], n) for cs, n in zip(CASES, n_real) if n == 0]


def test_two_fix_passes_move_the_history_twice():
    win, st6, has_prior = sc.make_scene("kitti")
    planted = sc.plant_history(len(win.host), win.W)
    c = make_ctx(win, st6, has_prior)
    c.ba_set_point_history(*planted)
    c.ba_linearize(False)
    st1 = c.ba_get_residuals()[0]
    c.ba_linearize(True)
    stA, acA = c.ba_get_residuals()[:2]
    hA = c.ba_get_point_history()
    c.ba_linearize(True)
    stB, acB = c.ba_get_residuals()[:2]
    hB = c.ba_get_point_history()
    c.close()
    mA = lm.history_update(*planted, st1, stA, acA, lm.removed_states(st1, st1, stA))
    assert_history(hA, mA, "first fix pass")
    mB = lm.history_update(*mA, stA, stB, acB, lm.removed_states(stA, stA, stB))           # every survivor of pass 1 is IN: what pass 2 removes is OUTLIER
    assert_history(hB, mB, "second fix pass")
    nA, nB = ((stA >= 0) & (acA != 0)).sum(1), ((stB >= 0) & (acB != 0)).sum(1)
    assert np.array_equal(hB[0].astype(np.int64), planted[0].astype(np.int64) + nA + nB) and nA.sum() > 0 and nB.sum() > 0
    gone = (planted[1] >= 0) & (hA[1] < 0)                                                   # pointers whose residual pass 1 removed
    assert gone.sum() >= 100
    assert (hB[1][gone] == -1).all() and np.array_equal(hB[2][gone], hA[2][gone])


def test_flag_points_runs_the_pending_accumulation_itself():
    """step API: nobody reads the points between the fix pass and the decision, so nalo_ba_flag_points has to accumulate that linearisation itself"""
    win, st6, has_prior = sc.make_scene("kitti")
    c = make_ctx(win, st6, has_prior)
    c.ba_set_point_history(*sc.plant_history(len(win.host), win.W))
    c.ba_linearize(False)
    c.ba_linearize(True)
    dec, H, counts = c.ba_flag_points(sc.flag_sets(win.W)[2])
    pts = c.ba_get_points()
    c.close()
    Hm = lm.idepth_hessian(pts["Hdd"], pts["HdiF"], has_prior)
    assert np.array_equal(bits(H), bits(Hm)) and (H > 0).sum() >= 1000 and (dec == lm.MARGINALIZE).sum() >= 100


@pytest.mark.parametrize("route", ["gated", "plain", "energy_test", "sharded"])
def test_optimize_updates_the_history_once(route):
    name = "w12" if route == "plain" else "kitti"
    win, st6, has_prior = sc.make_scene(name)
    planted = sc.plant_history(len(win.host), win.W)
    c = make_ctx(win, st6, has_prior)
    if route == "energy_test":
        c.set_settings(force_accept_step=False)
    if route == "sharded":
        c.ba_set_allreduce(lambda ptr, n: None)                      # a one-rank group: the sum over the ranks is the buffer itself (the hooked code path, thresholds
                                                                     # on the side stream included)
    assert c.ba_launch_config()["prelaunch_eligible"] == (1 if route == "gated" else 0)
    c.ba_set_point_history(*planted)
    c.ba_optimize(6)
    st2, ac2 = c.ba_get_residuals()[:2]
    ng, lt, ls = c.ba_get_point_history()
    c.close()
    st_pre = np.where(win.exists != 0, lm.IN, -1).astype(np.int8)                             # resetOOB: every residual takes part
    removed = (st_pre >= 0) & (st2 < 0)
    assert removed.sum() >= 100 and ((st2 >= 0) & (ac2 == 0)).sum() == 0
    m = lm.history_update(*planted, st_pre, st2, ac2, np.where(removed, lm.OUTLIER, -1).astype(np.int8))
    assert np.array_equal(ng.astype(np.int64), m[0]) and np.array_equal(lt, m[1])
    # the state a removed residual left is not observable from outside: it must be one of the two a removed residual can have; everything else equals the model
    P = len(win.host)
    unknown = np.zeros((P, 2), bool)
    for k in (0, 1):
        t = planted[1][:, k].astype(np.int64)
        ok = t >= 0
        unknown[ok, k] = removed[np.nonzero(ok)[0], t[ok]]
    unknown[:, 1] &= planted[1][:, 1] != planted[1][:, 0]                                     # [0] takes the state when both name one residual
    assert unknown.sum() >= 50
    assert np.isin(ls[unknown], (lm.OOB, lm.OUTLIER)).all()
    assert np.array_equal(ls[~unknown], m[2][~unknown])


def test_resident_marginalisation_is_marginalize_points_bit_for_bit():
    win, st6, has_prior = sc.make_scene("kitti")
    W = win.W
    planted = sc.plant_history(len(win.host), W)
    c = make_ctx(win, st6, has_prior)
    c.ba_set_point_history(*planted)
    c.ba_linearize(False)
    c.ba_linearize(True)
    st2 = c.ba_get_residuals()[0]
    c.ba_get_points()
    ff = sc.flag_sets(W)[2]
    c.ba_snapshot()
    hist0 = c.ba_get_point_history()
    dec, H, counts = c.ba_flag_points(ff)
    assert (dec == lm.MARGINALIZE).sum() >= 100 and (dec == lm.DROP).sum() >= 100 and (dec == lm.DROP_NORES).sum() >= 100 and (dec == lm.KEEP).sum() >= 100
    A = c.ba_marginalize_flagged()
    A_prior, A_counts, A_st = c.ba_get_prior(), c.ba_counts(), c.ba_get_residuals()[0]
    # afterwards: kept points only
    assert (A_st[dec != lm.KEEP] == -1).all() and np.array_equal(A_st[dec == lm.KEEP], st2[dec == lm.KEEP])
    with pytest.raises(binding.NaloError):
        c.ba_marginalize_flagged()                                                            # the decisions were consumed by the first call
    dec2, _, counts2 = c.ba_flag_points(np.zeros(W, np.uint8))                                # only valid points are counted: the kept ones, none on the flagged host
    assert np.array_equal(counts2.sum(1), counts[:, lm.KEEP]) and (dec2[dec != lm.KEEP] == lm.KEEP).all() and counts2[1].sum() == 0
    # the same marginalisation through the flag-byte entry point, on the restored window
    c.ba_restore()
    assert_history(c.ba_get_point_history(), hist0, "restore brings the history back")
    assert np.array_equal(c.ba_get_residuals()[0], st2)
    B = c.ba_marginalize_points((dec == lm.MARGINALIZE).astype(np.uint8))
    B_prior, B_counts, B_st = c.ba_get_prior(), c.ba_counts(), c.ba_get_residuals()[0]
    for a, b, n in zip(A + A_prior, B + B_prior, ("M", "Mb", "Msc", "Mbsc", "HM", "bM")):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (n, np.abs(a - b).max())
    assert np.abs(A[0]).max() > 0 and np.abs(A_prior[0]).max() > 0
    # resInM (not part of the snapshot) accumulates over both calls: the same residuals twice, and no more of them than the marginalised points had
    assert B_counts[2] == 2 * A_counts[2] and 0 < A_counts[2] <= (st2[dec == lm.MARGINALIZE] >= 0).sum()
    assert (B_st[dec == lm.MARGINALIZE] == -1).all() and np.array_equal(B_st[dec != lm.MARGINALIZE], st2[dec != lm.MARGINALIZE])
    # the flagged host can leave the window after the resident route, and the history's pointers follow the frames
    c.ba_restore()
    c.ba_flag_points(ff, outputs=False)
    c.ba_marginalize_flagged()
    h1 = c.ba_get_point_history()
    c.ba_marginalize_frame(1)
    h2 = c.ba_get_point_history()
    c.close()
    assert np.array_equal(h2[1], lm.remap_at_frame_marginalization(h1[1], 1)) and np.array_equal(h2[0], h1[0]) and np.array_equal(h2[2], h1[2])
    assert (h1[1] == 1).sum() >= 20 and (h1[1] > 1).sum() >= 100


def test_history_carries_across_five_keyframes():
    """A sliding window of 5 frames over 9 keyframes of the low-parallax corridor: every keyframe re-issues the window, carries the history through get / set
    with the caller's shift at insertion, runs the fix pass, decides with the oldest frame flagged, removes resident and marginalises that frame."""
    WW, KF = 5, 5
    s = sc.SCENES["kitti"]
    big = synth.make_window(w=s["w"], h=s["h"], W=WW + KF - 1, P=3600, seed=sc.SEED, n_extra=0, step_z=0.8 * s["scale"], step_x=0.03 * s["scale"], full_graph=False)
    F, P = big.W, len(big.host)
    st6_all = synth.perturbed_poses(big, sigma_t=0.004, sigma_r=0.0004)
    exists = big.exists.astype(bool)
    c = binding.Context(big.w, big.h, big.K, n_slots=F)
    for i in range(F):
        c.frame_upload(i, big.images[i])
    active = np.zeros(P, bool)
    ng_all, lt_all, ls_all = np.zeros(P, np.int32), np.full((P, 2), -1, np.int8), np.full((P, 2), lm.OOB, np.int8)
    seen = dict(dec=np.zeros(4, np.int64), carried=0)
    for k in range(KF):
        fids = list(range(k, k + WW))
        if k == 0:
            fresh = np.isin(big.host, fids[:-1])
        else:
            fresh = big.host == fids[-2]                                                      # the previous keyframe's candidates are activated now
            old = np.nonzero(active)[0]
            exists[old, fids[-1]] = True                                                      # FullSystem.cpp:1335-1348
            lt_all[old], ls_all[old] = lm.shift_at_insertion(lt_all[old], ls_all[old], np.ones(len(old), bool), WW - 1)
        ids_f = np.nonzero(fresh)[0]
        ex_f = exists[np.ix_(ids_f, fids)]
        ng_all[ids_f], lt_all[ids_f], ls_all[ids_f] = lm.default_history(ex_f)
        active |= fresh
        ids = np.nonzero(active)[0]
        host_w = np.array([fids.index(h) for h in big.host[ids]], np.int32)
        ex = exists[np.ix_(ids, fids)].astype(np.uint8)
        c.ba_set_window(fids, big.world_to_cam[fids], state6=st6_all[fids], frame_ids=fids)
        c.ba_set_points(host_w, big.u[ids], big.v[ids], big.idepth[ids], big.color[ids], big.weights[ids])
        c.ba_set_residuals(ex)
        if k == 0:
            c.ba_set_point_history()                                                          # the defaults of the header = optimizeImmaturePoint's
            assert_history(c.ba_get_point_history(), (ng_all[ids], lt_all[ids], ls_all[ids]), "default history")
        else:
            c.ba_set_point_history(ng_all[ids], lt_all[ids], ls_all[ids])
            seen["carried"] += int((ng_all[ids] > 0).sum())
        c.ba_linearize(False)
        st1 = c.ba_get_residuals()[0]
        c.ba_linearize(True)
        st2, ac2 = c.ba_get_residuals()[:2]
        pts = c.ba_get_points()
        m = lm.history_update(ng_all[ids], lt_all[ids], ls_all[ids], st1, st2, ac2, lm.removed_states(st1, st1, st2))
        assert_history(c.ba_get_point_history(), m, "keyframe %d" % k)
        ff = np.zeros(WW, np.uint8); ff[0] = 1
        dec, H, counts = c.ba_flag_points(ff)
        Hm = lm.idepth_hessian(pts["Hdd"], pts["HdiF"], np.zeros(len(ids)))
        mdec, mcounts, _, _ = lm.flag_points(host_w, st2, pts["idepth"], Hm, ff, m[0], m[2])
        assert np.array_equal(dec, mdec) and np.array_equal(counts, mcounts) and np.array_equal(bits(H), bits(Hm)), k
        seen["dec"] += np.bincount(dec, minlength=4)
        c.ba_marginalize_flagged()
        c.ba_marginalize_frame(0)
        ng, lt, ls = c.ba_get_point_history()
        assert np.array_equal(lt, lm.remap_at_frame_marginalization(m[1], 0))
        ng_all[ids], lt_all[ids], ls_all[ids] = ng, lt, ls
        exists[np.ix_(ids, fids)] = st2 >= 0
        exists[:, fids[0]] = False
        active[ids[dec != lm.KEEP]] = False
    c.close()
    print("decisions over the five keyframes", seen)
    assert (seen["dec"] >= 50).all() and seen["carried"] >= 1000


def test_error_cases_and_a_context_without_history():
    win, st6, has_prior = sc.make_scene("kitti")
    c = binding.Context(win.w, win.h, win.K, n_slots=win.W + 1)
    ff = np.zeros(win.W, np.uint8)
    assert c.L.nalo_ba_flag_points(c.h_, ff.ctypes.data_as(binding.c_u8p), None, None, None) == NALO_ERR_STATE        # before a window
    c.close()
    c = make_ctx(win, st6, has_prior)
    cfg = c.ba_launch_config()
    assert c.L.nalo_ba_flag_points(c.h_, ff.ctypes.data_as(binding.c_u8p), None, None, None) == NALO_ERR_STATE        # without a history
    assert c.L.nalo_ba_marginalize_flagged(c.h_, None, None, None, None) == NALO_ERR_STATE                            # without decisions
    assert c.L.nalo_ba_get_point_history(c.h_, None, None, None) == NALO_ERR_STATE
    c.profile_select("ba_hist_update")
    c.profile_enable(True)
    c.ba_optimize(6)
    st_plain = c.ba_get_residuals()[0]
    assert c.ba_launch_config() == cfg
    c.ba_linearize(True)
    assert len(c.profile_samples("ba_hist_update")) == 0                                      # no history: the per-point pass is never enqueued
    # the same window with a history: the launch configuration and the optimisation's result are those of the context without one
    h = make_ctx(win, st6, has_prior)
    h.ba_set_point_history()
    assert h.ba_launch_config() == cfg
    h.profile_select("ba_hist_update")
    h.profile_enable(True)
    h.ba_optimize(6)
    assert np.array_equal(h.ba_get_residuals()[0], st_plain)
    assert len(h.profile_samples("ba_hist_update")) == 1                                      # once per linearizeAll(true): the final pass of optimize()
    h.ba_linearize(False)
    assert len(h.profile_samples("ba_hist_update")) == 1
    h.ba_linearize(True)
    assert len(h.profile_samples("ba_hist_update")) == 2
    bad = np.full((len(win.host), 2), win.W, np.int8)
    with pytest.raises(binding.NaloError):
        h.ba_set_point_history(None, bad, np.zeros_like(bad))
    c.close(); h.close()
