"""The map side of the device chain - the archive of removed points (nalo_map_enable / nalo_map_get_frame / nalo_map_counts), the final cloud of a frame
(nalo_map_world_points) and the viewer's per-keyframe cloud (nalo_map_frame_cloud) - against the literal model of tests/map_model.py.

Every comparison is an equality over ALL records: integers as integers, floats bit for bit (NaN equal to NaN whatever its payload). The model works on the
library's public read-backs: nalo_ba_get_points before and after the marginalisation, nalo_ba_flag_points' decision and idepth_hessian, the submitted u, v,
colours and prior flags.

  1  the archive against a second context that takes the read-back route (640x480, W = 4, 400 points, the low-parallax scene of tests/lifecycle_scenes.py),
     and the archiving context's window against a context that never enabled the map
  2  planted sizes: hosts with 0, 1, 255, 256, 257 and 513 removed points, chunks of 300 records (every host run but the first two straddles a border), a keyframe
     that removes nothing, a second window on the same context that makes the archive grow (1282 archived + 3600 valid points > the 12 chunks of the first call)
  3  three keyframes of the device chain (flag -> marginalize_flagged -> marginalize_frame -> carry_window), frames leaving; nalo_map_reset
  4  nalo_map_world_points against the model and against the PCD writer's numbers (nalo_map_world_points_host)
  5  nalo_map_frame_cloud for a window frame with all four classes and for a frame that has left: display modes, every clause, draws, refusals
  6  1224x368, W = 8: one keyframe, all three calls

addPoint's zeroing of a marginalised point that ends its re-linearisation without an active residual is in the model (tests/test_map_cpu.py); none of these
scenes produces such a point (the tests print the count), so the device's two stores for it are not reached here."""
import ctypes as C

import numpy as np
import pytest

import lifecycle_model as lm
import lifecycle_scenes as sc
import map_model as mm
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
BIG = 1e30


def scene(w, h, W, P, seed=sc.SEED):
    """tests/lifecycle_scenes.make_scene at a size of its own: the low-parallax corridor, a third of the graph missing, 2 % negative inverse depths, 1 % of the
    points without a residual, the points of host 0 with the depth prior"""
    s = 3e-4
    win = synth.make_window(w=w, h=h, W=W, P=P, seed=seed, n_extra=0, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    rng = np.random.RandomState(seed + 1)
    idepth = win.idepth.copy()
    neg = rng.rand(P) < 0.02
    idepth[neg] = -idepth[neg]
    exists = win.exists.copy()
    exists[rng.rand(P) < 0.01] = 0
    return dict(win=win, idepth=idepth, exists=exists, st6=synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004), hp=(win.host == 0).astype(np.int32),
                host=win.host, u=win.u, v=win.v, color=win.color, fids=[100 + i for i in range(W)])


def make_ctx(S, n_slots=None):
    win = S["win"]
    c = binding.Context(win.w, win.h, win.K, n_slots=n_slots or win.images.shape[0])
    for i in range(win.images.shape[0]):
        c.frame_upload(i, win.images[i])
    issue(c, S)
    return c


def issue(c, S):
    win = S["win"]
    c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=S["st6"][:win.W], frame_ids=S["fids"])
    c.ba_set_points(S["host"], S["u"], S["v"], S["idepth"], S["color"], win.weights, has_prior=S["hp"])
    c.ba_set_residuals(S["exists"])


def calib_inv(c):
    return mm.calib_inverse(c.ba_get_frames()[2])


def keyframe(c, S, ff):
    """flag + resident removal on an archiving context, with the model's expectation from the context's own read-backs -> dict(dec, H, pre, post, exp)"""
    pre = c.ba_get_points()
    dec, H, cnt = c.ba_flag_points(ff)
    c.ba_marginalize_flagged()
    post = c.ba_get_points()                                       # the removed points' slots keep the sums of the marginalisation's accumulation
    exp = mm.flag_points_push(S["host"], S["fids"], S["u"], S["v"], pre["idepth"], S["color"], dec, H, pre["maxRelBaseline"], post["Hdd"], post["HdiF"], S["hp"])
    return dict(dec=dec, H=H, cnt=cnt, pre=pre, post=post, exp=exp)


def assert_frame(c, fid, marg, out, what):
    got = c.map_get_frame(fid)
    want = np.concatenate([marg, out])
    assert len(got) == len(want), (what, fid, len(got), len(want))
    for k in mm.RECORD.names:
        assert mm.bits_equal(got[k], want[k]), (what, fid, k, np.nonzero(~(got[k] == want[k]).reshape(len(got), -1).all(1))[0][:10])
    assert c.map_counts(fid) == (len(marg), len(out)), (what, fid)


# ------------------------------------------------------------------------------------------------ the shared small keyframe
@pytest.fixture(scope="module")
def small():
    """three contexts on the small scene after one keyframe with host 1 flagged: A archives, B takes the read-back route, N never enabled the map"""
    S = scene(640, 480, 4, 400)
    planted = sc.plant_history(400, 4)
    A, B, N = [make_ctx(S) for _ in range(3)]
    A.map_enable()
    for c in (A, B, N):
        c.ba_set_point_history(*planted)
        c.ba_linearize(False)
        c.ba_linearize(True)
    ff = sc.flag_sets(4)[1]
    preB = B.ba_get_points()
    decB, HB, _ = B.ba_flag_points(ff)
    N.ba_get_points()
    N.ba_flag_points(ff)
    N.ba_marginalize_flagged()
    k = keyframe(A, S, ff)
    B.ba_marginalize_points((decB == lm.MARGINALIZE).astype(np.uint8))
    postB = B.ba_get_points()
    expB = mm.flag_points_push(S["host"], S["fids"], S["u"], S["v"], preB["idepth"], S["color"], decB, HB, preB["maxRelBaseline"], postB["Hdd"], postB["HdiF"], S["hp"])
    r = dict(S=S, A=A, B=B, N=N, k=k, decB=decB, HB=HB, expB=expB, ci=calib_inv(A))
    yield r
    for c in (A, B, N):
        c.close()


def test_archive_equals_the_read_back_route(small):
    S, A, N, k = small["S"], small["A"], small["N"], small["k"]
    dec = k["dec"]
    print("MAP small: decisions", np.bincount(dec, minlength=4).tolist(), "marginalised without an active residual", int(((dec == 3) & (k["post"]["HdiF"] == 0)).sum()))
    assert (np.bincount(dec, minlength=4) >= 1).all()                                          # every decision class occurs
    assert np.array_equal(dec, small["decB"]) and mm.bits_equal(k["H"], small["HB"])
    for fid in S["fids"]:
        assert_frame(A, fid, *small["expB"][fid], "second context")
        assert_frame(A, fid, *k["exp"][fid], "own read-backs")
    assert A.map_counts(101)[0] + A.map_counts(101)[1] == (S["host"] == 1).sum()               # the flagged host lost every point
    assert sum(sum(A.map_counts(f)) for f in S["fids"]) == (dec != lm.KEEP).sum()
    assert np.array_equal(np.array([A.map_counts(f) for f in S["fids"]]), np.stack([k["cnt"][:, 3], k["cnt"][:, 1] + k["cnt"][:, 2]], 1))
    # the window is the one of a context that never enabled the map
    for a, n in zip(A.ba_get_prior(), N.ba_get_prior()):
        assert np.array_equal(a.view(np.uint64), n.view(np.uint64))
    assert A.ba_counts() == N.ba_counts()
    pa, pn = A.ba_get_points(), N.ba_get_points()
    assert all(mm.bits_equal(pa[q], pn[q]) for q in pa)
    for a, n in zip(A.ba_get_residuals(), N.ba_get_residuals()):
        assert mm.bits_equal(a, n)
    assert all(np.array_equal(a, n) for a, n in zip(A.ba_get_point_history(), N.ba_get_point_history()))
    with pytest.raises(binding.NaloError):
        A.map_counts(7)                                                                        # a frame_id the archive has never seen


def test_world_points(small):
    S, A, ci = small["S"], small["A"], small["ci"]
    rng = np.random.RandomState(5)
    m = np.concatenate([np.linalg.qr(rng.randn(3, 3))[0], [[2.5e6 + 0.37], [-8.1e5], [42.0]]], 1)          # a pose with a large translation
    lib = C.CDLL(binding.lib_path())
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    total = 0
    for fid in S["fids"]:
        marg = small["k"]["exp"][fid][0]
        got = A.map_world_points(fid, m)
        assert got.shape == (len(marg), 3)
        assert mm.bits_equal(got, mm.world_points(marg["u"], marg["v"], marg["idepth"], ci, m)), fid
        io = np.zeros((len(marg), 3))
        u, v, idp, mc = [np.ascontiguousarray(marg[q]) for q in ("u", "v", "idepth")] + [np.ascontiguousarray(m.ravel())]
        assert lib.nalo_map_world_points_host(len(marg), u.ctypes.data_as(fp), v.ctypes.data_as(fp), idp.ctypes.data_as(fp), ci.ctypes.data_as(fp), mc.ctypes.data_as(dp), io.ctypes.data_as(dp)) == 0
        assert mm.bits_equal(got, io), fid
        total += len(marg)
    print("MAP world points:", total)
    assert total >= 1
    fid = max(S["fids"], key=lambda f: A.map_counts(f)[0])
    n = C.c_int(-1)
    cnt = A.map_counts(fid)[0]
    buf = np.zeros((cnt, 3))
    mc = np.ascontiguousarray(m.ravel())
    assert A.L.nalo_map_world_points(A.h_, fid, mc.ctypes.data_as(dp), buf.ctypes.data_as(dp), cnt - 1, C.byref(n)) == ERR_ARG and n.value == cnt and not buf.any()   # cap too small
    assert A.L.nalo_map_world_points(A.h_, 7, mc.ctypes.data_as(dp), buf.ctypes.data_as(dp), 1, C.byref(n)) == ERR_ARG


def cloud_model(rec, ci, mode, scaledTH, absTH, minBS, draws):
    xyz, rgb, nrec, nsur = mm.refresh_pc(rec, scaledTH, absTH, mode, minBS, ci, draws)
    return dict(xyz=xyz, rgb=rgb, records=nrec, survivors=nsur)


def assert_cloud(got, want, what):
    assert np.array_equal(got["records"], want["records"]) and np.array_equal(got["survivors"], want["survivors"]), (what, got["records"], want["records"], got["survivors"], want["survivors"])
    assert got["xyz"].shape == want["xyz"].shape and mm.bits_equal(got["xyz"], want["xyz"]), (what, got["xyz"].shape, want["xyz"].shape)
    assert np.array_equal(got["rgb"], want["rgb"]), what


def immature_set(n, W, w, h, seed=11):
    """a resident immature set over W hosts, hosts interleaved in storage; fresh points (idepth_max = NaN), negative and zero depths among them"""
    rng = np.random.RandomState(seed)
    d = dict(u=rng.randint(4, w - 4, n).astype(np.float32), v=rng.randint(4, h - 4, n).astype(np.float32), color=rng.uniform(-20, 300, (n, 8)).astype(np.float32),
             weights=np.ones((n, 8), np.float32), gradH=np.ones((n, 3), np.float32), energyTH=np.full(n, 100, np.float32), host_idx=rng.randint(0, W, n).astype(np.int32),
             idmin=rng.uniform(0, 0.5, n).astype(np.float32), idmax=rng.uniform(0.5, 2, n).astype(np.float32), status=np.zeros(n, np.int32), quality=np.full(n, 10000, np.float32))
    d["idmax"][rng.rand(n) < 0.1] = np.nan
    d["idmin"][rng.rand(n) < 0.05] = -3.0
    z = rng.rand(n) < 0.03
    d["idmin"][z], d["idmax"][z] = 0.0, 0.0
    d["color"][rng.rand(n, 8) < 0.02] = np.nan
    return d


def frame_records(S, k, fid, widx, imm):
    """setFromKF for a frame of the small scene after the keyframe k: the immature points of host widx, its kept points, its archive lists"""
    im = None
    if imm is not None:
        sel = imm["host_idx"] == widx
        im = dict(u=imm["u"][sel], v=imm["v"][sel], idepth_min=imm["idmin"][sel], idepth_max=imm["idmax"][sel], color=imm["color"][sel])
    act = None
    if widx >= 0:
        idx = np.nonzero((S["host"] == widx) & (k["dec"] == lm.KEEP))[0]
        act = np.zeros(len(idx), mm.RECORD)
        act["u"], act["v"], act["idepth"], act["color"] = S["u"][idx], S["v"][idx], k["post"]["idepth"][idx], S["color"][idx]
        act["idepth_hessian"] = lm.idepth_hessian(k["post"]["Hdd"], k["post"]["HdiF"], S["hp"])[idx]
        act["maxRelBaseline"] = k["pre"]["maxRelBaseline"][idx]                                  # the last linearizeAll(true)'s
    return mm.set_from_kf(im, act, *k["exp"][fid])


def clause_values(rec):
    with np.errstate(all="ignore"):
        depth = np.float32(1) / rec["idepth"]
        var = (1.0 / (rec["idepth_hessian"].astype(np.float64) + 0.01)).astype(np.float32)
        return var, var * (depth * depth) * (depth * depth)


def test_frame_cloud(small):
    S, A, k, ci = small["S"], small["A"], small["k"], small["ci"]
    win = S["win"]
    imm = immature_set(500, 4, win.w, win.h)
    A.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
    # the unflagged frame whose rarest class is largest
    widx = max((0, 2, 3), key=lambda h: np.bincount(frame_records(S, k, 100 + h, h, imm)["status"], minlength=4).min())
    fid = 100 + widx
    rec = frame_records(S, k, fid, widx, imm)
    print("MAP cloud frame", fid, "records per status", np.bincount(rec["status"], minlength=4).tolist())
    assert (np.bincount(rec["status"], minlength=4) >= 1).all()                                # all four classes
    ok = rec["idepth"] >= 0
    var, sc4 = clause_values(rec)
    th_sc, th_abs, th_bs = np.median(sc4[ok & np.isfinite(sc4)]), np.median(var[ok]), np.median(rec["maxRelBaseline"][rec["maxRelBaseline"] > 0])
    draws = np.random.RandomState(9).randint(0, 2 ** 31 - 1, 8 * len(rec)).astype(np.int32)
    n_all = int(cloud_model(rec, ci, 0, BIG, BIG, 0.0, None)["survivors"].sum())
    for mode, a, b, bs, dr, what in ((0, th_sc, BIG, 0.0, None, "scaled"), (0, BIG, th_abs, 0.0, draws, "abs"), (0, BIG, BIG, th_bs, None, "baseline"),
                                     (1, th_sc, th_abs, th_bs, draws, "mode 1"), (2, BIG, BIG, 0.0, draws, "mode 2"), (3, BIG, BIG, 0.0, None, "mode 3"), (0, BIG, BIG, 0.0, draws, "all")):
        want = cloud_model(rec, ci, mode, a, b, bs, dr)
        got = A.map_frame_cloud(fid, mode, a, b, bs, draws=dr)
        assert_cloud(got, want, what)
        assert got["n_needed"] == 8 * len(rec)
        if what in ("scaled", "abs", "baseline"):                                              # the clause rejects some records and keeps some
            assert 0 < want["survivors"].sum() < n_all, (what, want["survivors"], n_all)
        if mode == 3:
            assert len(got["xyz"]) == 0
    assert np.isnan(cloud_model(rec, ci, 0, th_sc, th_abs, 0.0, None)["xyz"]).any()            # a fresh immature point passes with NaN vertices
    noimm = frame_records(S, k, fid, widx, None)
    assert_cloud(A.map_frame_cloud(fid, 0, th_sc, th_abs, 0.0, with_immature=False, draws=draws), cloud_model(noimm, ci, 0, th_sc, th_abs, 0.0, draws), "without the immature class")
    # refusals: nothing is written, n_needed answers
    a = binding.MapCloudArgs()
    a.frame_id, a.display_mode, a.with_immature, a.sparsity, a.scaledTH, a.absTH = fid, 0, 1, 2, BIG, BIG
    assert A.L.nalo_map_frame_cloud(A.h_, C.byref(a)) == ERR_ARG                               # sparsity > 1
    a.sparsity = 1
    xyz, rgb = np.zeros((8 * len(rec), 3), np.float32), np.zeros((8 * len(rec), 3), np.uint8)
    a.xyz, a.rgb, a.cap = xyz.ctypes.data_as(binding.c_fp), rgb.ctypes.data_as(binding.c_u8p), 8 * len(rec) - 1
    assert A.L.nalo_map_frame_cloud(A.h_, C.byref(a)) == ERR_ARG and a.n_needed == 8 * len(rec) and a.n == 0      # cap
    a.cap, a.draws, a.n_draws = 8 * len(rec), draws.ctypes.data_as(binding.c_ip), 8 * len(rec) - 1
    assert A.L.nalo_map_frame_cloud(A.h_, C.byref(a)) == ERR_ARG and a.n_needed == 8 * len(rec)                   # draws
    a.frame_id = 7
    assert A.L.nalo_map_frame_cloud(A.h_, C.byref(a)) == ERR_ARG                               # neither in the window nor in the archive
    assert not xyz.any() and not rgb.any()
    # the flagged frame leaves: only its archive classes remain, and they survive its leaving
    A.ba_marginalize_frame(1)
    left = mm.set_from_kf(None, None, *k["exp"][101])
    assert len(left) >= 50
    for mode, dr in ((0, draws), (1, None)):
        assert_cloud(A.map_frame_cloud(101, mode, th_sc, BIG, 0.0, draws=dr), cloud_model(left, ci, mode, th_sc, BIG, 0.0, dr), "a frame that has left")
    a.frame_id, a.n_draws = fid, 8 * len(rec)
    assert A.L.nalo_map_frame_cloud(A.h_, C.byref(a)) == ERR_STATE                             # a window frame between marginalize_frame and the carry
    assert_frame(A, 101, *k["exp"][101], "after the frame left")


def test_enabling_is_refused_on_a_sharded_window(small):
    N = small["B"]                                                                             # (its read-backs were taken when the fixture was made)
    N.ba_set_allreduce(lambda ptr, n: None)
    assert N.L.nalo_map_enable(N.h_, 1, 0) == ERR_STATE
    assert N.L.nalo_map_enable(N.h_, 1, -1) == ERR_ARG


def test_decisions_made_while_the_map_was_off_are_refused():
    S = scene(640, 480, 4, 400)
    c = make_ctx(S)
    c.ba_set_point_history(*sc.plant_history(400, 4))
    c.ba_linearize(False)
    c.ba_linearize(True)
    c.ba_flag_points(sc.flag_sets(4)[1])
    c.map_enable()
    st = c.ba_get_residuals()[0]
    assert c.L.nalo_ba_marginalize_flagged(c.h_, None, None, None, None) == ERR_STATE
    assert np.array_equal(c.ba_get_residuals()[0], st)
    c.map_enable(False)
    c.ba_marginalize_flagged()                                                                 # off again: the call of before
    c.close()


# ------------------------------------------------------------------------------------------------ 2: planted sizes
def planted_scene(sizes):
    """W = 6, 600 points per host, full graph, positive depths: a point is removed iff its lastResiduals[0] state is planted OOB (isOOB's second clause; null
    pointers, so that no pass rewrites the states). Marginalised or dropped is the data's choice (H on both sides of 50)."""
    W, P = 6, 3600
    s = 3e-4
    win = synth.make_window(w=640, h=480, W=W, P=P, seed=sc.SEED, n_extra=0, step_z=0.8 * s, step_x=0.03 * s, full_graph=True)
    S = dict(win=win, idepth=np.abs(win.idepth), exists=win.exists, st6=synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004), hp=(win.host == 0).astype(np.int32),
             host=win.host, u=win.u, v=win.v, color=win.color, fids=[100 + i for i in range(W)])
    return S


def plant(S, sizes, seed):
    P = len(S["host"])
    rng = np.random.RandomState(seed)
    ls = np.zeros((P, 2), np.int8)
    for h, n in enumerate(sizes):
        ls[rng.permutation(np.nonzero(S["host"] == h)[0])[:n], 0] = lm.OOB
    return np.full(P, 5, np.int32), np.full((P, 2), -1, np.int8), ls


def test_planted_sizes_chunk_borders_and_growth():
    sizes = [0, 1, 255, 256, 257, 513]
    S = planted_scene(sizes)
    A = make_ctx(S)
    A.map_enable(chunk_points=300)
    none = np.zeros(6, np.uint8)
    acc = {f: [[], []] for f in S["fids"]}
    snap = {}
    for rnd, sz in enumerate((sizes, sizes[::-1])):
        if rnd:
            issue(A, S)                                                                        # a second window on the same context: 3600 valid points again
        A.ba_set_point_history(*plant(S, sz, 20 + rnd))
        A.ba_linearize(False)
        k = keyframe(A, S, none)
        removed = [int(((S["host"] == h) & (k["dec"] != lm.KEEP)).sum()) for h in range(6)]
        print("MAP planted round %d: removed per host %s, marginalised %d" % (rnd, removed, int((k["dec"] == 3).sum())))
        assert removed == list(sz)
        for f in S["fids"]:
            acc[f][0].append(k["exp"][f][0]); acc[f][1].append(k["exp"][f][1])
            assert_frame(A, f, np.concatenate(acc[f][0]), np.concatenate(acc[f][1]), "round %d" % rnd)
        if rnd == 0:
            assert (k["dec"] == 3).sum() >= 50 and ((k["dec"] == 1) | (k["dec"] == 2)).sum() >= 50
            snap = {f: A.map_get_frame(f) for f in S["fids"]}
            assert A.map_world_points(100, np.eye(3, 4)).shape == (0, 3) and A.map_counts(100) == (0, 0)      # host 0 lost nothing: a frame without a marginalised point
            dec2, _, _ = A.ba_flag_points(none)                                                # a keyframe that removes nothing
            assert (dec2 == lm.KEEP).all()
            A.ba_marginalize_flagged()
            for f in S["fids"]:
                assert mm.records_equal(A.map_get_frame(f), snap[f])
    for f in S["fids"]:                                                                        # what was archived before the growth has not changed
        now = A.map_get_frame(f)
        n2, n3 = len(acc[f][0][0]), len(acc[f][1][0])
        m2 = len(acc[f][0][0]) + len(acc[f][0][1])
        assert mm.records_equal(np.concatenate([now[:n2], now[m2:m2 + n3]]), snap[f])
    A.close()


# ------------------------------------------------------------------------------------------------ 3: several keyframes of the device chain
def test_three_keyframes_of_the_device_chain():
    WW, KF = 5, 3
    s = 3e-4
    win = synth.make_window(w=640, h=480, W=WW, P=1500, seed=sc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    F = WW + KF
    rng = np.random.RandomState(sc.SEED + 3)
    st6 = np.zeros((F, 6))
    st6[1:, :3] = 0.004 * rng.randn(F - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * rng.randn(F - 1, 3)
    A = binding.Context(win.w, win.h, win.K, n_slots=F)
    for i in range(F):
        A.frame_upload(i, win.images[i])
    A.ba_set_prior_carry(True)
    fids = [200 + i for i in range(WW)]
    A.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=st6[:WW], frame_ids=fids)
    A.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    A.ba_set_residuals(win.exists)
    ng0, lt0, ls0 = lm.default_history(win.exists)
    ls0[win.host == WW - 1, 0] = lm.IN
    A.ba_set_point_history(ng0, lt0, ls0)
    A.map_enable(chunk_points=300)
    S = dict(host=win.host.copy(), u=win.u, v=win.v, color=win.color, hp=np.zeros(len(win.host), np.int32), fids=fids)
    acc, gone, total = {}, [], 0
    for kf in range(KF):
        if kf:
            A.ba_carry_window(A.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            m = A.ba_carry_map()
            S = dict(host=S["host"][m] - 1, u=S["u"][m], v=S["v"][m], color=S["color"][m], hp=S["hp"][m], fids=S["fids"][1:] + [200 + WW - 1 + kf])
        A.ba_linearize(False)
        A.ba_linearize(True)
        ff = np.zeros(WW, np.uint8); ff[0] = 1
        k = keyframe(A, S, ff)
        total += int((k["dec"] != lm.KEEP).sum())
        print("MAP chain keyframe %d: decisions %s" % (kf, np.bincount(k["dec"], minlength=4).tolist()))
        for f in S["fids"]:
            acc.setdefault(f, [[], []])
            acc[f][0].append(k["exp"][f][0]); acc[f][1].append(k["exp"][f][1])
        A.ba_marginalize_frame(0)
        gone.append(S["fids"][0])
        for f in acc:                                                                          # frames in the window and frames that have left alike, in run order
            assert_frame(A, f, np.concatenate(acc[f][0]), np.concatenate(acc[f][1]), "keyframe %d" % kf)
    assert total >= 300 and all(sum(A.map_counts(f)) >= 50 for f in gone)
    assert max(sum(1 for a, b in zip(*acc[f]) if len(a) + len(b)) for f in acc) >= 2           # some frame's records come from several keyframes' runs
    A.map_reset()
    for f in acc:
        with pytest.raises(binding.NaloError):
            A.map_counts(f)
    A.close()


# ------------------------------------------------------------------------------------------------ 6: the KITTI shape
def test_kitti_shaped_keyframe_end_to_end():
    win, st6, hp = sc.make_scene("kitti")
    S = dict(win=win, idepth=win.idepth, exists=win.exists, st6=st6, hp=hp, host=win.host, u=win.u, v=win.v, color=win.color, fids=[300 + i for i in range(win.W)])
    A = make_ctx(S)
    A.map_enable()
    A.ba_set_point_history(*sc.plant_history(len(win.host), win.W))
    A.ba_linearize(False)
    A.ba_linearize(True)
    k = keyframe(A, S, sc.flag_sets(win.W)[2])
    print("MAP kitti: decisions", np.bincount(k["dec"], minlength=4).tolist(), "marginalised without an active residual", int(((k["dec"] == 3) & (k["post"]["HdiF"] == 0)).sum()))
    assert (np.bincount(k["dec"], minlength=4) >= 100).all()
    ci = calib_inv(A)
    imm = immature_set(12000, win.W, win.w, win.h)
    A.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
    m = np.concatenate([np.linalg.qr(np.random.RandomState(2).randn(3, 3))[0], [[1e5], [-2e4], [3.0]]], 1)
    draws = np.random.RandomState(4).randint(0, 2 ** 31 - 1, 8 * 4000).astype(np.int32)
    for widx, fid in enumerate(S["fids"]):
        assert_frame(A, fid, *k["exp"][fid], "kitti")
        marg = k["exp"][fid][0]
        assert mm.bits_equal(A.map_world_points(fid, m), mm.world_points(marg["u"], marg["v"], marg["idepth"], ci, m)), fid
        rec = frame_records(S, k, fid, widx, imm)
        var, sc4 = clause_values(rec)
        fin = (rec["idepth"] >= 0) & np.isfinite(sc4)
        th = np.median(sc4[fin])
        assert_cloud(A.map_frame_cloud(fid, 0, th, np.median(var), 0.0, draws=draws), cloud_model(rec, ci, 0, th, np.median(var), 0.0, draws), "kitti cloud %d" % fid)
        assert_cloud(A.map_frame_cloud(fid, 1, BIG, BIG, 0.0), cloud_model(rec, ci, 1, BIG, BIG, 0.0, None), "kitti cloud %d mode 1" % fid)
    A.close()
