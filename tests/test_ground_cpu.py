"""The ground-plane state machine without a device: tests/ground_model.py on hand-worked inputs, and the library's context-free C functions
(nalo_ground_update, nalo_ground_set_global_plane, nalo_ground_local_scale; include/nalo_gpu.h) against the model, bit for bit, through
ctypes.CDLL(binding.lib_path())."""
import ctypes as C

import numpy as np
import pytest

import ground_model as gm
from nalo_slam_amd import binding

F = np.float32


def bits(x):
    return np.atleast_1d(np.asarray(x, F)).view(np.uint32).tolist()


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(binding.lib_path())
    binding._ground_argtypes(L)
    return L


# ------------------------------------------------------------------------------------------------ the model on hand-worked inputs
def hand_cluster(n, mask_value, plane, idp=0.5):
    K = (100.0, 100.0, 50.0, 40.0)
    return dict(members=np.arange(n), xx=np.full(n, 50), yy=np.full(n, 40), mask_value=F(mask_value), n=n, n_cloud=n, fitted=1, plane=np.array(plane, F)), np.full(n, idp, F), K


def test_model_score_by_hand():
    # 100 members at Z = 2: every term is 2 / 100 = 0.02f, added 100 times in float
    c, idp, K = hand_cluster(100, 255, (0.25, -0.5, 0.5, -1.5))
    s = F(0)
    for _ in range(100):
        s = F(s + F(F(2) / F(100)))
    scored, mz, sc = gm.score(c, idp, K)
    assert scored == 1 and bits(mz) == bits(s) and s != F(2)                     # the chain of adds does not land on 2 exactly
    assert sc == F(F(F(0.75) * F(1000)) + F(150)) + F(1)                         # (a + c) 1000 + |d| 100 + 100 / 100
    c, idp, K = hand_cluster(101, 255, (0.25, -0.5, 0.5, -1.5))
    assert gm.score(c, idp, K)[2] == F(900)                                      # 100 / 101 == 0
    for n, mv, idv in ((99, 255, 0.5), (100, 199, 0.5), (100, 255, -0.5)):       # n < 100, mask < 200, mid_z < 0
        c, idp, K = hand_cluster(n, mv, (0.25, -0.5, 0.5, -1.5), idv)
        assert gm.score(c, idp, K)[1:] == (gm.mid_z(c, idp, K), gm.SCORE_OUT)
    c, idp, K = hand_cluster(100, 200, (0.25, -0.5, 0.5, -1.5))
    assert gm.score(c, idp, K)[2] == F(901)
    rng = np.random.RandomState(3)                                               # the vectorised sum adds in the same order
    c2 = dict(c, members=np.arange(3000), xx=rng.randint(3, 90, 3000), yy=rng.randint(3, 70, 3000))
    idp2 = rng.uniform(-0.1, 0.9, 3000).astype(F)
    assert bits(gm.mid_z(c2, idp2, K)) == bits(gm.mid_z_fast(c2, idp2, K))
    c["n_cloud"] = 99                                                            # a member that failed the finite test: fitPlane returned false
    assert gm.score(c, idp, K) == (0, F(0), F(0))


def test_model_choice_by_hand():
    mk = lambda pl, mv=255, n=100: hand_cluster(n, mv, pl)[0]
    _, idp, K = hand_cluster(100, 255, (0, 0, 0, 0))
    idp = np.full(200, 0.5, F)
    cl = [mk((0.5, 0.5, 0.5, 1.0)), mk((0.1, 0.9, 0.1, -2.0)), mk((0.1, -0.9, 0.1, -2.0)), mk((0.9, 0.1, 0.9, 1.0))]
    p = gm.choose(cl, idp, K)
    assert p["ran"] == 1 and p["cluster"] == 1 and bits(p["gp_raw"]) == bits([-0.1, -0.9, -0.1, 2.0]) and p["ground_height"] == F(2)     # a tie: the first; b > 0 flips
    assert gm.choose(cl[:3], idp, K)["ran"] == 0
    cl2 = [mk((0.5, 0.5, 0.5, 1.0), n=50) for _ in range(4)]                     # all at 9999999: the first wins
    p = gm.choose(cl2, idp, K)
    assert p["cluster"] == 0 and all(s[2] == gm.SCORE_OUT for s in p["scores"])
    for c in cl2:
        c["fitted"] = 0
    p = gm.choose(cl2, idp, K)
    assert p["ran"] == 1 and p["cluster"] == -1 and not p["gp_raw"].any()
    cl3 = [mk((0.1, -0.0, 0.1, 1.0))] + cl2[:3]                                  # b == -0.0 is not > 0: no flip, the sign bit stays
    assert bits(gm.choose(cl3, idp, K)["gp_raw"]) == bits([0.1, -0.0, 0.1, 1.0])


def test_model_mark_by_hand():
    g_u, g_v = [10, 11, 10], [20, 20, 20]
    just_below = np.nextafter(F(9.5), F(0))
    on, num = gm.mark(g_u, g_v, [1, 1, 0, 1, 1], [9.5, just_below, 10.0, 10.2, 11.4], [19.5, 20.0, 20.0, 20.49, 20.6])
    assert on.tolist() == [1, 0, 0, 1, 0] and num == 2                           # x.5 rounds up, the float below does not; an untested point; v = 21 misses
    rng = np.random.RandomState(0)
    g_u, g_v = rng.randint(3, 30, 200).tolist(), rng.randint(3, 20, 200).tolist()
    cu, cv, te = rng.uniform(-3, 33, 500).astype(F), rng.uniform(-3, 23, 500).astype(F), rng.rand(500) < 0.8
    cu[:3], cv[:3] = [np.nan, 1e20, -1e20], [5.0, 5.0, np.nan]                   # the defined conversion: NaN -> 0, saturation
    a, b = gm.mark(g_u, g_v, te, cu, cv), gm.mark_fast(g_u, g_v, te, cu, cv)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and 0 < a[1] < 500


def test_gpu_cases_are_what_they_claim():
    """the scenes of test_ground_gpu.py through the model: every case holds the property it is there for"""
    import ground_cases as gc
    import plane_model as pm
    for w, h in ((64, 48), (80, 48)):
        got = {}
        for name, (sc, seed, _) in gc.score_scenes(w, h).items():
            m = pm.fit_planes(sc["u"], sc["v"], sc["idp"], sc["mask"], w, h, sc["K"], pm.make_draws(seed), min_points=20)
            got[name] = (m, gm.choose(m, sc["idp"], sc["K"]))
        sizes = {c["n"]: s for c, s in zip(got["sizes"][0], got["sizes"][1]["scores"])}
        assert sizes[99][2] == gm.SCORE_OUT and all(sizes[n][2] != gm.SCORE_OUT for n in (100, 101, 130))
        masks = {float(c["mask_value"]): s for c, s in zip(*[got["masks"][0], got["masks"][1]["scores"]])}
        assert masks[199.0][2] == gm.SCORE_OUT and all(masks[v][2] != gm.SCORE_OUT for v in (200.0, 201.0, 255.0))
        neg = [s for c, s in zip(got["negative"][0], got["negative"][1]["scores"]) if c["mask_value"] == 255][0]
        assert neg[1] < 0 and neg[2] == gm.SCORE_OUT
        z = got["zero_idepth"]
        assert z[0][0]["fitted"] == 1 and z[0][0]["n_cloud"] == 149 and z[1]["scores"][0][0] == 0 and z[1]["cluster"] != 0
        assert got["all_out"][1]["cluster"] == 0 and all(s[2] == gm.SCORE_OUT for s in got["all_out"][1]["scores"])
        assert got["zero_mask_wins"][1]["cluster"] == 0 and got["zero_mask_wins"][0][0]["mask_value"] == 0
        assert got["three"][1]["ran"] == 0
        bp = got["b_positive"]
        assert bp[0][bp[1]["cluster"]]["plane"][1] > 0 and bp[1]["gp_raw"][1] < 0
        assert got["big"][0][0]["n"] == 1025 and got["big"][1]["scores"][0][0] == 1
        col = got["column"]
        sc_ = [s[2] for s in col[1]["scores"]]
        win = col[1]["cluster"]
        assert sorted(sc_)[0] == sorted(sc_)[1] == F(-1000) and win == sc_.index(F(-1000))          # two equal real scores: the first wins
        assert col[1]["gp_raw"][1] == 0 and np.signbit(col[1]["gp_raw"][1]) and col[1]["gp_raw"][0] == -1     # b == -0.0 is not > 0: no flip


# ------------------------------------------------------------------------------------------------ the C functions against the model
def c_pick(p):
    k = binding.GroundPick()
    k.ran, k.cluster = int(p["ran"]), int(p["cluster"])
    for j in range(4):
        k.gp_raw[j] = float(p["gp_raw"][j])
    k.ground_height = float(p["ground_height"]) if p["ground_height"] is not None else 123.0      # garbage without a winner: must not be read
    return k


def state_bits_model(trs, g, frames):
    t = [bits([tr.ground_height, tr.last_height]) + [tr.suc_num] for tr in trs]
    gl = [g.scale_fix] + bits([g.init_height, g.last_ScaleRate]) + bits(g.last_gp) + [len(g.old_rate)] + bits(g.old_rate if g.old_rate else np.zeros(0, F))
    fr = [bits(f.groundP) + bits(f.last_ground) + [f.haveground, f.scaleFixed] for f in frames]
    return t, gl, fr


def state_bits_c(trs, g, frames):
    t = [bits([tr.ground_height, tr.last_height]) + [tr.suc_num] for tr in trs]
    gl = [g.scale_fix] + bits([g.init_height, g.last_ScaleRate]) + bits(list(g.last_gp)) + [g.n_old] + bits(list(g.old_rate)[:g.n_old])
    fr = [bits(list(f.groundP)) + bits(list(f.last_ground)) + [f.haveground, f.scaleFixed] for f in frames]
    return t, gl, fr


def pick_of(height, b=-0.98):
    pl = np.array([0.01, b, 0.02, height if b <= 0 else -height], F)
    return dict(ran=1, cluster=2, gp_raw=(-pl if pl[1] > 0 else pl), ground_height=F(abs(pl[3])))


NO_RUN = dict(ran=0, cluster=7, gp_raw=np.full(4, 9, F), ground_height=F(55))           # everything but `ran` is garbage that must not be read
NO_WINNER = dict(ran=1, cluster=-1, gp_raw=np.zeros(4, F), ground_height=None)


def script():
    """heights per keyframe: settle (two alternating trackers need four small differences EACH), latch, prime, fill and rotate old_rate, a rate 50 % off
    everything (outlier), a rise, then a fall that is > 25 % off the last rate but within 25 % of the longer averages (accepted)"""
    h = 1.65
    s = [pick_of(h), pick_of(h + 0.002), NO_RUN, pick_of(h + 0.001), pick_of(h + 0.004), NO_WINNER, pick_of(h + 0.003), pick_of(h), pick_of(h + 0.002), pick_of(h + 0.001),
         pick_of(h + 0.003), pick_of(h + 0.002)]
    s += [pick_of(h)]                                                            # the priming call
    s += [pick_of(h * r, b) for r, b in ((1.0, -0.98), (1.01, 0.97), (0.99, -0.98), (1.0, -0.0), (1.02, -0.98), (1.0, -0.98), (0.98, -0.98), (1.0, -0.98), (1.01, -0.98))]
    s += [NO_RUN, pick_of(h * 1.5), NO_WINNER, pick_of(h * 1.0), pick_of(h * 1.2), pick_of(h * 1.45), pick_of(h * 1.05), pick_of(h * 0.2)]
    return s


@pytest.mark.parametrize("W", [6, 7])
def test_update_scripted_run(lib, W):
    m_tr, m_g = [gm.Tracker(), gm.Tracker()], gm.Globals()
    c_tr, c_g = [binding.ground_tracker(), binding.ground_tracker()], binding.ground_globals()
    m_fr = [gm.Frame() for _ in range(W)]
    c_fr = binding.ground_frames(W)
    assert state_bits_model(m_tr, m_g, m_fr) == state_bits_c(c_tr, c_g, c_fr)    # the initial values
    events = set()
    picks = script()
    assert len(picks) >= 12
    for k, p in enumerate(picks):
        # a keyframe: the oldest frame leaves, a fresh one enters (every second time the frame before the newest is one without a ground: a zero groundP[3]
        # inside the walk for last_ground)
        m_fr = m_fr[1:] + [gm.Frame()]
        for i in range(W - 1):
            C.memmove(C.byref(c_fr[i]), C.byref(c_fr[i + 1]), C.sizeof(binding.GroundFrame))
        lib.nalo_ground_frame_init(C.byref(c_fr[W - 1]))
        if k % 2:
            m_fr[W - 2].groundP[3] = 0
            c_fr[W - 2].groundP[3] = 0.0
        before = state_bits_c(c_tr, c_g, c_fr)
        was_fixed, was_primed, n_old, gh_before = m_g.scale_fix, m_g.last_ScaleRate >= 0, len(m_g.old_rate), m_tr[k % 2].ground_height
        last_rate = m_g.last_ScaleRate
        gm.update(p, m_tr[k % 2], m_g, m_fr)
        kp = c_pick(p)
        assert lib.nalo_ground_update(C.byref(kp), C.byref(c_tr[k % 2]), C.byref(c_g), c_fr, W) == 0
        after = state_bits_c(c_tr, c_g, c_fr)
        assert state_bits_model(m_tr, m_g, m_fr) == after, (k, p)
        if not p["ran"]:
            assert after == before
            events.add("no_run_fixed" if was_fixed else "no_run")
            continue
        if p["cluster"] < 0:
            assert m_tr[k % 2].ground_height == gh_before                        # only ground_height is kept: it runs the machine again
            events.add("no_winner_fixed" if was_fixed else "no_winner")
        if m_g.scale_fix and not was_fixed:
            events.add("latched")
            assert m_tr[k % 2].suc_num == 4 and m_tr[1 - k % 2].suc_num <= 4
        elif was_fixed and not was_primed:
            events.add("primed")
            assert len(m_g.old_rate) == 1 and not m_fr[-1].haveground and not m_fr[-1].groundP.any()
        elif was_fixed and p["cluster"] >= 0:
            rate = F(p["ground_height"] / m_g.init_height)
            off_last = float(F(abs(F(last_rate - rate)) / last_rate)) > 0.25
            if not m_fr[-1].haveground:
                events.add("outlier")
                assert off_last and bits(m_fr[-1].groundP) == bits(m_g.last_gp) and m_g.last_ScaleRate == last_rate
            else:
                events.add("accepted_off_last" if off_last else "accepted")
                assert bits(m_fr[-1].groundP) == bits(p["gp_raw"])
            if n_old == 7:
                events.add("rotated")
                assert len(m_g.old_rate) == 7
        if m_g.scale_fix and W > 6 and m_fr[-1].last_ground[3] != 0:
            events.add("last_ground")
            src = [f for f in m_fr[W - 2:0:-1] if f.groundP[3] != 0][0]
            assert bits(m_fr[-1].last_ground) == bits(src.groundP)
            if m_fr[W - 2].groundP[3] == 0:
                events.add("last_ground_skipped_zero")
    want = {"no_run", "no_winner", "latched", "primed", "accepted", "rotated", "outlier", "accepted_off_last", "no_run_fixed", "no_winner_fixed"}
    if W > 6:
        want |= {"last_ground", "last_ground_skipped_zero"}
    else:
        assert not any(f.last_ground.any() for f in m_fr)
    assert want <= events, want - events


def frames_pair(planes):
    m = [gm.Frame() for _ in planes]
    c = binding.ground_frames(len(planes))
    for i, p in enumerate(planes):
        m[i].groundP = np.array(p, F)
        m[i].haveground = 1
        c[i].haveground = 1
        for j in range(4):
            c[i].groundP[j] = float(F(p[j]))
    return m, c


def run_global(lib, planes, M, max_frames=7):
    m, c = frames_pair(planes)
    fixed_m, gp_m, lgh_m = gm.set_global_plane(m, M, max_frames)
    gp, bk, lgh = np.full(4, 77.0), np.full(4, 77.0), np.full(1, 77, F)
    Mc = np.ascontiguousarray(M, np.float64).reshape(-1)
    rc = lib.nalo_ground_set_global_plane(c, len(planes), max_frames, binding._d(Mc), binding._d(gp), binding._d(bk), binding._f(lgh))
    assert rc == int(fixed_m)
    if fixed_m:
        assert gp.view(np.uint64).tolist() == gp_m.view(np.uint64).tolist() == bk.view(np.uint64).tolist() and bits(lgh) == bits(lgh_m)
    else:
        assert (gp == 77).all() and (bk == 77).all() and lgh[0] == 77            # nothing written
    return fixed_m, gp_m, lgh_m


def test_set_global_plane(lib):
    base = [0.0, -1.0, 0.0, 1.5]
    M = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]])
    same = [list(base) for _ in range(7)]
    fixed, gp, lgh = run_global(lib, same, M)
    # piw = M^T pih by hand: (R^T n, t . n + d) with n = (0, -1, 0): R^T n = (-1, 0, 0), t . n = -2
    assert fixed and gp.tolist() == [-1.0, 0.0, 0.0, -0.5] and lgh == F(1.5)
    assert not run_global(lib, same[:6], M)[0]                                   # W < max_frames
    assert run_global(lib, same[:6], M, max_frames=6)[0]
    for bad in ([np.nan, -1.0, 0.0, 1.5], [0.0, -1.0, 0.0, 0.0], [0.0, -1.25, 0.0, 1.5], [0.0, 1.25, 0.0, 1.5], [0.0, -1.0, 0.0, np.nan]):
        for at in (1, 3, 5):                                                     # anywhere in the chain W-2 .. 1
            pl = [list(base) for _ in range(7)]
            pl[at] = bad
            assert not run_global(lib, pl, M)[0], (bad, at)
    pl = [list(base) for _ in range(7)]
    pl[6] = [np.nan, 5.0, 0.0, 0.0]                                              # the newest frame is not in the chain
    assert run_global(lib, pl, M)[0]
    pl[0] = [0.0, -1.0, 0.0, 1.5 + 0.19]                                         # frame 0 enters as lastpi only: one difference of 0.19
    assert run_global(lib, pl, M)[0]
    pl[0] = [0.0, -1.0, 0.0, 1.5 + 0.21]
    assert not run_global(lib, pl, M)[0]
    # either side of 0.2 from several small steps, and a non-trivial plane against the model
    for step, want in ((0.039, True), (0.041, False)):
        pl = [[0.02, -0.99, 0.05, 1.5 + step * i] for i in range(7)]
        Mr = np.array([[0.36, 0.48, -0.8, 0.3], [-0.8, 0.6, 0.0, -1.7], [0.48, 0.64, 0.6, 2.9]])
        assert run_global(lib, pl, Mr)[0] == want


def test_local_scale(lib):
    m, c = frames_pair([[0.01, -0.98, 0.02, 1.7]])
    out = np.full(1, 77.0)
    assert lib.nalo_ground_local_scale(C.byref(c[0]), C.c_float(1.65), binding._d(out)) == 1
    want = gm.local_scale(m[0], F(1.65))
    assert out.view(np.uint64)[0] == np.float64(want).view(np.uint64) and want == float(np.float64(F(1.65)) / np.float64(F(1.7)))
    assert binding.ground_local_scale(c[0], 1.65) == want
    m[0].haveground = 0
    c[0].haveground = 0
    out[:] = 77.0
    assert lib.nalo_ground_local_scale(C.byref(c[0]), C.c_float(1.65), binding._d(out)) == 0 and out[0] == 77.0 and gm.local_scale(m[0], F(1.65)) is None


def test_reset_global_plane_and_wrappers(lib):
    m, c = frames_pair([[0.0, -1.0, 0.0, 1.5]] * 3)
    c[1].haveground = 0
    Ms = np.stack([np.array([[0.0, -1.0, 0.0, 1.0 + i], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]]) for i in range(3)])
    idx, gp = binding.ground_reset_global_plane(c, Ms)
    assert idx == 0 and gp.tolist() == [-1.0, 0.0, 0.0, -0.5]                    # W-2 has no ground: frame 0
    fixed, gp2, bk2, lgh = binding.ground_set_global_plane(c, Ms[0], max_frames=3)
    assert fixed and gp2.tolist() == [-1.0, 0.0, 0.0, -0.5] and lgh == F(1.5)
