"""nalo_ba_window_from_initializer - the first BA window issued from the initialiser's level-0 points on the device - against the re-issue it replaces.

Every comparison runs two contexts that hold the same frames and the same initialiser state. A uses the new call. B goes the old way: nalo_init_get_points ->
the literal model of tests/init_window_model.py (FullSystem::initializeFromInitializer, reference FullSystem.cpp:1589-1648, and the insertion :1335-1348) ->
nalo_imm_create -> nalo_ba_set_window / set_points / set_residuals / set_point_history with explicit arrays; B is given exactly the frame states A returned.
"Equal" is bit for bit.

  1  equality at 640x480 and 1224x368 after three tracked frames: launch configuration, frames, prior, points, residual states, history, the linearised system,
     the result of nalo_ba_optimize; the map; the returned poses against the model's fp64 ones
  2  the scale: sumID, numID, rescaleFactor equal the sequential float loop on an input where a pairwise and an fp64 sum give another float
  3  keep patterns planted through the draws, and all ~61 k points of 1920x1072 kept
  4  non-finite rejection
  5  idempotence, and the initialiser untouched
  6  every refusal of the header, each after a valid window was issued
  7  the bootstrap chain: two keyframes from the issued window on both contexts, every read-back equal after every step. The four window calls of a keyframe run
     in the reference's order - optimize, setCoarseTrackingRef, flagPointsForRemoval, marginalizePointsF (FullSystem.cpp:1362, 1404, 1446, 1453):
     nalo_trk_set_ref_from_window needs the fix pass nalo_ba_optimize ends with, which nalo_ba_marginalize_flagged re-linearises away.

The initialiser's LM loop is run once, on A; B is handed A's carried state (nalo_init_set_state / nalo_init_set_points), so that the two start from the same bits
whatever the order of the device's sums. That also leaves A with the device as the newer side and B with the host mirror - and test 2, which plants iR through
nalo_init_set_points on both, runs A from the host mirror too."""
import ctypes as C
import types

import numpy as np
import pytest

import init_window_model as iw
import lifecycle_model as lm
from imm_helpers import host_to_new
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
MAXD = 2 ** 31 - 1                                                          # the draw that is always skipped while keepPercentage < 1; 0 is always kept
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ two contexts, one initialiser state
def carried(c):
    """everything trackFrame carries, as nalo_init_set_state / nalo_init_set_points take it"""
    pts = []
    for l in range(c.levels):
        p, q = c.init_points(l), c.init_carried(l)
        d = {k: p[k] for k in ("idepth", "iR", "isGood", "lastHessian", "energy")}
        d.update(q)
        d["iRSumNum"] = np.zeros(len(p["iR"]), np.float32)
        pts.append(d)
    return dict(state=c.init_state(), points=pts)


class Pair:
    def __init__(self, w, h, frames=5, track=3, n_slots=None, seed=3):
        self.win = win = synth.make_window(w=w, h=h, W=2, P=20, seed=seed, n_extra=frames - 2, step_z=0.15, yaw_deg=0.1)
        self.track = track
        rp = np.random.RandomState(seed).randint(0, 256, w * h).astype(np.uint8)
        self.a, self.b = [binding.Context(w, h, win.K, n_slots=n_slots or frames + 1) for _ in range(2)]
        for c in (self.a, self.b):
            for i in range(frames):
                c.frame_upload(i, win.images[i])
            c.pixsel_set_random(rp)
            num, _ = c.init_set_first(0)
        self.n = int(num[0])
        for i in range(1, track + 1):
            self.a.init_track_frame(i)
        if track:
            self.b.init_set_carried(carried(self.a))
        self.rng = np.random.RandomState(seed + 1)

    def draws(self):
        return self.rng.randint(0, 2 ** 31, self.n).astype(np.int32)          # what rand() of a 31-bit libc returns

    def close(self):
        self.a.close(); self.b.close()


_PAIRS = {}


def pair(w, h):
    if (w, h) not in _PAIRS:
        _PAIRS[(w, h)] = Pair(w, h)
    return _PAIRS[(w, h)]


@pytest.fixture(scope="module", autouse=True)
def _close_pairs():
    yield
    for p in _PAIRS.values():
        p.close()
    _PAIRS.clear()


def issue_a(a, draws, density=2000.0, slots=(0, 3)):
    """-> (the two frame states as the call set them, scale, stats)"""
    return a.ba_window_from_initializer(a.frame_state(slots[0], EYE, frame_id=0), a.frame_state(slots[1], EYE, frame_id=1), draws, density)


def issue_b(b, frames, draws, density=2000.0):
    """the old route, with the frame states A returned -> the model's window"""
    p, T = b.init_points(0), b.init_state()["thisToNext"]
    sel = iw.select(draws, density)
    px = np.array([iw.pixel(p["u"][i], p["v"][i]) for i in sel], np.int32).reshape(-1, 2)
    color, weights, gradH, eth = b.imm_create(frames[0].slot, px[:, 0], px[:, 1])
    m = iw.window(p["u"], p["v"], p["iR"], sel, eth, T)
    fin = np.isfinite(eth)
    arr = (binding.FrameState * 2)(*frames)
    cal = np.asarray(b.K, np.float64)
    b._ck(b.L.nalo_ba_set_window(b.h_, 2, arr, binding._d(cal), binding._d(cal)))
    b.W = 2
    b.ba_set_points(m["host"], m["u"], m["v"], m["idepth"], color[fin], weights[fin], has_prior=m["has_prior"], idepth_zero=m["idepth"])
    b.ba_set_residuals(m["exists"])
    b.ba_set_point_history(*m["hist"])
    return m


def window_state(c, residual_floats=False):
    """every read-back of the window, floats as their bits"""
    fr, pre, cal = c.ba_get_frames()
    HM, bM = c.ba_get_prior()
    pts = c.ba_get_points()
    res = c.ba_get_residuals()
    ng, lt, ls = c.ba_get_point_history()
    s = dict(W=c.W, P=c.P, cfg=c.ba_launch_config(), frames=bytes(fr), PRE_worldToCam=u64(pre), calib=u64(cal), HM=u64(HM), bM=u64(bM),
             idepth_zero=u32(c.ba_get_idepth_zero(c.P)), res_state=res[0], res_active=res[1], numGood=ng, last_target=lt, last_state=ls)
    s.update({"pt_" + k: u32(v) for k, v in pts.items()})
    if residual_floats:
        s.update(JpJdF=u32(res[2]), energy_new=u32(res[3]), centre=u32(res[4]))
    return s


def assert_same(sa, sb, what):
    assert sa.keys() == sb.keys()
    for k in sa:
        x, y = sa[k], sb[k]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.array_equal(x, y), (what, k, x.shape, y.shape, int((x != y).sum()) if x.shape == y.shape else -1)
        else:
            assert x == y, (what, k, x, y)


def assert_same_windows(a, b, what, optimize=False):
    assert_same(window_state(a), window_state(b), what)
    ea, eb = a.ba_linearize(False), b.ba_linearize(False)
    assert np.array_equal(u64([ea]), u64([eb])) and np.isfinite(ea), (what, "energy", ea, eb)
    assert np.array_equal(u64(a.ba_get_acc13()), u64(b.ba_get_acc13())), (what, "acc13")
    if optimize:
        ra, rb = a.ba_optimize(), b.ba_optimize()
        assert np.array_equal(u64([ra]), u64([rb])) and ra > 0, (what, "rmse of nalo_ba_optimize", ra, rb)
        assert_same(window_state(a, True), window_state(b, True), what + ": after nalo_ba_optimize")


def check_issue(a, b, draws, density, what, optimize=False, slots=(0, 3)):
    """A's call, B's re-issue, the comparison -> (model, stats, frames)"""
    frames, scale, stats = issue_a(a, draws, density, slots)
    m = issue_b(b, frames, draws, density)
    P = len(m["src"])
    n = len(draws)
    assert stats == (n, n - len(iw.select(draws, density)), m["rejected"], P) and a.P == P, (what, stats)
    src = a.ba_init_window_map()
    assert np.array_equal(src, m["src"]) and (np.diff(src) > 0).all(), what
    for got, want in zip(scale, m["scale"]):
        assert u32([got])[0] == u32([want])[0], (what, "scale", scale, m["scale"])
    ng, lt, ls = a.ba_get_point_history()
    assert (ng == 0).all() and (lt == np.int8([1, -1])).all() and (ls == lm.IN).all(), what
    st = a.ba_get_residuals()[0]
    assert (st[:, 0] == -1).all() and (st[:, 1] == lm.IN).all(), what
    assert_same_windows(a, b, what, optimize)
    return m, stats, frames


# ------------------------------------------------------------------------------------------------ 1: equality
@pytest.mark.parametrize("w,h", [(640, 480), (1224, 368)])
def test_equal_to_the_reissue(w, h):
    pr = pair(w, h)
    a, b = pr.a, pr.b
    iR = a.init_points(0)["iR"]
    assert (iR != 1).sum() > 0.5 * pr.n, "iR has not left 1"
    draws = pr.draws()
    for c in (a, b):
        c.ba_set_prior_carry(True)                                           # the issue starts from a zero prior whatever this says
    m, stats, frames = check_issue(a, b, draws, 2000.0, "%dx%d" % (w, h), optimize=True)
    for c in (a, b):
        c.ba_set_prior_carry(False)
    print("INIT-WINDOW %dx%d: n %d, skipped %d, rejected %d, P %d, rescaleFactor %.6g" % ((w, h) + stats + (m["scale"][2],)))
    assert 1500 < stats[3] < 2500
    # the frame states the call returned: the first frame exactly, the entering pose within two 3-term rotations' worth of roundings of the model's fp64 one
    f0, f1 = frames
    assert np.array_equal(np.array(f0.worldToCam_evalPT).reshape(3, 4), EYE)
    for f in frames:
        assert not np.any(np.array(f.state)) and not np.any(np.array(f.state_zero))
    assert (f0.slot, f0.frame_id, f1.slot, f1.frame_id) == (0, 0, 3, 1)
    got, want = np.array(f1.worldToCam_evalPT).reshape(3, 4), m["poses"][1]
    bound = 16 * 2.0 ** -52 * max(1.0, np.linalg.norm(want[:, 3]))
    print("INIT-WINDOW %dx%d: pose difference %.3g, bound %.3g, |t| %.4g" % (w, h, np.abs(got - want).max(), bound, np.linalg.norm(want[:, 3])))
    assert np.abs(got - want).max() <= bound and np.linalg.norm(want[:, 3]) > 0


# ------------------------------------------------------------------------------------------------ 2: the scale
def planted_iR(n):
    """values around 1 whose sequential float sum differs from a pairwise and from an fp64 sum (searched on the CPU)"""
    for seed in range(100):
        iR = np.random.RandomState(seed).uniform(0.3, 3.0, n).astype(np.float32)
        seq = iw.scale(iR)[0]
        if seq != iw.pairwise_sum(iR) and seq != iw.fp64_sum(iR):
            return iR, seed
    raise AssertionError("no seed separates the sequential sum from the others")


def test_the_scale_is_the_sequential_sum():
    pr = pair(640, 480)
    a, b = pr.a, pr.b
    before = carried(a)
    iR, seed = planted_iR(pr.n)
    sumID, numID, rescale = iw.scale(iR)
    assert sumID != iw.pairwise_sum(iR) and sumID != iw.fp64_sum(iR)          # otherwise the input proves nothing
    try:
        for c in (a, b):
            c._ck(c.L.nalo_init_set_points(c.h_, 0, pr.n, None, None, binding._f(iR), *([None] * 8)))
        frames, scale, stats = issue_a(a, np.zeros(pr.n, np.int32))
        print("INIT-WINDOW scale (seed %d): sequential %r, pairwise %r, fp64 %r, device %r" % (seed, sumID, iw.pairwise_sum(iR), iw.fp64_sum(iR), scale[0]))
        assert [u32([x])[0] for x in scale] == [u32([x])[0] for x in (sumID, numID, rescale)], (scale, (sumID, numID, rescale))
        assert stats == (pr.n, 0, 0, pr.n)
        m = issue_b(b, frames, np.zeros(pr.n, np.int32))
        assert_same_windows(a, b, "planted iR")
        assert np.array_equal(u32(a.ba_get_points()["idepth"]), u32((iR * rescale).astype(np.float32)))
    finally:
        for c in (a, b):
            c.init_set_carried(before)


# ------------------------------------------------------------------------------------------------ 3: keep patterns
def straddling_draws(n, density=2000.0):
    keep = iw.keep_percentage(density, n)
    lo = int(np.floor(float(keep) * 2147483648.0))
    d = lo - 200
    while not iw.skipped(d + 1, keep):
        d += 1
    return [d, d + 1, lo, lo + 1]


@pytest.mark.parametrize("case", ["first", "last", "middle", "block edges", "all", "straddle"])
def test_keep_patterns_by_planted_draws(case):
    pr = pair(640, 480)
    a, b, n = pr.a, pr.b, pr.n
    assert n > 2000 + 257
    draws = np.full(n, MAXD, np.int64)
    density = 2000.0
    if case == "all":
        density, want = 1e9, np.arange(n)
    elif case == "straddle":
        vals = straddling_draws(n)
        at = [5, 6, 300, 301]
        draws[at] = vals
        keep = iw.keep_percentage(density, n)
        want = np.array([i for i, d in zip(at, vals) if not iw.skipped(d, keep)])
        assert 1 <= len(want) < 4                                            # the four values fall on both sides of the rule
    else:
        want = np.array(dict(first=[0], last=[n - 1], middle=[n // 2])[case] if case != "block edges" else [0, 63, 64, 255, 256, n - 1])
        draws[want] = 0
    draws = draws.astype(np.int32)
    assert np.array_equal(iw.select(draws, density), want)
    m, stats, _ = check_issue(a, b, draws, density, case)
    assert np.array_equal(m["src"], want) and stats == (n, n - len(want), 0, len(want))


def test_all_kept_at_1920x1072():
    """~61 k level-0 points, 241 point blocks: order, map and points equal to B's. The initialiser is not tracked here (that is seconds of makeNN and LM at this
    size): iR is planted through nalo_init_set_points and thisToNext through nalo_init_set_state"""
    w, h = 1920, 1072
    pr = Pair(w, h, frames=2, track=0, n_slots=2)
    try:
        a, b, n = pr.a, pr.b, pr.n
        assert n > 50000
        iR = np.random.RandomState(9).uniform(0.3, 3.0, n).astype(np.float32)
        T = np.concatenate([synth.so3_exp(np.array([0.01, -0.02, 0.005])), np.array([[0.05], [-0.01], [0.3]])], axis=1)
        for c in (a, b):
            c._ck(c.L.nalo_init_set_points(c.h_, 0, n, None, None, binding._f(iR), *([None] * 8)))
            c._ck(c.L.nalo_init_set_state(c.h_, binding._d(np.ascontiguousarray(T.reshape(-1))), binding._d(np.zeros(2)), 1, 7, 1))
        draws = pr.draws()
        m, stats, frames = check_issue(a, b, draws, 1e9, "1920x1072", slots=(0, 1))
        assert stats == (n, 0, 0, n) and a.ba_launch_config()["nblocks"] == (n + 255) // 256 > 200
        got, want = np.array(frames[1].worldToCam_evalPT).reshape(3, 4), m["poses"][1]
        assert np.abs(got - want).max() <= 16 * 2.0 ** -52 * max(1.0, np.linalg.norm(want[:, 3]))
        assert m["scale"][0] != iw.pairwise_sum(iR)
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 4: non-finite rejection
def test_non_finite_points_are_rejected():
    pr = pair(640, 480)
    a, b, n = pr.a, pr.b, pr.n
    draws = pr.draws()
    p = a.init_points(0)
    sel = iw.select(draws, 2000.0)
    px = np.array([iw.pixel(p["u"][i], p["v"][i]) for i in sel])
    # three kept points that no other kept point comes near: a NaN texel spoils every pattern whose bilinear footprint touches it
    chosen = []
    for k in range(len(sel) // 4, len(sel)):
        d = np.abs(px - px[k]).max(axis=1)
        d[k] = 99
        if d.min() > 6 and all(np.abs(px[k] - px[j]).max() > 12 for j in chosen):
            chosen.append(k)
        if len(chosen) == 3:
            break
    assert len(chosen) == 3
    img = pr.win.images[0].copy()
    for k in chosen:
        img[px[k][1], px[k][0]] = np.nan
    try:
        for c in (a, b):
            c.frame_upload(0, img)                                           # after setFirst: the initialiser's points stand, the slot holds the NaNs at call time
        m, stats, _ = check_issue(a, b, draws, 2000.0, "NaN")
        assert stats[2] == 3 and m["rejected"] == 3
        src = a.ba_init_window_map()
        assert not np.isin(sel[chosen], src).any() and np.array_equal(src, np.delete(sel, chosen))
    finally:
        for c in (a, b):
            c.frame_upload(0, pr.win.images[0])


# ------------------------------------------------------------------------------------------------ 5: idempotence
def init_readbacks(c):
    s = c.init_state()
    out = [s["thisToNext"].copy(), s["aff"].copy(), np.array([s["snapped"], s["frameID"], s["snappedAt"], s["n_evals"]])]
    for l in range(c.levels):
        out += list(c.init_points(l).values()) + list(c.init_carried(l).values())
    return out


def test_a_second_call_gives_the_same_window_and_the_initialiser_is_untouched():
    pr = pair(640, 480)
    a = pr.a
    draws = pr.draws()
    before = init_readbacks(a)
    f1, sc1, st1 = issue_a(a, draws)
    s1, map1 = window_state(a), a.ba_init_window_map()
    a.ba_optimize()                                                           # the window moves in between
    f2, sc2, st2 = issue_a(a, draws)
    assert_same(s1, window_state(a), "second call")
    assert np.array_equal(map1, a.ba_init_window_map()) and st1 == st2 and np.array_equal(u32(sc1), u32(sc2))
    assert bytes(f1[0]) == bytes(f2[0]) and bytes(f1[1]) == bytes(f2[1])
    after = init_readbacks(a)
    assert len(before) == len(after)
    for x, y in zip(before, after):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8) if x.dtype != bool else x, y.view(np.uint8) if y.dtype != bool else y)


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_leave_the_window_as_it_was():
    pr = Pair(640, 480, frames=3, track=1, n_slots=5)                         # slots 3 and 4 never get a pyramid
    a, b, n = pr.a, pr.b, pr.n
    try:
        draws = pr.draws()
        m, stats, frames = check_issue(a, b, draws, 2000.0, "valid", slots=(0, 1))
        a.ba_optimize()
        held = window_state(a, True)
        last = a.ba_init_window_last()

        def refused(c, code, held, first=0, entering=1, d=draws, density=2000.0, raw=None):
            args = c.init_window_args(c.frame_state(first, EYE), c.frame_state(entering, EYE, frame_id=1), d, density)
            if raw is not None:
                raw(args)
            rc = c.L.nalo_ba_window_from_initializer(c.h_, C.byref(args))
            msg = c.L.nalo_last_error(c.h_)
            assert rc == code and msg.startswith(b"nalo_ba_window_from_initializer"), (rc, msg)
            assert_same(window_state(c, True), held, msg.decode())
            return msg

        assert a.L.nalo_ba_window_from_initializer(a.h_, None) == ERR_ARG                    # a NULL argument
        assert_same(window_state(a, True), held, "NULL args")
        refused(a, ERR_ARG, held, d=None)                                                    # ... and NULL draws

        def fewer(args):
            args.n_draws = n - 1
        refused(a, ERR_ARG, held, raw=fewer)                                                 # n_draws != numPoints[0]
        refused(a, ERR_ARG, held, d=np.concatenate([draws, [0]]))
        for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
            refused(a, ERR_ARG, held, density=bad)
        refused(a, ERR_ARG, held, first=1, entering=2)                                       # first.slot is not the initialiser's first slot
        refused(a, ERR_ARG, held, first=0, entering=0)                                       # one slot for both frames
        refused(a, ERR_STATE, held, entering=3)                                              # an entering slot without a pyramid
        refused(a, ERR_STATE, held, entering=5)                                              # ... and no such slot
        refused(a, ERR_STATE, held, entering=-1)
        assert b"no point kept" in refused(a, ERR_STATE, held, d=np.full(n, MAXD, np.int32))
        assert a.ba_init_window_last()[1] == last[1] and np.array_equal(a.ba_init_window_map(), m["src"])
        # no initialiser: a context whose window was issued the old way
        c = binding.Context(640, 480, pr.win.K, n_slots=2)
        for i in range(2):
            c.frame_upload(i, pr.win.images[i])
        fs = b.ba_get_frames()[0]
        arr = (binding.FrameState * 2)(*fs)
        cal = np.asarray(c.K, np.float64)
        c._ck(c.L.nalo_ba_set_window(c.h_, 2, arr, binding._d(cal), binding._d(cal)))
        c.W = 2
        color, weights, _, _ = c.imm_create(0, m["u"].astype(np.int32), m["v"].astype(np.int32))
        c.ba_set_points(m["host"], m["u"], m["v"], m["idepth"], color, weights, has_prior=m["has_prior"])
        c.ba_set_residuals(m["exists"])
        c.ba_set_point_history(*m["hist"])
        assert b"no initialiser" in refused(c, ERR_STATE, window_state(c, True))
        c.close()
        # the window is as usable as before: A continues where B does
        b.ba_optimize()
        assert_same_windows(a, b, "after the refusals", optimize=True)
        # a sharded context, then one whose exchange failed (both latch: last)
        a.ba_set_allreduce(lambda ptr, k: None)
        held = window_state(a, True)
        assert b"sharded" in refused(a, ERR_STATE, held)
        a.ba_exchange_failed()
        assert b"failed" in refused(a, ERR_STATE, held)
        # before any call: nothing to report
        d = binding.Context(64, 64, (50.0, 50.0, 31.5, 31.5), n_slots=1)
        assert d.L.nalo_ba_init_window_map(d.h_, None) == ERR_STATE and d.L.nalo_ba_init_window_last(d.h_, None, None) == ERR_STATE
        d.close()
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 7: the bootstrap chain
def test_bootstrap_chain():
    from test_imm_activate_gpu import level1_maps
    from test_imm_carry_gpu import assert_same_state, full_state
    from test_trk_ref_window_gpu import assert_same_ref, tracker_ref
    pr = Pair(640, 480, frames=6, track=3, n_slots=6)
    a, b, win = pr.a, pr.b, pr.win
    both = (a, b)
    try:
        draws = pr.draws()
        m, stats, frames = check_issue(a, b, draws, 2000.0, "chain: issued")
        # the later frames in the window's world: the first frame, the initialiser's scale
        rel = lambda j: synth.se3_mul(win.world_to_cam[j], synth.se3_inv(win.world_to_cam[0]))
        s = np.linalg.norm(np.array(frames[1].worldToCam_evalPT).reshape(3, 4)[:, 3]) / np.linalg.norm(rel(3)[:, 3])

        def pose(j):
            T = rel(j).copy()
            T[:, 3] *= s
            return T

        def same(what, imm=False):
            assert_same(window_state(a, True), window_state(b, True), what)
            if imm:
                assert_same_state(full_state(a), full_state(b), what)

        order = [0, 3]                                                        # the image of every window frame
        act = None
        inserted = appended = 0
        for kf, new in enumerate((4, 5)):
            W = len(order)
            what = "chain: keyframe %d: " % kf
            rm = [c.ba_optimize() for c in both]
            assert np.array_equal(u64(rm[0:1]), u64(rm[1:2])), (what, rm)
            same(what + "optimize")
            for c in both:
                c.trk_set_ref_from_window()
            assert_same_ref(tracker_ref(a), tracker_ref(b))
            ff = np.zeros(W, np.uint8)
            dec = [c.ba_flag_points(ff) for c in both]
            assert np.array_equal(dec[0][0], dec[1][0]) and np.array_equal(u32(dec[0][1]), u32(dec[1][1])) and np.array_equal(dec[0][2], dec[1][2]), what
            for c in both:
                c.ba_marginalize_flagged()
            same(what + "marginalize_flagged")
            newest = order[-1]
            maps = [c.pixsel_make_maps(newest, 600.0, 3) for c in both]
            assert np.array_equal(maps[0][0], maps[1][0]) and maps[0][1:] == maps[1][1:], what
            kw = dict(append_slot=newest, append_host=W - 1)
            if act is not None:                                               # the activation of the keyframe before
                kw.update(fate=act[0], sel=act[1], result=act[2][0])
            st = [c.imm_resident_carry(**kw) for c in both]
            assert st[0][:4] == st[1][:4] and np.array_equal(st[0][4], st[1][4]) and st[0][3] >= 100, (what, st)
            appended += st[0][3]
            same(what + "resident carry", imm=True)
            nw = types.SimpleNamespace(W=W, K=win.K, world_to_cam=np.stack([pose(j) for j in order + [new]]))
            for c in both:
                c.imm_resident_trace(new, *host_to_new(nw, W))
            same(what + "trace", imm=True)
            entering = a.frame_state(new, pose(new), frame_id=W)
            for c in both:
                c.ba_carry_window(entering)
            order.append(new)
            W += 1
            same(what + "carry_window(entering)")
            nw = types.SimpleNamespace(W=W, K=win.K, world_to_cam=np.stack([pose(j) for j in order]))
            KRKi, Kt = level1_maps(nw, W - 1)
            acts = [c.imm_resident_activate(W - 1, KRKi, Kt, np.zeros(W, np.int32), 2.0, 1) for c in both]
            act = acts[0]
            assert np.array_equal(act[0], acts[1][0]) and np.array_equal(act[1], acts[1][1]), what
            assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(act[2], acts[1][2])), what
            cs = [c.ba_carry_window(None, insert_activated=True) for c in both]
            assert cs[0] == cs[1], (what, cs)
            inserted += cs[0][1]
            print("INIT-WINDOW chain keyframe %d: appended %d, selected %d, inserted %d, window P %d" % (kf, st[0][3], len(act[1]), cs[0][1], cs[0][2]))
            same(what + "carry_window(insert_activated)", imm=True)
        rm = [c.ba_optimize() for c in both]
        assert np.array_equal(u64(rm[0:1]), u64(rm[1:2]))
        same("chain: the last optimize")
        assert a.W == 4 and appended >= 200 and inserted >= 1                  # the carry took the issued window over, and the activation reached it
    finally:
        pr.close()
