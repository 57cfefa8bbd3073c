"""nalo_trk_track_tries: trackNewCoarse's whole hypothesis loop in one call (one persistent launch, the loop's decisions taken on the device).

THE BIT CONTRACT. One call over K tries gives, in every record and every output, the bits that K calls of nalo_trk_track give on a TWIN context driven by the
literal loop (track_tries_model.track_new_coarse over Context.trk_track): np.array_equal, no tolerance anywhere between the two forms (bits() below).
Against the fp32 oracle driven by the same loop, where it applies: the decisions are equal (tries run, per-try ok and abort_lvl, who was taken, the winner) and
the numbers of every good try and of the outputs keep test_tracker_gpu.py's bounds (pose_dist < 1e-5, lastResiduals rtol 1e-4, aff 1e-3). One decision is
left out where the oracle's own numbers say it is undecidable at that precision (knife_edge() below): who is taken among good tries that converged to the
same optimum (the 31-try lists at 1224x368 and 140x68: the half-motion try ends on the constant-motion try's residual to 1e-6).

Shapes: 640x480 with tracker_inputs (every level one round, ~30 workgroups; the scenarios and their branch patterns: track_tries_scenes.py, asserted on the
oracle by test_track_tries_cpu.py); 1224x368 with 8750 inputs (two rounds on levels 0 and 1, 64 workgroups); 140x68 with <= 512 points per level through
trk_set_pc (one workgroup: no exchange at all). At 140x68 the synthetic motion between two frames is too large to track at all, so the new frame there is
the reference frame itself, brightened (1.05 I + 3) with seeded noise, and the hypotheses lie around a small motion."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
import track_tries_model as model
import track_tries_scenes as scenes
from helpers import pose_dist, tracker_inputs, true_rel_pose
from nalo_slam_amd import binding, synth
from test_trk_large_gpu import EXPOSURES as EXPOSURES_LARGE, frames

pytestmark = pytest.mark.gpu

_OPEN = []
OUT_KEYS = ("T", "aff", "flow", "achievedRes")


class Rig:
    """a frame pair and a tracking reference on two contexts (the one-call form and its twin), with the fp32 oracle of the same reference"""

    def __init__(self, w, h, K, ref_img, new_img, exposures, inputs=None, clouds=None):
        self.w, self.h, self.K, self.ref_img, self.new_img, self.exposures, self.inputs, self.clouds = w, h, K, ref_img, new_img, list(exposures), inputs, clouds
        self.ctx, self.twin = self.context(), self.context()
        self.levels = self.ctx.levels
        self.dI_ref, _ = orc.make_images(ref_img, self.levels)

    def context(self, new_img=None):
        c = binding.Context(self.w, self.h, self.K, n_slots=2)
        _OPEN.append(c)
        c.frame_upload(0, self.ref_img); c.frame_upload(1, self.new_img if new_img is None else new_img)
        if self.inputs is not None:
            c.trk_set_ref(0, *self.inputs)
        else:
            for l, pc in enumerate(self.clouds):
                c.trk_set_pc(0, l, *pc)
        return c

    def upload_new(self, img):
        """the new frame of both contexts"""
        for c in (self.ctx, self.twin):
            c.frame_upload(1, img)

    def one_call(self, tries, rmse0, c=None, aff_init=(0, 0), **kw):
        c = c or self.ctx
        r = c.trk_track_tries(1, tries, aff_init, (0, 0), self.exposures, self.levels - 1, [rmse0] * 5, **kw)
        r["last_evals"] = c.trk_last_evals()[0]
        return r

    def looped(self, tries, rmse0, c=None, aff_init=(0, 0)):
        """the literal loop over nalo_trk_track; a record's extra = (n_evals, evaluations per level, haveRepeated)"""
        c = c or self.twin

        def track(T0, aff0, min_res):
            ok, T, aff, lr, lf, nev = c.trk_track(1, T0, aff0, (0, 0), self.exposures, self.levels - 1, min_res=min_res)
            return ok, T, aff, lr, lf, nev, c.trk_last_evals()[0].copy(), c.trk_launch_config()["have_repeated"]
        return model.track_new_coarse(track, tries, aff_init, rmse0)

    @functools.lru_cache(maxsize=None)
    def oracle_tracker(self):
        trk = orc.Tracker(self.w, self.h, self.levels, self.K)
        if self.inputs is not None:
            trk.set_ref(self.dI_ref, *self.inputs)
        else:
            for l, pc in enumerate(self.clouds):
                trk.set_pc(self.dI_ref, l, *pc)
        return trk

    def oracle(self, tries, rmse0, new_img=None):
        trk = self.oracle_tracker()
        dI_new, _ = orc.make_images(self.new_img if new_img is None else new_img, self.levels)

        def track(T0, aff0, min_res):
            orc.lib("f32").orc_set_sum_mode(0)
            return trk.track(dI_new, T0, aff0, (0, 0), self.exposures, self.levels - 1, min_res=min_res)
        return model.track_new_coarse(track, tries, (0, 0), rmse0)


def bits(one, loop, tag=""):
    """the bit contract between the one-call form and the loop over nalo_trk_track"""
    assert scenes.pattern(one) == scenes.pattern(loop), (tag, scenes.pattern(one), scenes.pattern(loop))
    for k in OUT_KEYS:
        assert np.array_equal(one[k], loop[k], equal_nan=True), (tag, k, one[k], loop[k])
    assert np.array_equal(one["lastCoarseRMSE"], loop["achievedRes"], equal_nan=True)
    assert len(one["records"]) == len(loop["records"])
    for i, (a, b) in enumerate(zip(one["records"], loop["records"])):
        for k in ("lastResiduals", "flow", "T", "aff"):
            assert np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1), equal_nan=True), (tag, i, k, a[k], b[k])
        nev, ev, rep = b["extra"]
        assert a["n_evals"] == nev and list(a["evals"]) == list(ev) and a["have_repeated"] == rep, (tag, i, a["n_evals"], nev, list(a["evals"]), list(ev), a["have_repeated"], rep)
    total = np.sum([b["extra"][1] for b in loop["records"]], axis=0)
    assert list(one["last_evals"]) == list(total), (tag, one["last_evals"], total)                # nalo_trk_last_evals: the sum over the tries


def knife_edge(orc_res):
    """does the ORACLE's own run hold a good try whose lastRes[0] lies within 1e-4 (relative: the bound on lastResiduals) of the achievedRes[0] it is compared
    with at :633? Then who is taken is decided inside the tolerance of the numbers compared, and two correct fp32 implementations may differ in it."""
    ach0 = np.nan
    for q in orc_res["records"]:
        lr0 = q["lastResiduals"][0]
        if q["ok"] and np.isfinite(lr0) and np.isfinite(ach0) and abs(lr0 - ach0) <= 1e-4 * ach0:
            return True
        if q["taken"]:
            ach0 = lr0
    return False


def against_oracle(one, orc_res, levels, tag=""):
    """decisions equal; test_tracker_gpu.py's bounds on every good try and on the outputs. On a knife-edge list (above) the take-over among the tied tries is
    not compared: tries run, per-try ok and abort_lvl and have_one_good still are, and the outputs are compared with the oracle's record of the SAME winner."""
    po, pr = scenes.pattern(one), scenes.pattern(orc_res)
    edge = knife_edge(orc_res)
    if edge:
        assert (po[0], po[2], [(a, c) for a, _, c in po[3]]) == (pr[0], pr[2], [(a, c) for a, _, c in pr[3]]), (tag, po, pr)
    else:
        assert po == pr, (tag, po, pr)
    for i, (a, b) in enumerate(zip(one["records"], orc_res["records"])):
        if a["ok"] and np.isfinite(b["lastResiduals"][0]):
            assert pose_dist(a["T"].reshape(3, 4), b["T"]) < 1e-5, (tag, i)
            assert np.allclose(a["lastResiduals"][:levels], b["lastResiduals"][:levels], rtol=1e-4), (tag, i, a["lastResiduals"], b["lastResiduals"])
            assert np.abs(a["aff"] - b["aff"]).max() < 1e-3, (tag, i)
    if one["have_one_good"]:
        w = orc_res["records"][one["winner"]] if edge else orc_res
        assert pose_dist(one["T"], w["T"]) < 1e-5 and np.abs(one["aff"] - w["aff"]).max() < 1e-3, tag
        assert np.allclose(one["achievedRes"][:levels], orc_res["achievedRes"][:levels], rtol=1e-4), (tag, one["achievedRes"], orc_res["achievedRes"])


@functools.lru_cache(maxsize=None)
def rig640():
    s = scenes.scene()
    return Rig(s.win.w, s.win.h, s.win.K, s.ref_img, s.new_img, scenes.EXPOSURES, inputs=s.inputs)


@functools.lru_cache(maxsize=None)
def rig1224():
    win, new = frames(1224, 368)
    r = Rig(win.w, win.h, win.K, win.images[0], new, EXPOSURES_LARGE, inputs=tracker_inputs(win, n=8750, seed=3))
    r.Ttrue = true_rel_pose(win, 0, 1)
    return r


@functools.lru_cache(maxsize=None)
def rig140():
    win = synth.make_window(w=140, h=68, W=1, P=16, seed=11, n_extra=1)
    levels = win.levels
    dI_ref, _ = orc.make_images(win.images[0], levels)
    rng, L, clouds = np.random.RandomState(5), orc.lib(), []
    for l, n in enumerate([512, 384][:levels]):
        wl, hl = win.w >> l, win.h >> l
        uu, vv = np.meshgrid(np.arange(2, wl - 3), np.arange(2, hl - 3))
        uu, vv = uu.ravel(), vv.ravel()
        d = win.depth[0][vv << l, uu << l]
        ok = np.isfinite(d) & (d > 0)
        uu, vv, d = uu[ok], vv[ok], d[ok]
        k = np.sort(rng.choice(len(uu), n, replace=False))
        col = dI_ref[L.orc_pyr_offset(win.w, win.h, l) + vv[k] * wl + uu[k], 0]
        clouds.append(tuple(a.astype(np.float32) for a in (uu[k], vv[k], 1.0 / d[k], col)))
    new = (1.05 * win.images[0] + 3.0 + np.random.RandomState(29).normal(0, 1.0, win.images[0].shape)).astype(np.float32)
    r = Rig(win.w, win.h, win.K, win.images[0], new, [1.0, 1.0], clouds=clouds)
    r.Ttrue = model.se3_exp([0.01, -0.005, 0.02, 0.002, -0.003, 0.001])      # the small motion the hypotheses lie around (the frame pair itself has none)
    return r


def two_lists(r):
    """the two multi-try lists of the larger and the smaller shape: the reference's 31 hypotheses, and [bad, good, the same bad one, a far one]"""
    T09 = orc.se3_exp(orc.se3_log(r.Ttrue) * 0.9)
    bad = model.se3_mul(r.Ttrue, scenes.rot(1, 0.25))
    return {"all31": model.motion_tries(model.se3_inv(T09), scenes.IDENTITY), "affine": np.array([bad, T09, bad, model.se3_exp([0.3, 0, 0, 0, 0, 0])])}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _OPEN:
        c.close()
    _OPEN.clear()
    for f in (rig640, rig1224, rig140):
        f.cache_clear()


# ---- 1, 2: the scenarios at 640x480
@pytest.mark.parametrize("name", scenes.SCENARIOS)
def test_scenarios_at_640x480(name):
    """each scenario: the bit contract, the branch pattern of track_tries_scenes.py in the records, and the oracle's decisions and bounds"""
    s, r = scenes.scene(), rig640()
    kind, tries, rmse0 = s.scenario(name)
    r.upload_new(s.new_frame(kind))
    one, loop = r.one_call(tries, rmse0), r.looped(tries, rmse0)
    cfg = r.ctx.trk_launch_config()
    assert one["driver"] == 1 and cfg["driver"] == 1 and 20 <= cfg["nblocks"] <= 40 and max(cfg["rounds"]) == 1, cfg
    assert scenes.pattern(one) == scenes.expected_pattern(name, r.levels - 1), scenes.pattern(one)
    bits(one, loop, name)
    against_oracle(one, s.oracle(name), r.levels, name)
    if name in ("bright", "nan"):                                 # the none-good defaults (:658-664), and achievedRes still replaces lastCoarseRMSE
        assert np.array_equal(one["T"], tries[0]) and np.array_equal(one["aff"], [0, 0]) and np.array_equal(one["flow"], [0, 0, 0])
        assert np.isnan(one["lastCoarseRMSE"]).all() and one["winner"] == -1
    if name == "affine":                                          # a record's T / aff: written by a try that failed the tail, the input of one that stopped early
        rec = one["records"]
        assert not np.array_equal(rec[0]["T"].reshape(3, 4), tries[0]) and abs(rec[0]["aff"][0]) > 1.2
        assert np.array_equal(rec[2]["T"].reshape(3, 4), tries[2]) and np.array_equal(rec[2]["aff"], [0, 0])
    if name == "repeat":                                          # haveRepeated is per try: set in tries 0 and 1, clear in try 2
        assert [int(q["have_repeated"]) for q in one["records"]] == [1, 1, 0]


# ---- 3, 4: two rounds on 64 workgroups; one workgroup
@pytest.mark.parametrize("which", ["all31", "affine"])
def test_two_rounds_on_64_workgroups_at_1224x368(which):
    r = rig1224()
    tries = two_lists(r)[which]
    one, loop = r.one_call(tries, 1e-6), r.looped(tries, 1e-6)
    cfg = r.ctx.trk_launch_config()
    assert one["driver"] == 1 and cfg["nblocks"] == 64 and cfg["rounds"][:4] == [2, 2, 1, 1], cfg
    assert one["try_iterations"] == len(tries) and one["have_one_good"] == 1
    bits(one, loop, which)
    against_oracle(one, r.oracle(tries, 1e-6), r.levels, which)


@pytest.mark.parametrize("which", ["all31", "affine"])
def test_one_workgroup_at_140x68(which):
    """NB == 1: no exchange, no tags"""
    r = rig140()
    tries = two_lists(r)[which]
    one, loop = r.one_call(tries, 1e-6), r.looped(tries, 1e-6)
    cfg = r.ctx.trk_launch_config()
    assert one["driver"] == 1 and cfg["nblocks"] == 1, cfg
    assert one["try_iterations"] == len(tries) and one["have_one_good"] == 1
    bits(one, loop, which)
    if which == "affine":
        assert scenes.pattern(one) == (4, 1, 1, [(0, 0, -1), (1, 1, -1), (0, 0, 1), (0, 0, 1)])
    against_oracle(one, r.oracle(tries, 1e-6), r.levels, which)


# ---- 5: a list of one
def test_one_try_equals_trk_track_with_nan_thresholds():
    s, r = scenes.scene(), rig640()
    r.upload_new(s.new_img)
    one = r.one_call(s.T09[None], 1e-6)
    ok, T, aff, lr, lf, nev = r.twin.trk_track(1, s.T09, (0, 0), (0, 0), r.exposures, r.levels - 1)          # min_res None: five NaNs
    q = one["records"][0]
    assert one["try_iterations"] == 1 and q["ok"] == ok == 1 and q["taken"] == 1 and one["winner"] == 0 and q["n_evals"] == nev
    for got, want in ((q["T"].reshape(3, 4), T), (q["aff"], aff), (q["lastResiduals"], lr), (q["flow"], lf), (one["T"], T), (one["aff"], aff), (one["flow"], lf),
                      (one["achievedRes"], lr)):
        assert np.array_equal(got, want, equal_nan=True)
    assert list(one["last_evals"]) == list(r.twin.trk_last_evals()[0])


# ---- 6: the library's own hypothesis list
def test_list_from_motion_tries():
    s, r = scenes.scene(), rig640()
    r.upload_new(s.new_img)
    tries = binding.trk_motion_tries(model.se3_inv(s.T09), scenes.IDENTITY)
    assert tries.shape == (31, 3, 4)
    one, loop = r.one_call(tries, 1e-6), r.looped(tries, 1e-6)
    assert one["try_iterations"] == 31 and one["winner"] == 0
    bits(one, loop, "motion_tries")


# ---- 7: no side effects on nalo_trk_track
def test_two_full_calls_then_trk_track_has_the_bits_of_a_twin_that_never_called():
    """two 31-try calls reserve 62 launch numbers and leave their tags in the partials buffer; the nalo_trk_track after them must not notice"""
    s, r = scenes.scene(), rig640()
    c, fresh = r.context(), r.context()
    a = r.one_call(s.list31, 1e-6, c=c)
    b = r.one_call(s.list31, 1e-6, c=c)
    assert a["try_iterations"] == b["try_iterations"] == 31
    got = c.trk_track(1, s.T09, (0, 0), (0, 0), r.exposures, r.levels - 1)
    want = fresh.trk_track(1, s.T09, (0, 0), (0, 0), r.exposures, r.levels - 1)
    assert got[0] == want[0] == 1 and got[5] == want[5]
    for x, y in zip(got[1:5], want[1:5]):
        assert np.array_equal(x, y, equal_nan=True)
    assert list(c.trk_last_evals()[0]) == list(fresh.trk_last_evals()[0]) and c.trk_launch_config() == fresh.trk_launch_config()


# ---- 9: drivers
def test_fixed_affine_parameter_runs_host_driven():
    """affine_opt_mode_a = -1: the persistent kernel does not solve that system, the list runs through the host-driven loop (driver 2) and equals the loop on a
    twin with the same setting - including the zeroing of the fixed parameter (:1255)"""
    s, r = scenes.scene(), rig640()
    c, twin = r.context(), r.context()
    for x in (c, twin):
        x.set_settings(affine_opt_mode_a=-1)
    tries = s.scenario("affine")[1]
    one, loop = r.one_call(tries, 1e-6, c=c), r.looped(tries, 1e-6, c=twin)
    assert one["driver"] == 2 and c.trk_launch_config()["driver"] == 2
    bits(one, loop, "fixed a")
    assert one["have_one_good"] == 1 and one["aff"][0] == 0.0


def test_lost_workgroup_redoes_the_list_from_the_host(capfd):
    """after nalo_test_inject the launch is reported lost: the WHOLE list is redone by the host-driven loop, the message appears once, the context stays latched
    (the next call goes to the host loop straight away, silently). Same decisions as the persistent launch, test_tracker_gpu.py's bounds on the numbers."""
    s, r = scenes.scene(), rig640()
    r.upload_new(s.new_img)
    tries = s.scenario("affine")[1]
    want = r.one_call(tries, 1e-6)
    assert want["driver"] == 1
    c = r.context()
    c.test_inject(binding.INJECT_LM_LOST_BLOCK)
    capfd.readouterr()
    msg = "drives the tracker's LM loop from the host"
    errs = []
    for _ in range(2):
        got = r.one_call(tries, 1e-6, c=c)
        errs.append(capfd.readouterr().err)
        assert got["driver"] == 2 and c.trk_launch_config()["driver"] == 2
        assert scenes.pattern(got) == scenes.pattern(want)
        assert pose_dist(got["T"], want["T"]) < 1e-5 and np.abs(got["aff"] - want["aff"]).max() < 1e-3
        assert np.allclose(got["achievedRes"][:r.levels], want["achievedRes"][:r.levels], rtol=1e-4)
        for a, b in zip(got["records"], want["records"]):
            fin = np.isfinite(b["lastResiduals"])
            assert np.array_equal(fin, np.isfinite(a["lastResiduals"]))
            if b["ok"]:
                assert np.allclose(a["lastResiduals"][fin], b["lastResiduals"][fin], rtol=1e-4)
    assert errs[0].count(msg) == 1 and msg not in errs[1]
    ok = c.trk_track(1, s.T09, (0, 0), (0, 0), r.exposures, r.levels - 1)[0]       # nalo_trk_track of the same context: latched too
    assert ok == 1 and c.trk_launch_config()["driver"] == 2 and msg not in capfd.readouterr().err


# ---- 10: refusals
def sentinel_args(r, tries):
    t = np.ascontiguousarray(tries, np.float64).reshape(-1, 12)
    a = binding.TrkTriesArgs()
    a.slot_new, a.n_tries, a.coarsestLvl = 1, len(t), r.levels - 1
    a.tries = t.ctypes.data_as(C.POINTER(C.c_double))
    a.exposures[:] = r.exposures
    a.lastCoarseRMSE_io[:] = [7.0] * 5
    for f in ("T", "aff", "flow", "achievedRes"):
        getattr(a, f)[:] = [-77.0] * len(getattr(a, f))
    a.have_one_good = a.try_iterations = a.winner = a.driver = -77
    a._keep = t
    return a


def outputs(a):
    return (list(a.T), list(a.aff), list(a.flow), list(a.achievedRes), list(a.lastCoarseRMSE_io), a.have_one_good, a.try_iterations, a.winner, a.driver)


def test_refusals_leave_everything_untouched():
    s, r = scenes.scene(), rig640()
    r.upload_new(s.new_img)
    c = r.context()
    good = s.scenario("affine")[1]
    nonfinite = good.copy(); nonfinite[2, 1, 3] = np.inf
    nan_entry = good.copy(); nan_entry[0, 0, 0] = np.nan
    empty = binding.Context(r.w, r.h, r.K, n_slots=2); _OPEN.append(empty)       # no reference at all
    cases = [
        ("n_tries 0", lambda a: setattr(a, "n_tries", 0), good, c, "-1"),
        ("n_tries 65", lambda a: setattr(a, "n_tries", binding.TRK_MAX_TRIES + 1), good, c, "-1"),
        ("inf in tries", lambda a: None, nonfinite, c, "-1"),
        ("nan in tries", lambda a: None, nan_entry, c, "-1"),
        ("null tries", lambda a: setattr(a, "tries", C.POINTER(C.c_double)()), good, c, "-1"),
        ("coarsestLvl", lambda a: setattr(a, "coarsestLvl", r.levels), good, c, "-1"),
        ("coarsestLvl < 0", lambda a: setattr(a, "coarsestLvl", -1), good, c, "-1"),
        ("slot", lambda a: setattr(a, "slot_new", 2), good, c, "-1"),
        ("records_cap < 0", lambda a: setattr(a, "records_cap", -1), good, c, "-1"),
        ("no reference", lambda a: None, good, empty, "-4"),
    ]
    for tag, spoil, tries, ctx, code in cases:
        a = sentinel_args(r, tries)
        spoil(a)
        before = outputs(a)
        ev_before, cfg_before = list(ctx.trk_last_evals()[0]), ctx.trk_launch_config()
        with pytest.raises(binding.NaloError, match="nalo error %s" % code):
            ctx.trk_track_tries(1, None, None, None, None, None, None, records=False, args=a)
        assert outputs(a) == before, tag
        assert list(ctx.trk_last_evals()[0]) == ev_before and ctx.trk_launch_config() == cfg_before, tag
    # the next legal call on the same context is correct: the bits of the shared context's
    want = r.one_call(good, 1e-6)
    got = r.one_call(good, 1e-6, c=c)
    assert got["driver"] == 1 and scenes.pattern(got) == scenes.pattern(want)
    for k in OUT_KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True)
    assert got["records"].tobytes() == want["records"].tobytes()
    # a records array shorter than the tries run: the first records_cap entries, the outputs unchanged
    a = sentinel_args(r, good)
    rec = np.zeros(2, binding.TRY_RECORD_DTYPE)
    a.records, a.records_cap = rec.ctypes.data_as(C.POINTER(binding.TrkTryRecord)), 2
    a.lastCoarseRMSE_io[:] = [1e-6] * 5
    c._ck(c.L.nalo_trk_track_tries(c.h_, C.byref(a)))
    assert a.try_iterations == 4 and rec.tobytes() == want["records"][:2].tobytes()


# ---- 11: determinism
def test_same_call_twice_gives_equal_bytes():
    s, r = scenes.scene(), rig640()
    r.upload_new(s.new_img)
    a, b = r.one_call(s.list31, 1e-6), r.one_call(s.list31, 1e-6)
    assert a["records"].tobytes() == b["records"].tobytes() and len(a["records"]) == 31
    for k in OUT_KEYS + ("lastCoarseRMSE",):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert (a["have_one_good"], a["try_iterations"], a["winner"], a["driver"]) == (b["have_one_good"], b["try_iterations"], b["winner"], b["driver"])
