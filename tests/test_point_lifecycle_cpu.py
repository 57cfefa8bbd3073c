"""The point-lifecycle model (tests/lifecycle_model.py) on hand-built points, one per clause and boundary of PointHessian::isOOB / isInlierNew and
FullSystem::flagPointsForRemoval, the two index manipulations the caller and the library apply to lastResiduals, and the declarations of the four entry points.
Needs no device. CASES is also what tests/test_point_lifecycle_gpu.py plants into a real window."""
import os
import re

import numpy as np

import lifecycle_model as lm
from lifecycle_model import IN, OOB, OUTLIER, KEEP, DROP_NORES, DROP, MARGINALIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = -1      # no residual

# One point of a W = 8 window per row, hosted by frame `host`: res = state of its residual per target, idepth, H = idepth_hessian, flagged = the frames with
# flaggedForMarginalization, numGood, lastResiduals[k].second, and the decision the reference takes with the clause of isOOB that fires (0 = isOOB false).
CASES = [
    #     name                         host res                                   idepth H      flagged numGood last_state       decision     clause
    dict(name="keep",                  host=0, res=[N, IN, IN, IN, IN, N, N, N],  idepth=.1, H=900., flagged=[], ng=20, ls=(IN, IN),           dec=KEEP,        clause=0),
    dict(name="negative_idepth",       host=0, res=[N, IN, IN, IN, IN, N, N, N],  idepth=-.1, H=900., flagged=[], ng=20, ls=(IN, IN),          dec=DROP_NORES,  clause=-1),
    dict(name="no_residuals",          host=0, res=[N] * 8,                       idepth=.1, H=0.,   flagged=[], ng=20, ls=(OOB, OOB),         dec=DROP_NORES,  clause=-1),
    dict(name="last_oob_marg",         host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=900., flagged=[], ng=20, ls=(OOB, IN),          dec=MARGINALIZE, clause=2),
    dict(name="last_oob_H_is_50",      host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=50.,  flagged=[], ng=20, ls=(OOB, IN),          dec=DROP,        clause=2),
    dict(name="last_oob_H_above_50",   host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=float(np.nextafter(np.float32(50), np.float32(51))), flagged=[], ng=20, ls=(OOB, IN), dec=MARGINALIZE, clause=2),
    dict(name="last_oob_not_inlier_3", host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=900., flagged=[], ng=3,  ls=(OOB, IN),          dec=DROP,        clause=2),
    dict(name="last_oob_inlier_4",     host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=900., flagged=[], ng=4,  ls=(OOB, IN),          dec=MARGINALIZE, clause=2),
    dict(name="last_oob_two_res",      host=0, res=[N, IN, IN, N, N, N, N, N],    idepth=.1, H=900., flagged=[], ng=20, ls=(OOB, IN),          dec=DROP,        clause=2),
    dict(name="two_outliers_nres_2",   host=0, res=[N, IN, IN, N, N, N, N, N],    idepth=.1, H=900., flagged=[], ng=20, ls=(OUTLIER, OUTLIER), dec=DROP,        clause=4),
    dict(name="two_outliers_nres_1",   host=0, res=[N, IN, N, N, N, N, N, N],     idepth=.1, H=900., flagged=[], ng=20, ls=(OUTLIER, OUTLIER), dec=KEEP,        clause=3),
    dict(name="two_outliers_nres_3",   host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=900., flagged=[], ng=20, ls=(OUTLIER, OUTLIER), dec=MARGINALIZE, clause=4),
    dict(name="one_outlier",           host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=900., flagged=[], ng=20, ls=(OUTLIER, IN),      dec=KEEP,        clause=0),
    dict(name="outlier_then_oob",      host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=900., flagged=[], ng=20, ls=(OUTLIER, OOB),     dec=KEEP,        clause=0),
    dict(name="vis_leaves_2_ng_15",    host=0, res=[N, IN, IN, IN, IN, N, N, N],  idepth=.1, H=900., flagged=[1, 2], ng=15, ls=(IN, IN),       dec=MARGINALIZE, clause=1),
    dict(name="vis_leaves_2_ng_14",    host=0, res=[N, IN, IN, IN, IN, N, N, N],  idepth=.1, H=900., flagged=[1, 2], ng=14, ls=(IN, IN),       dec=KEEP,        clause=0),
    dict(name="vis_leaves_3_ng_15",    host=0, res=[N, IN, IN, IN, IN, N, N, N],  idepth=.1, H=900., flagged=[1], ng=15, ls=(IN, IN),          dec=KEEP,        clause=0),
    dict(name="vis_counts_IN_only",    host=0, res=[N, OUTLIER, IN, IN, N, N, N, N], idepth=.1, H=900., flagged=[1], ng=15, ls=(IN, IN),       dec=KEEP,        clause=0),
    dict(name="vis_counts_IN_only_b",  host=0, res=[N, IN, IN, IN, N, N, N, N],   idepth=.1, H=900., flagged=[1], ng=15, ls=(IN, IN),          dec=MARGINALIZE, clause=1),
    dict(name="vis_two_res_only",      host=0, res=[N, IN, IN, N, N, N, N, N],    idepth=.1, H=900., flagged=[1, 2], ng=15, ls=(IN, IN),       dec=KEEP,        clause=0),
    dict(name="flagged_host_marg",     host=3, res=[IN, IN, IN, N, IN, N, N, N],  idepth=.1, H=900., flagged=[3], ng=20, ls=(IN, IN),          dec=MARGINALIZE, clause=0),
    dict(name="flagged_host_low_H",    host=3, res=[IN, IN, IN, N, IN, N, N, N],  idepth=.1, H=10.,  flagged=[3], ng=20, ls=(IN, IN),          dec=DROP,        clause=0),
    dict(name="flagged_host_two_res",  host=3, res=[IN, IN, N, N, N, N, N, N],    idepth=.1, H=900., flagged=[3], ng=20, ls=(IN, IN),          dec=DROP,        clause=0),
    dict(name="flagged_host_ng_3",     host=3, res=[IN, IN, IN, N, IN, N, N, N],  idepth=.1, H=900., flagged=[3], ng=3, ls=(IN, IN),           dec=DROP,        clause=0),
    dict(name="flagged_host_no_res",   host=3, res=[N] * 8,                       idepth=.1, H=0.,   flagged=[3], ng=20, ls=(IN, IN),          dec=DROP_NORES,  clause=-1),
]


def test_every_case_takes_the_reference_decision():
    for c in CASES:
        dec, clause = lm.flag_point(c["res"], c["idepth"], c["H"], c["host"] in c["flagged"], c["flagged"], c["ng"], c["ls"])
        assert (dec, clause) == (c["dec"], c["clause"]), (c["name"], dec, clause)
    # every decision and every clause of isOOB is reached by some case
    assert {c["dec"] for c in CASES} == {KEEP, DROP_NORES, DROP, MARGINALIZE}
    assert {c["clause"] for c in CASES} == {-1, 0, 1, 2, 3, 4}


def test_flag_points_counts_per_host_are_the_decisions():
    W = 8
    for flagged in ([], [3], [1, 2], [1]):
        cs = [c for c in CASES if c["flagged"] == flagged]
        ff = np.array([i in flagged for i in range(W)], np.uint8)
        dec, counts, clause, reached = lm.flag_points(np.array([c["host"] for c in cs]), np.array([c["res"] for c in cs], np.int8), np.array([c["idepth"] for c in cs], np.float32),
                                                      np.array([c["H"] for c in cs], np.float32), ff, [c["ng"] for c in cs], [c["ls"] for c in cs])
        assert dec.tolist() == [c["dec"] for c in cs] and clause.tolist() == [c["clause"] for c in cs]
        assert counts.sum() == len(cs)
        for h in range(W):
            assert counts[h].tolist() == [sum(1 for c in cs if c["host"] == h and c["dec"] == k) for k in range(4)]
        # the test on H is reached exactly by the points that end MARGINALIZE or are dropped FOR their H
        for c, r in zip(cs, reached):
            n = sum(1 for s in c["res"] if s >= 0)
            assert bool(r) == (c["dec"] == MARGINALIZE or (c["dec"] == DROP and n >= 3 and c["ng"] >= 4)), c["name"]


def test_idepth_hessian_is_the_float_sum_with_the_floor():
    Hdd = np.array([49.999996, 50.0, 0.0, -1.0, 3.0, 1e-12], np.float32)
    HdiF = np.array([0.02, 0.02, 1e10, 1e10, 0.0, 1e10], np.float32)
    prior = np.array([0, 0, 0, 0, 1, 0])
    H = lm.idepth_hessian(Hdd, HdiF, prior)
    assert H.dtype == np.float32
    assert H.tolist() == [float(np.float32(49.999996)), 50.0, float(np.float32(1e-10)), float(np.float32(1e-10)), 0.0, float(np.float32(1e-10))]
    assert lm.idepth_hessian(np.float32([3.0]), np.float32([1.0]), [1])[0] == np.float32(2503.0)
    # 1 / HdiF is not that float: the two roundings do not undo each other, so the value returned for a bitwise check has to be H itself
    Hs = np.float32(50) + np.arange(-2000, 2000).astype(np.float32) * np.spacing(np.float32(50))
    back = (np.float32(1) / (np.float64(1.0) / Hs.astype(np.float64)).astype(np.float32)).astype(np.float32)
    assert (back != Hs).any()


def test_swap_at_insertion():
    lt = np.array([[6, 5], [-1, 5], [6, -1], [3, 3]], np.int8)
    ls = np.array([[IN, OUTLIER], [OOB, IN], [OUTLIER, OOB], [IN, IN]], np.int8)
    lt2, ls2 = lm.shift_at_insertion(lt, ls, [True, True, False, True], 7)
    assert lt2.tolist() == [[7, 6], [7, -1], [6, -1], [7, 3]]
    assert ls2.tolist() == [[IN, IN], [IN, OOB], [OUTLIER, OOB], [IN, IN]]
    assert lt.tolist() == [[6, 5], [-1, 5], [6, -1], [3, 3]]          # the inputs are not modified


def test_frame_remap():
    lt = np.array([[7, 6], [2, 1], [3, 7], [-1, 2], [0, 3]], np.int8)
    assert lm.remap_at_frame_marginalization(lt, 2).tolist() == [[6, 5], [-1, 1], [2, 6], [-1, -1], [0, 2]]
    assert lm.remap_at_frame_marginalization(lt, 0).tolist() == [[6, 5], [1, 0], [2, 6], [-1, 1], [-1, 2]]
    assert lm.remap_at_frame_marginalization(lt, 7).tolist() == [[-1, 6], [2, 1], [3, -1], [-1, 2], [0, 3]]


def test_default_history_is_optimize_immature_points():
    ex = np.array([[1, 1, 1, 0], [1, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 0]], np.uint8)
    ng, lt, ls = lm.default_history(ex)
    assert ng.tolist() == [0, 0, 0, 0]
    assert lt.tolist() == [[-1, 2], [3, -1], [-1, 2], [-1, -1]]
    assert ls.tolist() == [[OOB, IN], [IN, OOB], [OOB, IN], [OOB, OOB]]


def test_history_update_on_a_hand_built_pass():
    # point 0: both pointers live, [0]'s residual survives IN, [1]'s is removed as OUTLIER; point 1: [0] names a slot that did not take part; point 2: both pointers
    # name the same residual, which is removed as OOB ([0] takes the state, both pointers go); point 3: no pointer
    st_pre = np.array([[N, IN, IN, IN], [N, IN, IN, N], [IN, N, IN, OOB], [IN, IN, N, IN]], np.int8)
    st_post = np.array([[N, IN, N, IN], [N, IN, IN, N], [IN, N, IN, N], [N, N, N, IN]], np.int8)
    act = st_post == IN
    removed = np.array([[N, N, OUTLIER, N], [N, N, N, N], [N, N, N, OOB], [OUTLIER, OOB, N, N]], np.int8)
    ng, lt, ls = lm.history_update([0, 5, 14, 100000], [[3, 2], [3, 2], [3, 3], [-1, -1]], [[OUTLIER, IN], [OUTLIER, OUTLIER], [IN, IN], [OOB, OUTLIER]], st_pre, st_post, act, removed)
    assert ng.tolist() == [2, 7, 16, 100001]
    assert lt.tolist() == [[3, -1], [3, 2], [-1, -1], [-1, -1]]
    assert ls.tolist() == [[IN, OUTLIER], [OUTLIER, IN], [OOB, IN], [OOB, OUTLIER]]
    st_nofix = np.array([[N, IN, OUTLIER, IN], [N, IN, IN, N], [IN, N, IN, OOB], [IN, OOB, N, IN]], np.int8)
    assert np.array_equal(lm.removed_states(st_nofix, st_pre, st_post), removed)


def test_header_and_binding_declare_the_entry_points():
    names = ["nalo_ba_set_point_history", "nalo_ba_get_point_history", "nalo_ba_flag_points", "nalo_ba_marginalize_flagged"]
    with open(os.path.join(ROOT, "include", "nalo_gpu.h")) as f:
        hdr = f.read()
    from nalo_slam_amd import binding
    for n in names:
        assert re.search(r"^int %s\(nalo_ctx\* ctx" % n, hdr, re.M), n
        assert n in binding.EXPORTS
    for m in ("ba_set_point_history", "ba_get_point_history", "ba_flag_points", "ba_marginalize_flagged"):
        assert callable(getattr(binding.Context, m))
    consts = binding.constants()
    assert consts["setting_minGoodActiveResForMarg"] == lm.MIN_GOOD_ACTIVE_RES_FOR_MARG and consts["setting_minGoodResForMarg"] == lm.MIN_GOOD_RES_FOR_MARG
    assert consts["setting_minIdepthH_marg"] == float(lm.MIN_IDEPTH_H_MARG)


def _oracle_route(name, every=1):
    import orc
    import lifecycle_scenes as sc
    win, st6, has_prior = sc.make_scene(name, every)
    ba = orc.BA(win.W, len(win.host), win.w, win.h, win.K, "f32")
    for i in range(win.W):
        dI, _ = orc.make_images(win.images[i], 1, "f32")
        ba.set_frame(i, dI, win.world_to_cam[i], state6=st6[i])
    ba.set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights, has_prior=has_prior)
    ba.set_residuals(win.exists)
    ba.prepare()
    ba.linearize_all(False)
    ba.apply_res()
    st1 = ba.slots()[0]
    ba.linearize_all(True)
    st2, ac2 = ba.slots()[:2]
    ba.accumulate(0)
    ba.accumulate_sc(True)
    pts = ba.points()
    planted = sc.plant_history(len(win.host), win.W)
    return sc.model_route(win, has_prior, planted, st1, st2, ac2, pts)


def test_scenes_reach_every_class_clause_and_both_sides_of_H_with_the_fp32_oracle_alone():
    """the coverage the GPU test asserts does not hang on the device's numbers: the reference arithmetic (fp32 oracle) alone meets it on the same scenes
    (the 250 k-point window is checked on one point in 25: a point's decision depends on the other points only through the newest frame's energy threshold, a
    quantile the thinning keeps, so the full scene reaches 25 times what the thinned one does; its full oracle pass takes minutes)"""
    import lifecycle_scenes as sc
    for name in ("kitti", "w12", "w16"):
        sc.assert_coverage(name, _oracle_route(name))
    sc.assert_coverage("stress250k", _oracle_route("stress250k", 25), 25)
