"""trackNewCoarse's hypothesis loop without a device: the numpy model (track_tries_model.py) on scripted trackers, worked by hand; nalo_trk_motion_tries
(host code of the library) against the model's builder; and the scenarios of test_track_tries_gpu.py run through the model over the fp32 oracle, where the
branch pattern each of them must reach is asserted - so the GPU file never asserts a pattern the reference arithmetic does not produce."""
import numpy as np
import pytest

import track_tries_model as model
import track_tries_scenes as scenes
from nalo_slam_amd import binding

NAN = float("nan")
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def scripted(script):
    """a tracker that answers try i with script[i] = (ok, lastRes[5]) (flow = i + 1, T = its input shifted by i + 1 in x, aff = (i, -i)) and logs the bounds it got"""
    log = []

    def track(T0, aff0, min_res):
        i = len(log)
        log.append(min_res.copy())
        ok, lr = script[i]
        T = T0.copy()
        T[0, 3] += i + 1
        return ok, T, np.array([i, -i], float), np.array(lr, float), np.full(3, i + 1.0)
    return track, log


def tries(n):
    out = np.repeat(I34[None], n, 0).copy()
    out[:, 1, 3] = np.arange(n) * 10.0                           # a tag that tells the tries apart
    return out


def test_nan_residual_with_ok_is_not_taken_and_defaults_hold():
    """lastRes[0] NaN with ok true fails :633's isfinite; with no good try the outputs are tries[0], aff_init, flow 0 and achievedRes stays NaN"""
    track, log = scripted([(1, [NAN] * 5), (1, [NAN, 3, 3, 3, NAN])])
    r = model.track_new_coarse(track, tries(2), (0.5, -2.0), 100.0)
    assert scenes.pattern(r) == (2, -1, 0, [(1, 0, -1), (1, 0, -1)])
    assert np.array_equal(r["T"], tries(2)[0]) and np.array_equal(r["aff"], [0.5, -2.0]) and np.array_equal(r["flow"], [0, 0, 0])
    assert np.isnan(r["achievedRes"]).all() and all(np.isnan(b).all() for b in log)


def test_first_good_try_is_taken_through_not_ge_nan():
    """!(a >= NaN) is true: the first good try wins; a failed try before it neither wins nor touches achievedRes"""
    track, log = scripted([(0, [9, 9, 9, 9, NAN]), (1, [5, 6, 7, 8, NAN])])
    r = model.track_new_coarse(track, tries(2), (0, 0), 1e-6)
    assert scenes.pattern(r) == (2, 1, 1, [(0, 0, -1), (1, 1, -1)])
    assert np.isnan(log[1]).all()                                # try 0 was not good: try 1 still got NaN bounds
    assert np.array_equal(r["achievedRes"][:4], [5, 6, 7, 8]) and np.isnan(r["achievedRes"][4])
    assert r["T"][0, 3] == 2 and r["T"][1, 3] == 10 and np.array_equal(r["aff"], [1, -1]) and np.array_equal(r["flow"], [2, 2, 2])


def test_good_but_not_better_try_still_lowers_a_coarser_level_and_nan_never_overwrites():
    """try 1 is good with lastRes[0] == achievedRes[0] (>= : not taken) yet lowers level 2; its NaN at level 3 does not overwrite a finite bound; try 2 is
    not ok and stopped at level 2 (7 > 1.5 x 4), and its level-3 residual still lowers that level (:643-650 run for every try)"""
    track, log = scripted([(1, [5, 6, 7, 8, NAN]), (1, [5, 6.5, 4, NAN, NAN]), (0, [NAN, NAN, 7, 2, NAN])])
    r = model.track_new_coarse(track, tries(3), (0, 0), 1e-6)
    assert scenes.pattern(r) == (3, 0, 1, [(1, 1, -1), (1, 0, -1), (0, 0, 2)])
    assert np.array_equal(log[1][:4], [5, 6, 7, 8]) and np.array_equal(log[2][:4], [5, 6, 4, 8])
    assert np.array_equal(r["achievedRes"][:4], [5, 6, 4, 2]) and np.isnan(r["achievedRes"][4])
    assert r["T"][0, 3] == 1 and np.array_equal(r["flow"], [1, 1, 1])                # the winner's outputs stay


def test_later_better_try_takes_over():
    track, _ = scripted([(1, [5, 6, 7, 8, NAN]), (1, [4, 7, 7, 9, NAN])])
    r = model.track_new_coarse(track, tries(2), (0, 0), 1e-6)
    assert scenes.pattern(r) == (2, 1, 1, [(1, 1, -1), (1, 1, -1)])
    assert np.array_equal(r["achievedRes"][:4], [4, 6, 7, 8]) and r["T"][1, 3] == 10


def test_early_out_is_strict():
    """achievedRes[0] < lastCoarseRMSE[0] * 1.5: 3.0 against 2.0 * 1.5 goes on, against 2.0000001 * 1.5 it ends; a NaN lastCoarseRMSE never ends it"""
    for rmse0, run in ((2.0, 2), (2.0000001, 1), (NAN, 2)):
        track, _ = scripted([(1, [3, 3, 3, 3, NAN]), (0, [NAN, NAN, NAN, 9, NAN])])
        assert model.track_new_coarse(track, tries(2), (0, 0), rmse0)["try_iterations"] == run


def test_float_cast_of_isfinite():
    """isfinite((float)x): a residual beyond FLT_MAX is not taken"""
    track, _ = scripted([(1, [1e39, 1, 1, 1, NAN])])
    assert scenes.pattern(model.track_new_coarse(track, tries(1), (0, 0), 1e-6)) == (1, -1, 0, [(1, 0, -1)])


# ---- nalo_trk_motion_tries against the builder
def poses():
    a = model.se3_exp([0.02, -0.01, 0.11, 0.004, -0.013, 0.002])
    b = model.se3_exp([-0.3, 0.05, 0.8, -0.02, 0.03, 0.01])
    return a, b


def test_motion_tries_count_order_and_values():
    a, b = poses()
    got, want = binding.trk_motion_tries(a, b), model.motion_tries(a, b)
    assert got.shape == want.shape == (31, 3, 4)
    inv = model.se3_inv(a)
    assert np.abs(got[0] - model.se3_mul(inv, b)).max() < 1e-15                      # constant motion first
    assert np.abs(got[1] - model.se3_mul(model.se3_mul(inv, inv), b)).max() < 4e-15   # double
    assert np.abs(model.se3_mul(model.se3_mul(got[2], model.se3_inv(b)), model.se3_mul(got[2], model.se3_inv(b))) - inv).max() < 1e-14   # half: its square is the whole
    assert np.array_equal(got[3], b) and np.array_equal(got[4], I34)                # zero motion, identity
    assert np.abs(got - want).max() < 1e-13, np.abs(got - want).reshape(31, -1).max(1)
    # the order of the 26 rotation variants: each equals constant * R(q) for ITS sign pattern and no other
    for k, s in enumerate(model.ROT_SIGNS):
        rel = model.se3_mul(model.se3_inv(got[0]), got[5 + k])
        axis = np.array([rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1]])
        assert np.array_equal(np.sign(np.round(axis, 6)), s), (k, s, axis)
        assert np.abs(rel[:, 3]).max() < 1e-15


def test_motion_tries_rotation_blocks():
    """every rotation block orthonormal and equal to constant * R(normalised quaternion) to a few ulp (entries <= 1: 8 eps absolute)"""
    a, b = poses()
    got = binding.trk_motion_tries(a, b)
    eps = np.finfo(np.float64).eps
    for k, s in enumerate(model.ROT_SIGNS):
        R = got[5 + k][:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 8 * eps and abs(np.linalg.det(R) - 1) < 8 * eps
        want = got[0][:, :3] @ model.quat_rotation(1.0, *(np.array(s) * model.ROT_DELTA))
        assert np.abs(R - want).max() <= 8 * eps, (k, np.abs(R - want).max())
    q = model.quat_rotation(1.0, model.ROT_DELTA, 0, 0)
    assert abs(np.arctan2(q[2, 1], q[1, 1]) - 2 * np.arctan(model.ROT_DELTA)) < 4 * eps     # the quaternion (1, d, 0, 0) NORMALISED: an angle of 2 atan(d), not 2 d


def test_motion_tries_without_valid_poses():
    a, b = poses()
    got = binding.trk_motion_tries(a, b, poses_valid=False)
    assert got.shape == (1, 3, 4) and np.array_equal(got[0], I34)
    assert np.array_equal(model.motion_tries(a, b, poses_valid=False), got)


# ---- the GPU file's scenarios on the fp32 oracle
@pytest.mark.parametrize("name", scenes.SCENARIOS)
def test_scenario_reaches_its_branches_on_the_oracle(name):
    s = scenes.scene()
    r = s.oracle(name)
    top = s.levels - 1
    assert scenes.pattern(r) == scenes.expected_pattern(name, top), scenes.pattern(r)
    recs = r["records"]
    if name == "affine":                                         # try 0 ran every level: finite residuals, the pose written, and the tail said no
        assert np.isfinite(recs[0]["lastResiduals"][:top + 1]).all() and not np.array_equal(recs[0]["T"], s.scenario(name)[1][0])
    if name == "bright":
        assert all(np.isfinite(q["lastResiduals"][:top + 1]).all() for q in recs) and np.isnan(r["achievedRes"]).all()
    if name == "nan":
        assert all(np.isnan(q["lastResiduals"]).all() for q in recs)
    if name == "all31":                                          # none of the 30 losers stops at the coarsest level
        assert all(np.isfinite(q["lastResiduals"][top]) and q["abort_lvl"] < top for q in recs[1:])
    if name == "coarsest":
        assert recs[1]["lastResiduals"][top] < recs[0]["lastResiduals"][top] and r["achievedRes"][top] == recs[1]["lastResiduals"][top]
        assert recs[2]["lastResiduals"][top] > 1.5 * r["achievedRes"][top] and np.isnan(recs[2]["lastResiduals"][:top]).all()
    if name == "takeover":
        assert recs[1]["lastResiduals"][0] < 0.9 * recs[0]["lastResiduals"][0]       # a clear margin: no fp32 / fp64 difference flips it
        assert np.array_equal(r["T"], recs[1]["T"])
    if name == "repeat":
        assert [q["extra"][1] for q in recs] == [1, 1, 0]
