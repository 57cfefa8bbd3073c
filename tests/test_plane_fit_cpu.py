"""tests/plane_model.py on hand-built inputs: the semantics nalo_trk_fit_planes / nalo_dense_fit_planes are held to (tests/test_plane_fit_gpu.py), worked out
by hand from DenseMapping::makeMaskDistMap (FullSystem/MapPoint.cpp:445-513) and the fit the header defines. No device."""
import numpy as np
import pytest

import plane_cases as pc
import plane_model as pm

F = np.float32
K = (100.0, 100.0, 32.0, 24.0)


def stripes(w, h, values):
    """a mask of len(values) vertical stripes of equal width"""
    m = np.zeros((h, w), F)
    sw = w // len(values)
    for k, val in enumerate(values):
        m[:, k * sw:(k + 1) * sw if k + 1 < len(values) else w] = val
    return m


def pts_in_stripes(w, h, n_stripes, which, y0=10):
    """one point per entry of `which`, in the stripe it names, at distinct pixels"""
    sw = w // n_stripes
    seen = {}
    u, v = [], []
    for s in which:
        k = seen.get(s, 0)
        seen[s] = k + 1
        u.append(s * sw + 4 + k % (sw - 8))
        v.append(y0 + k // (sw - 8))
    return np.array(u, F), np.array(v, F)


def test_alternating_order_on_five_values():
    w, h = 100, 40
    mask = stripes(w, h, [10, 20, 30, 40, 50])
    # input order by stripe:      0  1  2  3  4  5  6  7  8  9
    which = [1, 0, 2, 0, 3, 1, 4, 2, 2, 3]
    u, v = pts_in_stripes(w, h, 5, which)
    cl = pm.cluster(u, v, np.ones(10, F), mask, w, h)
    # sweep 1 starts at the back (point 9, value 40): members in descending index; what is left is then walked from its front (point 0, value 20): ascending;
    # then from the back again (point 8, value 30): descending; then the front (point 1, value 10): ascending; last value 50.
    # discovery: 40 {9, 4}, 20 {0, 5}, 30 {8, 7, 2}, 10 {1, 3}, 50 {6}. By size, ties in discovery order: 30, 40, 20, 10, 50
    assert [float(c["mask_value"]) for c in cl] == [30, 40, 20, 10, 50]
    assert [list(c["members"]) for c in cl] == [[8, 7, 2], [9, 4], [0, 5], [1, 3], [6]]


def test_size_tie_keeps_discovery_order():
    w, h = 100, 40
    mask = stripes(w, h, [1, 2, 3, 4])
    which = [0, 1, 2, 3, 0, 1, 2, 3]
    u, v = pts_in_stripes(w, h, 4, which)
    cl = pm.cluster(u, v, np.ones(8, F), mask, w, h)
    # discovery: back -> 4 {7, 3}; front -> 1 {0, 4}; back -> 3 {6, 2}; front -> 2 {1, 5}; all of size two
    assert [float(c["mask_value"]) for c in cl] == [4, 1, 3, 2]
    assert [list(c["members"]) for c in cl] == [[7, 3], [0, 4], [6, 2], [1, 5]]


def test_xx_never_rounds_up():
    w, h = 64, 48
    mask = np.zeros((h, w), F)
    mask[:, 10] = 5
    mask[:, 11] = 6
    u = np.array([10.9, 10.2], F)
    v = np.array([20.7, 20.1], F)
    cl = pm.cluster(u, v, np.ones(2, F), mask, w, h)
    assert len(cl) == 1 and float(cl[0]["mask_value"]) == 5 and list(cl[0]["xx"]) == [10, 10] and list(cl[0]["yy"]) == [20, 20]


def test_border_values():
    w, h = 64, 48
    mask = np.full((h, w), 9, F)
    xs = np.array([2, 3, w - 3, w - 2, 30, 30, 30, 30], F)
    ys = np.array([20, 20, 20, 20, 2, 3, h - 3, h - 2], F)
    cl = pm.cluster(xs, ys, np.ones(8, F), mask, w, h)
    assert len(cl) == 1 and sorted(cl[0]["members"]) == [1, 2, 5, 6]
    # a coordinate far outside the image or not finite is no member and reads no mask
    cl = pm.cluster(np.array([1e12, np.nan, -5, 30], F), np.array([20, 20, 20, np.inf], F), np.ones(4, F), mask, w, h)
    assert cl == []


def test_negative_zero_joins_zero_and_nan_is_dropped():
    w, h = 64, 48
    mask = np.zeros((h, w), F)
    mask[:, 32:] = -0.0
    mask[10, 10] = np.nan
    u = np.array([5, 40, 10, 6, 41], F)
    v = np.array([10, 10, 10, 10, 10], F)
    cl = pm.cluster(u, v, np.ones(5, F), mask, w, h)
    assert len(cl) == 1 and list(cl[0]["members"]) == [4, 3, 1, 0]


def plane_cluster(n, seed=0, w=64, h=48):
    """n distinct pixels with inverse depths of the plane z = 2 + 0.5 x (exact up to float rounding)"""
    rng = np.random.RandomState(seed)
    pix = rng.choice((w - 6) * (h - 6), n, replace=False)
    xx, yy = 3 + pix % (w - 6), 3 + pix // (w - 6)
    fxi, cxi, _, _ = [float(t) for t in pm.ki(K)]
    rx = fxi * xx + cxi
    Z = 2.0 / (1.0 - 0.5 * rx)
    return xx, yy, (1.0 / Z).astype(F)


def test_zero_idepth_is_member_but_not_in_cloud():
    w, h = 64, 48
    mask = np.full((h, w), 3, F)
    xx, yy, idp = plane_cluster(12)
    idp[4] = 0.0
    xx[4], yy[4] = 60, 44          # the rect's corner comes from the point that is not in the cloud
    cl = pm.fit_planes(xx.astype(F), yy.astype(F), idp, mask, w, h, K, pm.make_draws(0))
    assert len(cl) == 1
    c = cl[0]
    assert c["n"] == 12 and c["n_cloud"] == 11 and c["rect"][1] == 60 and c["rect"][3] == 44 and c["fitted"] == 1
    assert c["inliers"] == 11


@pytest.mark.parametrize("m,fitted", [(9, 0), (10, 1), (11, 1)])
def test_min_points(m, fitted):
    xx, yy, idp = plane_cluster(m, seed=m)
    r = pm.fit(xx, yy, idp, K, pm.make_draws(1))
    assert r["n_cloud"] == m and r["fitted"] == fitted
    if fitted:
        assert r["inliers"] == m and r["refined"]
        n = r["plane"][:3].astype(np.float64)
        # z - 0.5 x = 2  ->  normal (-0.5, 0, 1) / |.|, distance 2 / |.|, sign as the sample's
        ref = np.array([-0.5, 0.0, 1.0]) / np.sqrt(1.25)
        assert abs(abs(n @ ref) - 1) < 1e-6 and abs(abs(float(r["plane"][3])) - 2 / np.sqrt(1.25)) < 1e-5
        assert n @ r["sample"][:3].astype(np.float64) >= 0
    else:
        assert r["best_sample"] == -1 and r["inliers"] == 0 and not r["plane"].any()


def test_triplets_are_distinct_and_cover_the_cloud():
    for m in (3, 4, 10):
        seen = set()
        for d0 in range(m + 1):
            for d1 in range(m):
                for d2 in range(m - 1):
                    t = pm.triplet((d0, d1, d2), m)
                    assert len(set(t)) == 3 and all(0 <= i < m for i in t)
                    seen.add(t)
        assert len(seen) == m * (m - 1) * (m - 2)


def test_collinear_triplet_scores_nothing():
    p = [(F(0), F(0), F(1)), (F(1), F(1), F(2)), (F(2), F(2), F(3))]
    assert pm.sample_model(*p) is None
    # a cloud whose first samples are collinear: the first non-degenerate sample wins, a cloud on one line is not fitted
    xx = np.arange(3, 15)
    yy = np.full(12, 24)               # the row through cy: Y = 0 for every point
    idp = np.full(12, 0.5, F)          # constant depth: all points on the line Y = 0, Z = 2
    r = pm.fit(xx, yy, idp, K, pm.make_draws(2))
    assert r["n_cloud"] == 12 and r["fitted"] == 0 and r["best_sample"] == -1
    yy2 = yy.copy()
    yy2[11] = 30
    draws = pm.make_draws(2).copy()
    draws[0:3] = (0, 0, 0)             # -> cloud points 0, 1, 2: collinear
    draws[3:6] = (0, 0, 9)             # -> 0, 1, 11
    r = pm.fit(xx, yy2, idp, K, draws)
    assert r["fitted"] == 1 and r["best_sample"] == 1 and r["inliers"] == 12


@pytest.mark.parametrize("n,share", [(10, 0.0), (64, 0.3), (300, 0.3), (2000, 0.4)])
@pytest.mark.parametrize("seed", range(6))
def test_planted_plane_inliers_recovered(n, share, seed):
    u, v, idp, planted = pm.planted_plane(seed, n, share)
    w, h = 1224, 368
    mask = np.full((h, w), 2, F)
    cl = pm.fit_planes(u, v, idp, mask, w, h, (718.856, 718.856, 607.19, 185.2), pm.make_draws(seed))
    assert len(cl) == 1 and cl[0]["n"] == n and cl[0]["n_cloud"] == n and cl[0]["fitted"] == 1
    c = cl[0]
    got = np.zeros(n, bool)
    got[c["members"][c["inlier_idx"]]] = True
    assert np.array_equal(got, planted)
    # the refined plane is y = 1.6 up to the noise, with the sign of the winning sample
    p = c["plane"].astype(np.float64)
    assert abs(abs(p[1]) - 1) < 1e-3 and abs(abs(p[3]) - 1.6) < 5e-3 and p[:3] @ c["sample"][:3].astype(np.float64) >= 0


def test_fast_clustering_equals_the_literal_loops():
    for seed in range(4):
        rng = np.random.RandomState(seed)
        w, h = 40, 30
        mask = rng.randint(0, 6, (h, w)).astype(F)
        mask[rng.rand(h, w) < 0.05] = -0.0
        mask[rng.rand(h, w) < 0.02] = np.nan
        u, v = rng.uniform(-2, w + 2, 400).astype(F), rng.uniform(-2, h + 2, 400).astype(F)
        a, b = pm.cluster(u, v, None, mask, w, h), pm.cluster_fast(u, v, None, mask, w, h)
        assert len(a) == len(b) > 3
        for x, y in zip(a, b):
            assert x["mask_value"] == y["mask_value"] and all(np.array_equal(x[k], y[k]) for k in ("members", "xx", "yy"))


def test_float64_floor_of_the_gpu_tests_inputs():
    """the distance between the refinement in float64 and in long double on the planted scenes of tests/test_plane_fit_gpu.py stays under the FLOOR that file's
    bound is tied to (5.3e-15, measured over all its inputs: the 1224x368 cloud gives the largest figure)"""
    worst = 0.0
    for w, h in ((64, 48), (320, 240)):
        for k, sc in enumerate(pc.planted_scenes(w, h).values()):
            args = (sc["u"], sc["v"], sc["idp"], sc["mask"], w, h, sc["K"], pm.make_draws(k))
            for a, b in zip(pm.fit_planes(*args), pm.fit_planes(*args, dtype=np.longdouble)):
                assert a["best_sample"] == b["best_sample"]
                if a["refined"]:
                    worst = max(worst, float(np.abs(a["plane_wide"].astype(np.longdouble) - b["plane_wide"]).max()))
    print("float64 floor on the planted scenes: %.3e" % worst)
    assert 0 < worst <= 5.3e-15
