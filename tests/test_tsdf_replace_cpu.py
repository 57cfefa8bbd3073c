"""tests/tsdf_replace_model.py on hand-worked inputs, its two forms against each other and against tests/tsdf_model.py at s == 1, the removal as the inverse of
the add (and where it is not), and the host-only half of "The replacement" (nalo_tsdf_est_world_to_cam, nalo_tsdf_frustum_box_est, nalo_tsdf_box_shift)
against the model and under the address and undefined-behaviour sanitizers as a stand-alone program. No device."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import tsdf_color_model as cm
import tsdf_model as tm
import tsdf_replace_model as rm
from conftest import ROOT
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, desc_of, pose, seeded_case, wavy_depth

F = np.float32
W0, H0 = 64, 48
K0 = (70.0, 68.0, 31.5, 23.5)
POSES = [EYE, pose(0.15, -0.25, 0.1, (0.2, -0.1, 0.15)), pose(-0.3, 0.35, 1.2, (-0.25, 0.2, -0.1))]      # tests/test_tsdf_gpu.py's
GRID0 = dict(origin=(-1.2, -0.9, 0.9), vs=0.075, dims=(32, 24, 40), trunc=0.25)


def same(a, b):
    """bit for bit, every NaN counting as one value: IEEE 754 leaves the sign and payload of a NaN an operation makes (inf / inf, inf - inf) to the machine"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def vol_same(a, b):
    return same(a["tsdf"], b["tsdf"]) and same(a["weight"], b["weight"]) and ("colour" not in a or same(a["colour"], b["colour"]))


def six_planes(gi=0):
    """the six integrations of tests/test_tsdf_gpu.py's `fused` fixture on grid gi: (depth, pose) in its order"""
    return [(wavy_depth(W0, H0, 10 * gi + pi, base=2.0 + 0.02 * rnd), POSES[pi]) for rnd in range(2) for pi in range(3)]


def test_exports_and_entry_points():
    for s in ("nalo_tsdf_replace_depth", "nalo_tsdf_replace_last", "nalo_tsdf_replace_frame", "nalo_tsdf_log_enable", "nalo_tsdf_log_get", "nalo_tsdf_est_world_to_cam",
              "nalo_tsdf_frustum_box_est", "nalo_tsdf_box_shift"):
        assert s in binding.EXPORTS and hasattr(binding.host_lib(), s)
    for m in ("tsdf_replace_depth", "tsdf_replace_last", "tsdf_replace_frame", "tsdf_log_enable", "tsdf_log_get"):
        assert callable(getattr(binding.Context, m))


@pytest.mark.parametrize("s_r,s_a", [(1.0, 1.0), (0.8, 1.25), (2.0, 0.5)])
def test_vectorised_model_equals_the_literal_one(s_r, s_a):
    K, w, h = (20.0, 19.0, 11.5, 8.5), 24, 18
    rng = np.random.RandomState(7)
    a, b = (cm.volume((-1.1, -0.9, 0.8), 0.17, (13, 11, 12), 0.4, 3.0) for _ in range(2))
    bgr = rng.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    planes = [rm.side(wavy_depth(w, h, 3 + q), K, c2w, 1.0, 0.5, 3.0, bgr[q]) for q, c2w in enumerate((EYE, pose(0.2, -0.3, 0.1, (0.1, -0.2, 0.3)), pose(-0.1, 0.2, 0.0, (0.0, 0.1, -0.2))))]
    for sd in planes + planes[:2]:                                             # five adds: weights 0 .. 3, some saturated
        na, nb = rm.replace_literal(a, add=sd), rm.replace(b, add=sd)
        assert na["added"] == nb["added"] == na["written"] == nb["written"] > 50 and vol_same(a, b)
    assert a["weight"].max() == 3.0 and (a["weight"] == 1.0).sum() > 10
    # removal only, coloured and not, with and without a box; then a replacement whose sides differ in pose, scale and plane
    for kw in (dict(remove=dict(planes[0], s=s_r)), dict(remove=dict(planes[1], s=s_r, bgr=None), box=((2, 1, 3), (7, 9, 5))),
               dict(remove=dict(planes[2], s=s_r), add=dict(planes[0], s=s_a, c2w=pose(0.02, -0.01, 0.0, (0.05, 0.0, 0.02)))),
               dict(remove=dict(planes[0], s=s_r), add=dict(planes[1], s=s_a, bgr=None), box=((0, 0, 0), (13, 5, 12)))):
        na, nb = rm.replace_literal(a, **kw), rm.replace(b, **kw)
        assert all(na[k] == nb[k] for k in na) and na["removed"] > 30 and na["written"] >= max(na["removed"], na["added"]) and vol_same(a, b), kw.keys()
        if "box" in kw:
            assert nb["rem"].sum() < rm.sample(b, kw["remove"])[0].sum()          # the box cut voxels the side would have taken
    assert na["reset"] > 0 and na["removed"] > na["reset"]


def one_voxel(t0, w0, depth_value=2.25, max_weight=4.0, s=1.0):
    """a 1x1x1 grid whose voxel centre is (0, 0, 2) seen at the identity by pixel (8, 6) (tests/test_tsdf_cpu.py's one_voxel); d = (depth - 2) s / 0.5"""
    vol = cm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, max_weight)
    vol["tsdf"][:], vol["weight"][:], vol["colour"][:] = t0, w0, 100.0
    depth = np.full((12, 16), 9.0, F)
    depth[6, 8] = depth_value
    bgr = np.full((12, 16, 3), 40, np.uint8)
    sd = rm.side(depth, (10.0, 10.0, 8.0, 6.0), EYE, s, 0.5, 4.0, bgr)
    twin = dict(vol, tsdf=vol["tsdf"].copy(), weight=vol["weight"].copy(), colour=vol["colour"].copy())
    n, m = rm.replace(vol, remove=sd), rm.replace_literal(twin, remove=sd)
    assert all(n[k] == m[k] for k in m) and vol_same(vol, twin)
    return vol["tsdf"][0, 0, 0], vol["weight"][0, 0, 0], vol["colour"][0, 0, 0, 0], n


def test_one_voxel_by_hand_through_every_branch_of_the_removal():
    up = np.nextafter(F(1.0), F(2.0))
    # w0 = 0, 1, a NaN: the initial values, colour too; counted as removed and reset
    for w0 in (0.0, 1.0, np.nan, 0.5, -3.0):
        t, w, c, n = one_voxel(0.3, w0)
        assert (t, w, c) == (1.0, 0.0, 0.0) and (n["removed"], n["reset"], n["written"]) == (1, 1, 1), w0
    # one ulp above 1: w1 = 2^-23 > 0, the quotient is taken, every step exact: 0.5 * (1 + 2^-23) = 0.5 + 2^-24, minus d = 0.5, over 2^-23
    t, w, c, n = one_voxel(0.5, up)
    assert (t, w) == (0.5, F(2.0 ** -23)) and n["reset"] == 0 and n["removed"] == 1
    # w0 = 2: (t0 * 2 - d) / 1 with d = 0.5: 0.25 * 2 - 0.5 = 0; colour (100 * 2 - 40) / 1
    assert one_voxel(0.25, 2.0)[:3] == (0.0, 1.0, 160.0)
    # the inverse of the add on an unsaturated voxel: (0.5 * 1 + 0) / 2 = 0.25 at weight 2 was made from t = 0.5 and d = 0
    assert one_voxel(0.25, 2.0, depth_value=2.0)[:2] == (0.5, 1.0)
    # saturated at max_weight = 4: the removal still divides by w0 - 1 = 3, whatever number of planes the mean really holds
    t, w, c, n = one_voxel(0.5, 4.0)
    assert (t, w) == ((F(0.5) * F(4.0) - F(0.5)) / F(3.0), 3.0) and c == (F(100.0) * F(4.0) - F(40.0)) / F(3.0)
    # +inf: w1 = inf > 0; inf / inf is a NaN, the weight stays inf. t0 NaN: the NaN goes through, the weight is w1
    t, w, c, n = one_voxel(0.5, np.inf)
    assert np.isnan(t) and w == np.inf and n["reset"] == 0
    t, w, c, n = one_voxel(np.nan, 3.0)
    assert np.isnan(t) and w == 2.0 and c == (F(100.0) * F(3.0) - F(40.0)) / F(2.0)
    # the scale s = 2: M = R^T / 2 puts the voxel at zc = 1 and still at pixel (8, 6). sdf = (1.125 - 1) * 2 = 0.25 -> d = 0.5: (1 * 2 - 0.5) / 1
    assert one_voxel(1.0, 2.0, depth_value=1.125, s=2.0)[:2] == (1.5, 1.0)
    # the predicate's skip is taken on the scaled sdf: (0.7 - 1) * 2 = -0.6 < -trunc leaves the voxel alone (unscaled, -0.3 would not); (0.8 - 1) * 2 = -0.4 does not
    assert one_voxel(0.3, 2.0, depth_value=0.7, s=2.0)[3]["written"] == 0 and one_voxel(0.3, 2.0, depth_value=0.8, s=2.0)[3]["removed"] == 1


def test_an_add_at_scale_one_is_the_integration():
    g = GRID0
    a, b = (cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 4.0) for _ in range(2))
    rng = np.random.RandomState(3)
    for q, (depth, c2w) in enumerate(six_planes()):
        bgr = rng.randint(0, 256, (H0, W0, 3)).astype(np.uint8)
        r = cm.integrate(a, depth, bgr, K0, c2w, 0.5, 3.5)
        n = rm.replace(b, add=rm.side(depth, K0, c2w, 1.0, 0.5, 3.5, bgr))
        assert n["added"] == r["updated"] > 300 and np.array_equal(n["add"], r["code"] == tm.UPDATED)
        assert a["tsdf"].tobytes() == b["tsdf"].tobytes() and a["weight"].tobytes() == b["weight"].tobytes() and a["colour"].tobytes() == b["colour"].tobytes()
        assert rm.est_world_to_cam(c2w, 1.0).tobytes() == tm.world_to_cam(c2w).tobytes()
        assert rm.hull(b, add=rm.side(depth, K0, c2w, 1.0, 0.5, 3.5))[:2] == tm.frustum_box(a, W0, H0, K0, c2w, 3.5)
    assert a["weight"].max() == 4.0


@pytest.mark.parametrize("order", ["same", "reversed"])
def test_adds_then_removals_give_the_initial_bytes_while_the_weight_has_room(order):
    g = GRID0
    vol = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 64.0)
    rng = np.random.RandomState(5)
    sides = [rm.side(d, K0, c2w, 1.0, 0.5, 3.5, rng.randint(0, 256, (H0, W0, 3)).astype(np.uint8)) for d, c2w in six_planes()]
    for sd in sides:
        rm.replace(vol, add=sd)
    assert vol["weight"].max() == 6.0 and (vol["tsdf"] != 1.0).sum() > 2000 and (vol["colour"] != 0).sum() > 6000
    resets = 0
    for sd in (sides if order == "same" else sides[::-1]):
        resets += rm.replace(vol, remove=sd)["reset"]
    fresh = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 64.0)
    assert resets > 2000 and vol["tsdf"].tobytes() == fresh["tsdf"].tobytes() and vol["weight"].tobytes() == fresh["weight"].tobytes() and vol["colour"].tobytes() == fresh["colour"].tobytes()


def test_with_a_saturated_weight_the_removal_is_not_the_inverse():
    """max_weight = 4 under the same six planes: the saturation clause is reached. Removing all six still ENDS at the initial values - a voxel that sat at 4
    is reset by its fourth removal and again by every later one - but what a removal leaves on the way is not what the remaining planes would have fused"""
    g = GRID0
    vol = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 4.0)
    sides = [rm.side(d, K0, c2w, 1.0, 0.5, 3.5) for d, c2w in six_planes()]
    for sd in sides:
        rm.replace(vol, add=sd)
    sat = vol["weight"] == 4.0
    assert sat.sum() > 100
    seen = np.zeros(sat.shape, np.int32)
    for sd in sides:
        seen += rm.replace(vol, remove=sd)["rem"]
    # a voxel five or six planes saw sat at 4 and is back at the initial values after four removals: the later ones find w0 = 0 and reset it again, so the
    # volume IS initial there. What differs is the path: the running mean forgot planes, and the intermediate values are not those of the remaining planes
    assert (seen[sat] >= 4).all() and vol["weight"].max() == 0.0
    # the intermediate state: remove the first plane only, against a volume that fused planes 1 .. 5 alone
    vol = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 4.0)
    rest = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 4.0)
    for q, sd in enumerate(sides):
        rm.replace(vol, add=sd)
        if q:
            rm.replace(rest, add=sd)
    rm.replace(vol, remove=sides[0])
    differs = (vol["weight"] != rest["weight"]) & sat
    assert differs.sum() > 50 and (vol["weight"][differs] == 3.0).all() and (rest["weight"][differs] == 4.0).all()      # 4 - 1, where four or five planes remain
    assert (vol["tsdf"][differs] != rest["tsdf"][differs]).sum() > 50
    loose = ~sat & (vol["weight"] > 0)
    assert loose.sum() > 100 and np.array_equal(vol["weight"][loose], rest["weight"][loose])       # and where the weight never saturated the count is exact


def test_the_float_removal_against_exact_rational_arithmetic():
    """q = fl(fl(fl(t0 w0) - d) / w1) with w1 = w0 - 1 exact for 1 < w0 < 2^24 (Sterbenz below 2, a multiple of ulp(w0) above). Round to nearest has relative
    error at most v = u / (1 + u), u = 2^-24, per operation: with A = |t0| w0 and B = |t0 w0 - d| <= A + |d| the error of q is at most
    (A v (1 + v)^2 + B ((1 + v)^2 - 1)) / w1 <= (A + |d|) ((1 + v)^3 - 1) / w1, and (1 + v)^3 - 1 = (3u + 9u^2 + 7u^3) / (1 + u)^3 < 3u. Three roundings, derived."""
    rng = np.random.RandomState(11)
    n = 20000
    t0 = rng.uniform(-1, 1, n).astype(F)
    w0 = np.concatenate([rng.randint(2, 65, n // 2).astype(F), (1.0 + rng.uniform(0, 63, n - n // 2)).astype(F)])
    w0[:8] = [np.nextafter(F(1), F(2)), 2, 3, 64, 1.5, 1.0000119, 63.99999, 2.0000002]
    d = np.fmin(F(1.0), rng.uniform(-1, 1.5, n).astype(F))
    w1 = w0 - F(1.0)
    assert (w1 > 0).all() and all(Fraction(float(a)) - 1 == Fraction(float(b)) for a, b in zip(w0[:200], w1[:200]))
    q = (t0 * w0 - d) / w1
    assert q.dtype == F
    u3 = 3 * Fraction(1, 2 ** 24)
    worst = Fraction(0)
    for a, b, c, e, got in zip(t0.tolist(), w0.tolist(), d.tolist(), w1.tolist(), q.tolist()):
        a, b, c, e = Fraction(a), Fraction(b), Fraction(c), Fraction(e)
        exact, bound = (a * b - c) / e, u3 * (abs(a) * b + abs(c)) / e
        err = abs(Fraction(got) - exact)
        assert err <= bound, (a, b, c, float(err), float(bound))
        if bound:
            worst = max(worst, err / bound)
    print("removal against exact arithmetic: worst error / bound = %.3f over %d voxels" % (float(worst), n))
    assert worst > Fraction(1, 20)                                             # the bound is of the error's order, not a formality


def test_est_matrix_and_box_against_the_model_on_seeded_poses():
    n_boxes = 0
    for seed in range(200):
        vol, c2w, w, h, K, max_depth, rng = seeded_case(seed)
        s = float(np.exp(rng.uniform(-1.0, 1.0)))
        assert binding.tsdf_est_world_to_cam(c2w, s).tobytes() == rm.est_world_to_cam(c2w, s).tobytes(), seed
        assert binding.tsdf_est_world_to_cam(c2w, 1.0).tobytes() == tm.world_to_cam(c2w).tobytes(), seed
        lo, hi = binding.tsdf_frustum_box_est(desc_of(vol), w, h, K, c2w, s, max_depth)
        assert (tuple(lo), tuple(hi)) == rm.frustum_box_est(vol, w, h, K, c2w, s, max_depth), seed
        lo1, hi1 = binding.tsdf_frustum_box_est(desc_of(vol), w, h, K, c2w, 1.0, max_depth)
        lo0, hi0 = binding.tsdf_frustum_box(desc_of(vol), w, h, K, c2w, max_depth)
        assert (tuple(lo1), tuple(hi1)) == (tuple(lo0), tuple(hi0)) == tm.frustum_box(vol, w, h, K, c2w, max_depth), seed
        n_boxes += hi[0] > lo[0]
    assert n_boxes >= 60
    for bad in (dict(s=0.0), dict(s=-1.0), dict(s=np.nan), dict(s=np.inf), dict(c2w=pose(0, 0, 0, (np.nan, 0, 0))), dict(c2w=pose(0, 0, 0, (0, np.inf, 0)))):
        a = dict(c2w=EYE, s=1.0)
        a.update(bad)
        with pytest.raises(binding.NaloError):
            binding.tsdf_est_world_to_cam(a["c2w"], a["s"])
        with pytest.raises(binding.NaloError):
            binding.tsdf_frustum_box_est(desc_of(tm.volume((0, 0, 0), 0.1, (8, 8, 8), 0.2, 4.0)), 32, 24, (30.0, 30.0, 15.5, 11.5), a["c2w"], a["s"], 2.0)


@pytest.mark.parametrize("s", [0.5, 1.25, 2.0])
def test_the_box_holds_every_voxel_the_model_adds_or_removes(s):
    n_touched = 0
    for seed in range(120):
        vol, c2w, w, h, K, max_depth, rng = seeded_case(seed)
        depth = rng.uniform(0.1, max_depth * 1.2, (h, w)).astype(F)
        sd = rm.side(depth, K, c2w, s, 0.1, max_depth)
        lo, hi = binding.tsdf_frustum_box_est(desc_of(vol), w, h, K, c2w, s, max_depth)
        vol["weight"][:] = 2.0
        n = rm.replace(vol, remove=sd, add=sd)
        assert np.array_equal(n["rem"], n["add"])
        k, j, i = np.nonzero(n["rem"])
        if len(i):
            n_touched += 1
            assert lo[0] <= i.min() and i.max() < hi[0] and lo[1] <= j.min() and j.max() < hi[1] and lo[2] <= k.min() and k.max() < hi[2], (seed, lo, hi)
    assert n_touched >= 30, n_touched                                          # the property was exercised, not vacuous


def test_box_shift_by_brute_force():
    rng = np.random.RandomState(2)
    n_empty = n_cut = 0
    for q in range(4000):
        dims = rng.randint(1, 7, 3)
        shift = rng.randint(-2, 3, 3) if q % 2 else rng.randint(-8, 9, 3)
        lo = rng.randint(-2, 4, 3)
        size = rng.randint(-1, 8, 3) if q % 4 == 0 else rng.randint(1, 8, 3)
        glo, gsize = binding.tsdf_box_shift(dims, shift, lo, size)
        assert (tuple(glo), tuple(gsize)) == rm.box_shift(dims, shift, lo, size), (dims, shift, lo, size)
        # every cell of the (unclipped) box lands at its index - shift; those inside the grid are the result
        cells = set()
        for i in range(lo[0], lo[0] + max(size[0], 0)):
            for j in range(lo[1], lo[1] + max(size[1], 0)):
                for k in range(lo[2], lo[2] + max(size[2], 0)):
                    p = (i - shift[0], j - shift[1], k - shift[2])
                    if all(0 <= p[a] < dims[a] for a in range(3)):
                        cells.add(p)
        want = {(i, j, k) for i in range(glo[0], glo[0] + gsize[0]) for j in range(glo[1], glo[1] + gsize[1]) for k in range(glo[2], glo[2] + gsize[2])}
        assert cells == want, (dims, shift, lo, size)
        n_empty += not cells
        n_cut += 0 < len(cells) < max(size[0], 0) * max(size[1], 0) * max(size[2], 0)
        if not cells:
            assert tuple(glo) == tuple(gsize) == (0, 0, 0)
    assert n_empty > 500 and n_cut > 500
    with pytest.raises(binding.NaloError):
        binding.tsdf_box_shift((0, 4, 4), (0, 0, 0), (0, 0, 0), (1, 1, 1))
    with pytest.raises(binding.NaloError):
        binding.tsdf_box_shift((4, 4, 2049), (0, 0, 0), (0, 0, 0), (1, 1, 1))


def test_the_log_model_follows_a_shift():
    log = []
    rm.log_put(log, (8, 6, 4), 7, 100, EYE, 1.0, K0, 0.5, 3.5)
    rm.log_put(log, (8, 6, 4), 9, 50, POSES[1], 1.0, K0, 0.5, 3.5)
    rm.log_shift(log, (8, 6, 4), (0, 0, 0))
    assert [e["size"] for e in log] == [(8, 6, 4)] * 2
    rm.log_shift(log, (8, 6, 4), (3, 0, -1))
    assert [(e["lo"], e["size"]) for e in log] == [((0, 0, 1), (5, 6, 3))] * 2
    rm.log_put(log, (8, 6, 4), 9, 60, POSES[2], 1.02, K0, 0.5, 3.5)            # replaced: resident in the whole grid again, its place in the order kept
    assert [e["frame_id"] for e in log] == [7, 9] and log[1]["size"] == (8, 6, 4) and log[1]["n_records"] == 60 and log[1]["s"] == 1.02
    rm.log_shift(log, (8, 6, 4), (5, 0, 0))
    assert [(e["frame_id"], e["lo"], e["size"]) for e in log] == [(9, (0, 0, 0), (3, 6, 4))]      # frame 7's five columns left the grid
    rm.log_drop(log, 9)
    assert log == []


SAN_MAIN = r'''
#include <climits>
#include <cmath>
#include <initializer_list>
#include <cstdio>
#include "nalo_gpu.h"
static int box_in_grid(const nalo_tsdf_desc& d, int rc, const int lo[3], const int hi[3]) {
    if (rc == 0) for (int a = 0; a < 3; ++a) if (lo[a] < 0 || hi[a] > d.dims[a] || lo[a] > hi[a]) return 1;
    return 0;
}
int main() {
    const nalo_tsdf_desc d = {{0.f, 0.f, 0.f}, 0.1f, {8, 8, 8}, 0.2f, 4.f}, one = {{0.f, 0.f, 1.f}, 0.1f, {1, 1, 1}, 0.2f, 4.f};
    const float K[4] = {30.f, 30.f, 15.5f, 11.5f};
    const double scales[] = {1.0, 0.5, 2.0, 0.0, -1.0, NAN, INFINITY, 1e300, 1e-300, 4.9e-324};
    int bad = 0;
    for (double s : scales)
        for (int p = 0; p < 3; ++p) {
            nalo_tsdf_align_est e = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, s};
            if (p == 1) e.camToWorld[3] = e.camToWorld[7] = e.camToWorld[11] = 0.4;
            if (p == 2) { e.camToWorld[3] = 1e30; e.camToWorld[7] = -1e30; e.camToWorld[11] = 1e300; }
            float M[12];
            int lo[3] = {-7, -7, -7}, hi[3] = {-7, -7, -7};
            const int r0 = nalo_tsdf_est_world_to_cam(&e, M);
            const int r1 = nalo_tsdf_frustum_box_est(&d, 32, 24, K, &e, 2.f, lo, hi);
            bad += box_in_grid(d, r1, lo, hi);
            const int r2 = nalo_tsdf_frustum_box_est(&one, 1, 1, K, &e, 3e38f, lo, hi);
            bad += box_in_grid(one, r2, lo, hi);
            const int want = (s > 0.0 && std::isfinite(s)) ? 0 : -1;
            if (r0 != want || r1 != want || r2 != want) ++bad;
            std::printf("s %g pose %d: %d %d %d\n", s, p, r0, r1, r2);
        }
    const int shifts[] = {INT_MIN, INT_MIN + 1, -3, 0, 2, INT_MAX - 1, INT_MAX};
    const int dimss[3][3] = {{1, 1, 1}, {8, 6, 4}, {2048, 1, 2048}};
    for (const auto& dims : dimss)
        for (int sx : shifts)
            for (int sz : shifts)
                for (int l : {INT_MIN, -1, 0, 3, INT_MAX})
                    for (int n : {INT_MIN, 0, 1, 5, INT_MAX}) {
                        const int shift[3] = {sx, 0, sz};
                        int lo[3] = {l, 0, l}, size[3] = {n, 1, n};
                        if (nalo_tsdf_box_shift(dims, shift, lo, size) != 0) ++bad;
                        for (int a = 0; a < 3; ++a) if (lo[a] < 0 || size[a] < 0 || (long long)lo[a] + size[a] > dims[a]) ++bad;
                        if ((size[0] == 0) != (size[1] == 0) || (size[0] == 0) != (size[2] == 0)) ++bad;
                    }
    const int zero[3] = {8, 0, 8}, sh[3] = {0, 0, 0};
    int lo[3] = {0, 0, 0}, size[3] = {1, 1, 1};
    if (nalo_tsdf_box_shift(zero, sh, lo, size) != -1 || nalo_tsdf_box_shift(nullptr, sh, lo, size) != -1) ++bad;
    std::printf("bad %d\n", bad);
    return bad;
}
'''


def test_the_three_helpers_under_the_sanitizers_on_degenerate_inputs(tmp_path):
    """nalo-slam_amd/csrc/host_tsdf.cpp with a main of its own under -fsanitize=address,undefined: scales of 0, negative, NaN, infinite, 1e300 and denormal at
    poses up to 1e300, on an 8^3 grid and a 1-voxel grid; box shifts of INT_MIN / INT_MAX with boxes at INT_MIN / INT_MAX on dims of 1, a small grid and 2048"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_replace_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(ROOT, "nalo-slam_amd", "csrc", "host_tsdf.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    assert p.stdout.count("\n") == 31 and p.stdout.endswith("bad 0\n")
