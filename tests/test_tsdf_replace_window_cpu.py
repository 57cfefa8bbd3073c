"""tests/tsdf_replace_window_model.py on a hand-worked voxel, the planted case in which the order of the list shows, written_total against the pairs' sums, and
the host-only half of nalo_tsdf_replace_frames (nalo_tsdf_replace_frames_plan: the list's checks and skip_unchanged's predicate) on hand-built log entries and
under the address and undefined-behaviour sanitizers as a stand-alone program. No device."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_model as tm
import tsdf_replace_model as rm
import tsdf_replace_window_model as wm
from conftest import ROOT
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth
from test_tsdf_replace_cpu import GRID0, H0, K0, POSES, W0, same, vol_same

F = np.float32


def test_exports_and_entry_points():
    for s in ("nalo_tsdf_replace_depth_n", "nalo_tsdf_replace_last_n", "nalo_tsdf_replace_frames", "nalo_tsdf_replace_frames_plan"):
        assert s in binding.EXPORTS and hasattr(binding.host_lib(), s)
    for m in ("tsdf_replace_depth_n", "tsdf_replace_last_n", "tsdf_replace_frames"):
        assert callable(getattr(binding.Context, m))


def test_one_voxel_by_hand_through_three_pairs():
    """tests/test_tsdf_cpu.py's 1x1x1 grid, voxel centre (0, 0, 2), pixel (8, 6), trunc 0.5, max_weight = 2. The voxel starts at (0.25, 1). Pair 0 removes
    (weight 1: a reset) and adds d = 0.5; pair 1 adds d = -0.5, which takes the weight to max_weight; pair 2 removes d = 0.25"""
    K = (10.0, 10.0, 8.0, 6.0)

    def side(D):
        depth = np.full((12, 16), 9.0, F)
        depth[6, 8] = D
        return rm.side(depth, K, EYE, 1.0, 0.5, 4.0)
    for literal in (False, True):
        vol = tm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, 2.0)
        vol["tsdf"][:], vol["weight"][:] = 0.25, 1.0
        r = wm.replace_n(vol, [dict(remove=side(2.125), add=side(2.25)), dict(add=side(1.75)), dict(remove=side(2.125))], literal)
        assert r["pairs"] == [dict(removed=1, reset=1, added=1, written=1), dict(removed=0, reset=0, added=1, written=1), dict(removed=1, reset=0, added=0, written=1)]
        assert literal or r["written_total"] == 1
        # reset: (1, 0); add 0.5: ((1 * 0 + 0.5) / 1, 1); add -0.5: ((0.5 * 1 - 0.5) / 2, min(2, 2)) = (0, 2); remove 0.25: ((0 * 2 - 0.25) / 1, 1)
        assert (vol["tsdf"][0, 0, 0], vol["weight"][0, 0, 0]) == (-0.25, 1.0)
    # one more add at max_weight = 2 and the chain no longer inverts: the mean has forgotten a plane
    vol = tm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, 2.0)
    wm.replace_n(vol, [dict(add=side(2.25)), dict(add=side(2.25)), dict(add=side(1.75)), dict(remove=side(1.75))])
    assert vol["weight"][0, 0, 0] == 1.0 and vol["tsdf"][0, 0, 0] == ((F(0.5) * F(2) - F(0.5)) / F(3) * F(2) + F(0.5)) / F(1)


def order_volumes():
    """wm.order_case() in the model: the fused volume, and the two pairs as model pairs"""
    import tsdf_color_model as cm
    g, fused, pairs = wm.order_case()
    vol = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    for sd in fused:
        rm.replace(vol, add=rm.side(*sd))
    mp = [dict(remove=None if p["remove"] is None else rm.side(*p["remove"]), add=None if p["add"] is None else rm.side(*p["add"])) for p in pairs]
    return vol, mp


def test_the_order_of_the_list_shows_in_the_planted_case():
    vol, pairs = order_volumes()
    assert vol["weight"].max() == 4.0 and (vol["weight"] == 1.0).sum() > 10
    before = vol["weight"].copy()
    a = dict(vol, **{k: vol[k].copy() for k in ("tsdf", "weight", "colour")})
    b = dict(vol, **{k: vol[k].copy() for k in ("tsdf", "weight", "colour")})
    ra, rb = wm.replace_n(a, pairs), wm.replace_n(b, pairs[::-1])
    assert ra["written_total"] == rb["written_total"] > 500 and np.array_equal(ra["fired"], rb["fired"])      # the predicates do not depend on the order
    both = rm.sample(vol, pairs[0]["remove"])[0] & rm.sample(vol, pairs[1]["add"])[0]
    one, sat = both & (before == 1.0), both & (before == 4.0)
    assert one.sum() > 5 and sat.sum() > 20
    # weight 1: reset, then the add into the initial values, against the add first and a removal that leaves a mean of weight 1
    assert (a["weight"][one] == 1.0).all() and (b["weight"][one] == 1.0).all()
    # saturated: 4 -> 3 -> 4 against 4 -> 4 -> 3
    assert (a["weight"][sat] == 4.0).all() and (b["weight"][sat] == 3.0).all()
    assert not same(a["weight"], b["weight"]) and not same(a["tsdf"], b["tsdf"]) and not same(a["colour"], b["colour"])
    assert ra["pairs"][0]["reset"] > rb["pairs"][1]["reset"]                      # the reversed list resets fewer voxels: the add came first
    # the literal form agrees with the vectorised one on the chain
    c = dict(vol, **{k: vol[k].copy() for k in ("tsdf", "weight", "colour")})
    rc = wm.replace_n(c, pairs, literal=True)
    assert rc["pairs"] == ra["pairs"] and vol_same(a, c)


def test_written_total_against_the_sum_over_the_pairs():
    g = GRID0
    planes = [rm.side(wavy_depth(W0, H0, 30 + q), K0, POSES[q % 3], 1.0, 0.5, 3.5) for q in range(4)]
    vol = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 4.0)
    # overlapping frusta: the same voxels fire in several pairs and are counted once
    r = wm.replace_n(vol, [dict(add=planes[0]), dict(add=planes[1]), dict(remove=planes[0], add=planes[2]), dict(remove=planes[1], add=planes[3])])
    total = sum(p["written"] for p in r["pairs"])
    assert 0 < r["written_total"] < total and r["written_total"] >= max(p["written"] for p in r["pairs"])
    assert all(p["written"] <= p["removed"] + p["added"] and p["written"] >= max(p["removed"], p["added"]) and p["reset"] <= p["removed"] for p in r["pairs"])
    # frusta that do not meet: equality
    KN = (200.0, 200.0, 31.5, 23.5)
    apart = [rm.side(wavy_depth(W0, H0, 40 + q), KN, pose(0, 0, 0, (tx, 0.0, 0.0)), 1.0, 0.5, 3.5) for q, tx in enumerate((-0.6, 0.99))]
    g = wm.order_case()[0]                                                      # the 33x17x5 grid, where tests/test_tsdf_replace_gpu.py keeps these two frusta apart
    vol = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], 4.0)
    r = wm.replace_n(vol, [dict(add=apart[0]), dict(add=apart[1])])
    assert all(p["written"] > 0 for p in r["pairs"]) and r["written_total"] == sum(p["written"] for p in r["pairs"])
    lo, hi, visited = wm.hull_n(vol, [dict(add=apart[0]), dict(add=apart[1])])
    assert visited > sum(rm.hull(vol, add=sd)[2] for sd in apart)                 # and the hull is larger than the two boxes together


def test_skip_unchanged_on_hand_built_entries():
    pa, pb = pose(0.1, 0.2, 0.3, (0.4, 0.5, 0.6)), pose(0.1, 0.2, 0.3, (0.4, 0.5, np.nextafter(0.6, 1.0)))
    K = (70.0, 68.0, 31.5, 23.5)
    log = [binding.tsdf_log_entry(7, 100, pa, 1.0, K, 0.5, 8.0), binding.tsdf_log_entry(9, 50, pb, 1.02, K, 0.5, 8.0), binding.tsdf_log_entry(11, 60, pa, 1.0, K, 0.5, 8.0)]
    args = lambda ids, poses, s=1.0, K_=K, mn=0.5, mx=8.0, skip=True: binding.tsdf_replace_frames_args(ids, poses, K_, mn, mx, s, skip)
    plan = binding.tsdf_replace_frames_plan
    assert plan(args([7, 9, 11], [pa, pb, pa], s=[1.0, 1.02, 1.0]), log, [100, 50, 60]) == [True, True, True]
    assert plan(args([7, 9, 11], [pa, pb, pa], s=[1.0, 1.02, 1.0], skip=False), log, [100, 50, 60]) == [False, False, False]
    # one ulp in a translation, another scale, a list that has grown, a frame without an entry, a frame that is removed only
    assert plan(args([7, 9, 11, 13], [pb, pb, pa, pa], s=[1.0, 1.0, 1.0, 1.0]), log, [100, 50, 61, 10]) == [False, False, False, False]
    assert plan(args([11, 7], [None, pa]), log, [60, 100]) == [False, True]
    assert plan(args([7], None), log, [100]) == [False]
    # K and the range, bit for bit: -0.0 is not 0.0, one ulp is not equal
    assert plan(args([7], [pa], K_=(70.0, 68.0, 31.5, np.nextafter(F(23.5), F(24)))), log, [100]) == [False]
    assert plan(args([7], [pa], mn=np.nextafter(F(0.5), F(1))), log, [100]) == [False] and plan(args([7], [pa], mx=7.5), log, [100]) == [False]
    zero = [binding.tsdf_log_entry(7, 100, pa, 1.0, K, 0.0, 8.0)]
    assert plan(args([7], [pa], mn=0.0), zero, [100]) == [True] and plan(args([7], [pa], mn=-0.0), zero, [100]) == [False]
    assert plan(args([7], [pa]), log, None) == [False]                            # no list lengths: nothing is skipped
    # the list's own refusals
    for bad in (args([], []), args(list(range(17)), [pa] * 17), args([7, 9, 7], [pa] * 3), args([7], [np.full((3, 4), np.nan)]), args([7], [pa], s=0.0), args([7], [pa], s=np.nan),
                args([7], [pa], K_=(np.inf, 1.0, 1.0, 1.0)), args([7], [pa], mn=3.0, mx=1.0), args([7], [pa], mx=np.nan)):
        with pytest.raises(binding.NaloError):
            plan(bad, log, None)
    assert plan(args(list(range(16)), [pa] * 16), log, None) == [False] * 16
    assert plan(args([7], None, K_=(np.nan,) * 4, mn=3.0, mx=1.0), log, [100]) == [False]      # removed only: K and the range are not looked at


SAN_MAIN = r'''
#include <cmath>
#include <cstdio>
#include <vector>
#include "nalo_gpu.h"
int main() {
    int bad = 0;
    const nalo_tsdf_align_est good = {{1, 0, 0, 0.25, 0, 1, 0, -0.5, 0, 0, 1, 2.0}, 1.0};
    std::vector<nalo_tsdf_log_entry> log;
    for (int q = 0; q < 16; ++q) { nalo_tsdf_log_entry e = {}; e.frame_id = 100 + q; e.n_records = 10 + q; e.est = good; e.K[0] = e.K[1] = 50.f; e.K[2] = 15.5f; e.K[3] = 11.5f; e.min_depth = 0.5f; e.max_depth = 8.f; log.push_back(e); }
    for (int n : {0, 1, 16, 17}) {
        // heap arrays of exactly n elements: a read past the list is the sanitizer's to catch
        std::vector<int> ids((size_t)n), len((size_t)n);
        std::vector<nalo_tsdf_align_est> est((size_t)n, good);
        std::vector<unsigned char> has((size_t)n, 1), skip((size_t)(n > 16 ? 16 : n) + 1, 7);
        for (int k = 0; k < n; ++k) { ids[k] = 100 + k; len[k] = 10 + k; }
        nalo_tsdf_replace_frames_args a = {};
        a.n = n; a.frame_id = ids.data(); a.est_new = est.data(); a.has_est = has.data();
        a.K[0] = a.K[1] = 50.f; a.K[2] = 15.5f; a.K[3] = 11.5f; a.min_depth = 0.5f; a.max_depth = 8.f; a.skip_unchanged = 1;
        const int want = (n >= 1 && n <= 16) ? 0 : -1;
        int rc = nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), len.data(), skip.data());
        if (rc != want) ++bad;
        if (rc == 0) for (int k = 0; k < n; ++k) if (skip[k] != 1) ++bad;       // every frame is where it was fused
        if (skip.back() != 7) ++bad;
        std::printf("n %d: %d\n", n, rc);
        if (want) continue;
        a.skip_unchanged = 0;
        rc = nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), nullptr, skip.data());
        if (rc != 0) ++bad;
        for (int k = 0; k < n; ++k) if (skip[k] != 0) ++bad;
        a.skip_unchanged = 1;
        if (n > 1) {                                                            // a duplicate, first and last
            ids[n - 1] = ids[0];
            if (nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), len.data(), skip.data()) != -1) ++bad;
            ids[n - 1] = 100 + n - 1;
        }
        for (double v : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {   // NaN and infinite estimates, in the last frame
            est[n - 1] = good; est[n - 1].camToWorld[11] = v;
            if (nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), len.data(), skip.data()) != -1) ++bad;
            est[n - 1] = good; est[n - 1].s = v;
            if (nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), len.data(), skip.data()) != -1) ++bad;
            has[n - 1] = 0;                                                     // removed only: the estimate is not looked at
            if (nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), len.data(), skip.data()) != 0 || skip[n - 1] != 0) ++bad;
            has[n - 1] = 1; est[n - 1] = good;
        }
        for (float s : {0.f, -1.f, 1e-45f}) {
            est[0].s = s;
            if (nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), len.data(), skip.data()) != (s > 0.f ? 0 : -1)) ++bad;
            est[0] = good;
        }
        a.K[3] = NAN;
        if (nalo_tsdf_replace_frames_plan(&a, log.data(), (int)log.size(), len.data(), skip.data()) != -1) ++bad;
        a.K[3] = 11.5f;
        // an empty log, a NULL log of no entries, NULL pieces
        if (nalo_tsdf_replace_frames_plan(&a, nullptr, 0, len.data(), skip.data()) != 0) ++bad;
        for (int k = 0; k < n; ++k) if (skip[k] != 0) ++bad;
        if (nalo_tsdf_replace_frames_plan(&a, nullptr, 3, len.data(), skip.data()) != -1 || nalo_tsdf_replace_frames_plan(&a, log.data(), -1, len.data(), skip.data()) != -1) ++bad;
        if (nalo_tsdf_replace_frames_plan(nullptr, log.data(), 16, len.data(), skip.data()) != -1 || nalo_tsdf_replace_frames_plan(&a, log.data(), 16, len.data(), nullptr) != -1) ++bad;
        a.frame_id = nullptr;
        if (nalo_tsdf_replace_frames_plan(&a, log.data(), 16, len.data(), skip.data()) != -1) ++bad;
        a.frame_id = ids.data(); a.est_new = nullptr;
        if (nalo_tsdf_replace_frames_plan(&a, log.data(), 16, len.data(), skip.data()) != 0) ++bad;
    }
    std::printf("bad %d\n", bad);
    return bad;
}
'''


def test_the_plan_helper_under_the_sanitizers(tmp_path):
    """nalo-slam_amd/csrc/host_tsdf.cpp with a main of its own under -fsanitize=address,undefined: nalo_tsdf_replace_frames_plan on lists of 0, 1, 16 and 17
    frames in heap arrays of exactly that length, duplicate ids, NaN and infinite estimates, scales of 0, below 0 and denormal, a NaN K, an empty and a NULL log"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_replace_window_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(ROOT, "nalo-slam_amd", "csrc", "host_tsdf.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    assert p.stdout.count("\n") == 5 and p.stdout.endswith("bad 0\n")
