"""tests/tsdf_shift_model.py against itself and a volume worked by hand, and the host-only half of nalo_tsdf_shift (nalo_tsdf_shift_for, nalo_tsdf_shift_boxes,
the origin formula) against the model, on its refusals and under the address and undefined-behaviour sanitizers as a stand-alone program. No device."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_shift_model as sm
from conftest import ROOT
from nalo_slam_amd import binding

F, U = np.float32, np.uint32


def test_exports_and_entry_points():
    for s in ("nalo_tsdf_shift", "nalo_tsdf_geometry", "nalo_tsdf_shift_for", "nalo_tsdf_shift_boxes"):
        assert s in binding.EXPORTS and hasattr(binding.host_lib(), s)
    for m in ("tsdf_shift", "tsdf_geometry"):
        assert callable(getattr(binding.Context, m))
    assert callable(binding.tsdf_shift_for) and callable(binding.tsdf_shift_boxes)


def test_vectorised_model_equals_the_literal_one():
    rng = np.random.RandomState(1)
    n_kept = n_empty = 0
    for seed in range(120):
        dims = tuple(int(v) for v in rng.randint(1, 8, 3))
        src = sm.random_words(rng, dims[::-1])
        s = tuple(int(v) for v in rng.randint(-9, 10, 3)) if seed % 3 else tuple(int(v) for v in rng.randint(-1, 2, 3))
        init = (sm.ONE, sm.ZERO)[seed % 2]
        a, b = sm.shift_literal(src, s, init), sm.shift_words(src, s, init)
        assert a.dtype == U and a.tobytes() == b.tobytes(), (dims, s)
        kept = all(abs(s[a_]) < dims[a_] for a_ in range(3))
        n_kept += kept
        n_empty += not kept
        if not kept:
            assert (b == init).all()
        if s == (0, 0, 0):
            assert b.tobytes() == src.tobytes()
    assert n_kept >= 30 and n_empty >= 30


def test_a_3x2x2_volume_by_hand():
    # words 100 i + 10 j + k at voxel (i, j, k): array [k][j][i]
    src = np.array([[[100 * i + 10 * j + k for i in range(3)] for j in range(2)] for k in range(2)], U)
    I = U(7)
    for fn in (sm.shift_literal, sm.shift_words):
        # s = (1, 0, 0): voxel i takes voxel i + 1; the low x slab leaves, initial values enter at the high end
        assert fn(src, (1, 0, 0), I).tolist() == [[[100, 200, 7], [110, 210, 7]], [[101, 201, 7], [111, 211, 7]]]
        # s = (-2, 0, 0): voxel 2 takes voxel 0
        assert fn(src, (-2, 0, 0), I).tolist() == [[[7, 7, 0], [7, 7, 10]], [[7, 7, 1], [7, 7, 11]]]
        # s = (0, 1, -1): j takes j + 1, k takes k - 1: only (i, 0, 1) <- (i, 1, 0) lies in the grid
        assert fn(src, (0, 1, -1), I).tolist() == [[[7, 7, 7], [7, 7, 7]], [[10, 110, 210], [7, 7, 7]]]
        assert fn(src, (3, 0, 0), I).tolist() == [[[7] * 3] * 2] * 2 and fn(src, (0, -2, 0), I).tolist() == [[[7] * 3] * 2] * 2
        assert fn(src, (0, 0, 0), I).tobytes() == src.tobytes()
    vol = dict(origin=np.array([-1.0, 0.5, 2.0], F), vs=F(0.25), dims=(3, 2, 2), tsdf=src.view(F).copy(), weight=src.view(F).copy(), colour=None)
    sm.shift_volume(vol, (1, 0, -2))
    assert vol["base"].tolist() == [1, 0, -2] and vol["origin"].tolist() == [-0.75, 0.5, 1.5] and vol["origin0"].tolist() == [-1.0, 0.5, 2.0]
    assert (vol["tsdf"].view(U) == sm.ONE).all() and (vol["weight"].view(U) == 0).all()      # |s2| = nz: nothing is kept
    # the bits that matter pass: a signalling NaN, -0.0f, a denormal
    sp = np.array([[[0xFFA00001, 0x80000000, 0x00000001]]], U)
    assert sm.shift_words(sp, (1, 0, 0), sm.ONE).tolist() == [[[0x80000000, 0x00000001, 0x3F800000]]]


def test_the_recomputed_origin_differs_from_an_accumulated_one_and_returns():
    """origin0 = -12.8f, voxel_size = 0.1f: a running origin += (float)s * vs leaves the formula on almost every step, and only the formula comes back to origin0
    when base comes back to 0. This is what gives the device's geometry test teeth."""
    rng = np.random.RandomState(7)
    o0, vs = F(-12.8), F(0.1)
    acc, base, differ = o0, 0, 0
    for _ in range(200):
        s = int(rng.randint(-40, 41))
        base += s
        acc = F(acc + F(F(s) * vs))
        want = sm.origin([o0, o0, o0], [base, base, base], vs)
        assert want.dtype == F and want[0] == F(o0 + F(F(base) * vs))
        differ += int(want[0] != acc)
    assert differ >= 150, differ
    acc = F(acc + F(F(-base) * vs))
    assert acc != o0 and sm.origin([o0] * 3, [0] * 3, vs)[0] == o0
    # exact at the bound: 2^24 and 2^24 - 1 are both floats
    assert sm.origin([F(0)] * 3, [1 << 24, (1 << 24) - 1, -(1 << 24)], F(1.0)).tolist() == [16777216.0, 16777215.0, -16777216.0]
    assert not sm.shift_refusal([0, 0, 0], [0, 0, 0], [1 << 24, 0, 0], 0.1) and sm.shift_refusal([0, 0, 0], [1 << 24, 0, 0], [1, 0, 0], 0.1)
    assert sm.shift_refusal([0, 0, 0], [0, 0, 0], [0, 0, 2 ** 31 - 1], 0.1) and sm.shift_refusal([0, 0, 0], [0, 0, 0], [0, 1 << 24, 0], 1e32)


def seeded_desc(rng):
    dims = tuple(int(v) for v in rng.randint(1, 300, 3))
    return rng.uniform(-20, 20, 3).astype(F), F(rng.uniform(0.01, 0.5)), dims


def test_shift_for_equals_the_model():
    rng = np.random.RandomState(3)
    moved = stayed = 0
    for seed in range(200):
        o, vs, dims = seeded_desc(rng)
        d = binding.tsdf_desc(o, vs, dims, 0.3, 4.0)
        centre = o.astype(np.float64) + rng.uniform(-1.5, 2.5, 3) * np.asarray(dims) * float(vs)
        if seed % 5 == 0:                                                       # exactly on a voxel face, from float32 arithmetic
            centre = (o + F(rng.randint(0, 50)) * vs).astype(np.float64)
        margin = tuple(int(v) for v in rng.randint(0, 60, 3))
        got = tuple(int(v) for v in binding.tsdf_shift_for(d, centre, margin))
        want = sm.shift_for(o, vs, dims, centre, margin)
        assert got == want, (seed, got, want)
        moved += sum(1 for v in got if v)
        stayed += sum(1 for v in got if not v)
        # behind the shift the centre's voxel has index dims / 2 on every axis that moved
        o2 = sm.origin(o, got, vs)
        again = sm.shift_for(o2, vs, dims, centre, (1, 1, 1))                   # one voxel of slack: o2 is rounded to float32
        assert all(again[a] == 0 or got[a] == 0 for a in range(3)), (seed, got, again)
    assert moved > 150 and stayed > 30


def test_shift_for_refusals():
    good = binding.tsdf_desc((0, 0, 0), 0.1, (8, 8, 8), 0.2, 4.0)
    assert tuple(binding.tsdf_shift_for(good, (0.45, 0.0, 0.79), (0, 0, 0))) == (0, -4, 3)
    assert tuple(binding.tsdf_shift_for(good, (0.45, 0.0, 0.79), (0, 4, 2))) == (0, 0, 3)       # |d| == margin stays
    for centre, margin in (((np.nan, 0, 0), (0, 0, 0)), ((0, np.inf, 0), (0, 0, 0)), ((0, 0, 0), (0, -1, 0)), ((0.1 * (2 ** 24 + 6), 0, 0), (0, 0, 0)), ((0, 0, -1e300), (0, 0, 0))):
        with pytest.raises(binding.NaloError):
            binding.tsdf_shift_for(good, centre, margin)
        assert sm.shift_for((0, 0, 0), 0.1, (8, 8, 8), centre, margin) is None
    assert tuple(binding.tsdf_shift_for(binding.tsdf_desc((0, 0, 0), 1.0, (8, 8, 8), 0.2, 4.0), (2.0 ** 24 + 4.5, 0, 0), (0, 0, 0)))[0] == 2 ** 24     # d exactly 2^24 is taken
    for d in (binding.tsdf_desc((0, 0, 0), 0.1, (0, 8, 8), 0.2, 4.0), binding.tsdf_desc((0, 0, 0), 0.0, (8, 8, 8), 0.2, 4.0), binding.tsdf_desc((0, np.nan, 0), 0.1, (8, 8, 8), 0.2, 4.0),
              binding.tsdf_desc((0, 0, 0), 0.1, (8, 8, 8), -1.0, 4.0), binding.tsdf_desc((0, 0, 0), 0.1, (1024, 1024, 1024), 0.2, 4.0)):
        with pytest.raises(binding.NaloError):
            binding.tsdf_shift_for(d, (0, 0, 0), (0, 0, 0))
    L = binding.host_lib()
    out = np.full(3, 77, np.int32)
    ce, mg = np.zeros(3), np.zeros(3, np.int32)
    ip, dp = binding.c_ip, binding.c_dp
    import ctypes as C
    assert L.nalo_tsdf_shift_for(None, ce.ctypes.data_as(dp), mg.ctypes.data_as(ip), out.ctypes.data_as(ip)) == -1
    assert L.nalo_tsdf_shift_for(C.byref(good), None, mg.ctypes.data_as(ip), out.ctypes.data_as(ip)) == -1
    assert L.nalo_tsdf_shift_for(C.byref(good), ce.ctypes.data_as(dp), None, out.ctypes.data_as(ip)) == -1
    assert L.nalo_tsdf_shift_for(C.byref(good), ce.ctypes.data_as(dp), mg.ctypes.data_as(ip), None) == -1
    bad = np.array([0.0, 0.0, np.nan])
    assert L.nalo_tsdf_shift_for(C.byref(good), bad.ctypes.data_as(dp), mg.ctypes.data_as(ip), out.ctypes.data_as(ip)) == -1 and out.tolist() == [77, 77, 77]     # refused: not written


def test_shift_boxes_equals_the_model():
    rng = np.random.RandomState(5)
    counts = set()
    for seed in range(200):
        dims = tuple(int(v) for v in rng.randint(1, 40, 3))
        s = tuple(int(rng.randint(-dims[a] - 2, dims[a] + 3)) if rng.rand() < 0.8 and seed else 0 for a in range(3))
        got, want = binding.tsdf_shift_boxes(dims, s), sm.shift_boxes(dims, s)
        assert got == want, (dims, s, got, want)
        counts.add(len(got["boxes"]))
    assert counts == {0, 1, 2, 3}
    assert binding.tsdf_shift_boxes((8, 6, 4), (2, 0, -1)) == dict(boxes=[((0, 0, 0), (3, 6, 4)), ((2, 0, 2), (6, 6, 2))], kept_lo=(2, 0, 0), kept_size=(6, 6, 3))
    assert binding.tsdf_shift_boxes((8, 6, 4), (0, 0, 0)) == dict(boxes=[], kept_lo=(0, 0, 0), kept_size=(8, 6, 4))
    assert binding.tsdf_shift_boxes((8, 6, 4), (1, -6, 0)) == dict(boxes=[((0, 0, 0), (8, 6, 4))], kept_lo=(0, 0, 0), kept_size=(0, 0, 0))
    assert binding.tsdf_shift_boxes((8, 6, 4), (2 ** 31 - 1, -2 ** 31, 0))["boxes"] == [((0, 0, 0), (8, 6, 4))]
    for dims in ((0, 1, 1), (1, 2049, 1), (1, 1, -3)):
        with pytest.raises(binding.NaloError):
            binding.tsdf_shift_boxes(dims, (0, 0, 0))
    L = binding.host_lib()
    z = np.ones(3, np.int32)
    assert L.nalo_tsdf_shift_boxes(None, z.ctypes.data_as(binding.c_ip), None) == -1 and L.nalo_tsdf_shift_boxes(z.ctypes.data_as(binding.c_ip), None, None) == -1


def test_the_boxes_cells_are_disjoint_and_cover_exactly_the_lost_cells():
    """brute force on grids of 1 .. 6 voxels an axis and shifts of -8 .. 8: the cells of the boxes are pairwise disjoint and their union is the set of cells that
    do not survive; of the library's boxes and of the model's"""
    rng = np.random.RandomState(11)
    n_lost = n_multi = 0
    for seed in range(4000):
        dims = tuple(int(v) for v in rng.randint(1, 7, 3))
        s = tuple(int(v) for v in rng.randint(-8, 9, 3))
        lost = sm.lost_cells(dims, s)
        got = binding.tsdf_shift_boxes(dims, s) if seed % 4 == 0 else sm.shift_boxes(dims, s)
        seen = set()
        for lo, size in got["boxes"]:
            assert all(size[a] >= 1 and lo[a] >= 0 and lo[a] + size[a] <= dims[a] for a in range(3)), (dims, s, got)
            cells = sm.cells_of_box(lo, size)
            assert not (cells & seen), (dims, s, got)
            seen |= cells
        assert seen == lost, (dims, s, got)
        n_lost += bool(lost)
        n_multi += len(got["boxes"]) > 1 and bool(lost)
        # the kept voxels are what the model of the shift keeps
        if got["kept_size"] != (0, 0, 0):
            assert all(got["kept_lo"][a] == max(s[a], 0) and got["kept_size"][a] == dims[a] - abs(s[a]) for a in range(3))
    assert n_lost > 1000 and n_multi > 100


SAN_MAIN = r'''
#include <climits>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include "nalo_gpu.h"
static int boxes(const int* dims, int s0, int s1, int s2) {
    const int s[3] = {s0, s1, s2};
    struct nalo_tsdf_shift_boxes b;
    const int rc = nalo_tsdf_shift_boxes(dims, s, &b);
    std::printf("B %d %d\n", rc, rc == 0 ? b.n_boxes : -1);
    if (rc != 0) return 0;
    if (b.n_boxes < 0 || b.n_boxes > 3) return 1;
    for (int k = 0; k < b.n_boxes; ++k)
        for (int a = 0; a < 3; ++a) if (b.lo[k][a] < 0 || b.size[k][a] < 1 || b.lo[k][a] > dims[a] - b.size[k][a]) return 1;
    for (int a = 0; a < 3; ++a) if (b.kept_lo[a] < 0 || b.kept_size[a] < 0 || b.kept_lo[a] > dims[a] - b.kept_size[a]) return 1;
    return 0;
}
static int shift_for(const nalo_tsdf_desc& d, double x, double y, double z, int m) {
    const double c[3] = {x, y, z};
    const int margin[3] = {m, m, m};
    int s[3] = {-7, -7, -7};
    const int rc = nalo_tsdf_shift_for(&d, c, margin, s);
    std::printf("F %d %d %d %d\n", rc, s[0], s[1], s[2]);
    return rc == 0 ? 0 : (s[0] != -7 || s[1] != -7 || s[2] != -7);
}
int main() {
    int bad = 0;
    const int one[3] = {1, 1, 1}, thin[3] = {1, 2048, 1}, big[3] = {2048, 2048, 128}, zero[3] = {1, 0, 1};
    const int sh[] = {0, 1, -1, 2, 2047, 2048, -2048, INT_MAX, INT_MIN, INT_MAX - 1, INT_MIN + 1};
    for (const int* dims : {one, thin, big})
        for (int a : sh) for (int b : sh) bad += boxes(dims, a, b, 0) + boxes(dims, 0, a, b) + boxes(dims, b, a, 1);
    bad += boxes(zero, 0, 0, 0);
    nalo_tsdf_desc d1 = {{0.f, 0.f, 0.f}, 0.1f, {1, 1, 1}, 0.2f, 4.f}, tiny = {{-3e38f, 3e38f, 0.f}, 1e-30f, {2048, 1, 2048}, 1e30f, 1.f}, huge = {{0.f, 0.f, 0.f}, 3e38f, {1, 1, 1}, 1.f, 1.f};
    for (int m : {0, INT_MAX}) {
        bad += shift_for(d1, 0.05, 0.05, 0.05, m) + shift_for(d1, 1e300, -1e300, 0.0, m) + shift_for(d1, 1677721.65, -1677721.55, 0.0, m);
        bad += shift_for(tiny, 0.0, 0.0, 0.0, m) + shift_for(tiny, -3e38, 3e38, 1e-23, m) + shift_for(huge, 1e308, -1e308, 0.0, m) + shift_for(d1, NAN, 0.0, 0.0, m);
    }
    bad += shift_for(d1, 0.0, 0.0, 0.0, -1);
    nalo_tsdf_desc refused = d1; refused.dims[2] = 0;
    bad += shift_for(refused, 0.0, 0.0, 0.0, 0);
    return bad;
}
'''


def test_shift_helpers_under_the_sanitizers_on_degenerate_inputs(tmp_path):
    """nalo-slam_amd/csrc/host_tsdf.cpp is plain C++: built with a main of its own under -fsanitize=address,undefined, nalo_tsdf_shift_boxes and nalo_tsdf_shift_for
    run clean on dims of 1, shifts of INT_MIN / INT_MAX and margins of 0, every box they return lies in the grid, and a refused call writes nothing"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_shift_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(ROOT, "nalo-slam_amd", "csrc", "host_tsdf.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    rows = [line.split() for line in p.stdout.split("\n") if line]
    b, f = [r for r in rows if r[0] == "B"], [r for r in rows if r[0] == "F"]
    assert len(b) == 3 * 11 * 11 * 3 + 1 and b[-1][1] == "-1" and all(r[1] == "0" for r in b[:-1]) and {r[2] for r in b[:-1]} == {"0", "1", "2", "3"}
    assert len(f) == 16 and [r[1] for r in f[-2:]] == ["-1", "-1"] and f[0] == ["F", "0", "0", "0", "0"] and f[1][1] == "-1"
