"""tests/tsdf_raycast_model.py, the yardstick of nalo_tsdf_raycast: its two forms against each other on seeded volumes, hand cases whose numbers are exactly
representable so that the expected depths follow without rounding, one cell through every branch of the march, and the host-only nalo_tsdf_raycast_steps
against the model and under the address and undefined-behaviour sanitizers as a stand-alone program. No device."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_color_model as tcm
import tsdf_model as tm
import tsdf_raycast_model as rm
from conftest import ROOT
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth

F = np.float32


def same(a, b):
    """two results of the model (or of the device) bit for bit: a NaN equals the same NaN"""
    if set(a) != set(b):
        return False
    for k in a:
        if isinstance(a[k], np.ndarray):
            if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
                return False
        elif a[k] != b[k]:
            return False
    return True


def fused_volume(seed):
    """a small coloured volume after three integrations, then salted with NaN, infinities, -0.0 and weights on either side of 1"""
    vol = tcm.volume((-1.1, -0.9, 0.8), 0.17, (13, 11, 12), 0.4, 3.0)
    K, w, h = (20.0, 19.0, 11.5, 8.5), 24, 18
    rng = np.random.RandomState(seed)
    for it, c2w in enumerate((EYE, pose(0.2, -0.3, 0.1, (0.1, -0.2, 0.3)), pose(-0.1, 0.25, 0.0, (-0.3, 0.2, -0.1)))):
        bgr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        tcm.integrate(vol, wavy_depth(w, h, seed + it), bgr, K, c2w, 0.5, 3.0)
    salt = rng.rand(*vol["tsdf"].shape)
    vol["tsdf"][salt < 0.01] = np.nan
    vol["tsdf"][(salt > 0.01) & (salt < 0.02)] = np.inf
    vol["tsdf"][(salt > 0.02) & (salt < 0.03)] = -0.0
    vol["weight"][(salt > 0.03) & (salt < 0.05)] = np.nextafter(F(1.0), F(0.0))
    vol["colour"][:, (salt > 0.05) & (salt < 0.06)] = np.nan
    vol["colour"][:, (salt > 0.06) & (salt < 0.07)] = 300.0
    return vol


VIEWS = [(EYE, (14.0, 13.0, 7.5, 5.5)), (pose(0.15, -0.2, 0.3, (0.2, 0.1, 0.4)), (11.0, 12.0, 8.0, 6.0)), (pose(0.0, 0.1, 0.0, (0.0, 0.0, 1.6)), (9.0, 9.0, 7.5, 5.5)),
         (pose(0.0, np.pi, 0.0, (0.0, 0.0, 0.0)), (14.0, 13.0, 7.5, 5.5))]       # the third stands inside the grid, the last looks away from it


@pytest.mark.parametrize("vi", range(len(VIEWS)))
def test_vectorised_model_equals_the_literal_one(vi):
    c2w, K = VIEWS[vi]
    vol = fused_volume(3 + vi)
    hits = 0
    for normals, colour in ((False, False), (True, True)):
        a = rm.raycast_literal(vol, 16, 12, K, c2w, 0.3, 3.2, 0.06, 1.0, normals, colour)
        b = rm.raycast(vol, 16, 12, K, c2w, 0.3, 3.2, 0.06, 1.0, normals, colour)
        assert same(a, b), (vi, normals, colour)
        hits = a["n_hit"]
        assert a["n_steps"] == 49 and (a["depth"] > 0).sum() == a["n_hit"] - int(np.isnan(a["depth"]).sum())
    assert (hits == 0) == (vi == 3) and (vi == 3 or hits > 40)
    if vi == 0:
        assert 0 < b["n_normal"] <= b["n_hit"] and b["rgba"][..., 3].max() == 255 and b["n_back"] >= 0


def test_steps_equal_the_model_and_refuse_4097():
    cases = [(0.5, 2.5, 0.125), (0.5, 0.5, 0.125), (0.0, 1.0, 0.1), (0.3, 3.2, 0.06), (0.0, 4095.0, 1.0), (0.0, 4095.5, 1.0), (1000.0, 1000.1, 1e-6 * 64), (0.0, 1.0, 3e38), (0.25, 3e38, 1e35),
             (0.0, 0.0, 1e-45), (0.1, 0.7, 0.1), (0.1, np.nextafter(F(0.1) + F(6.0) * F(0.1), F(0)), 0.1)]
    for mn, mx, st in cases:
        assert binding.tsdf_raycast_steps(mn, mx, st) == rm.steps(mn, mx, st), (mn, mx, st)
    assert binding.tsdf_raycast_steps(0.5, 2.5, 0.125) == 17                    # max_depth exactly on sample 16: it counts
    assert binding.tsdf_raycast_steps(0.5, np.nextafter(F(2.5), F(0)), 0.125) == 16 and binding.tsdf_raycast_steps(0.5, 0.5, 0.125) == 1
    assert binding.tsdf_raycast_steps(0.0, 4095.0, 1.0) == 4096 and rm.steps(0.0, 4096.0, 1.0) == 4097
    for bad in ((0.0, 4096.0, 1.0), (0.0, 1.0, 1e-6), (-0.1, 1.0, 0.1), (2.0, 1.0, 0.1), (0.0, 1.0, 0.0), (0.0, 1.0, -0.1), (np.nan, 1.0, 0.1), (0.0, np.inf, 0.1), (0.0, 1.0, np.nan),
                (0.0, 1.0, np.inf)):
        with pytest.raises(binding.NaloError):
            binding.tsdf_raycast_steps(*bad)
    assert "nalo_tsdf_raycast" in binding.EXPORTS and "nalo_tsdf_raycast_view" in binding.EXPORTS and hasattr(binding.host_lib(), "nalo_tsdf_raycast")
    assert callable(binding.Context.tsdf_raycast) and callable(binding.Context.tsdf_raycast_view)


def plane_volume(z0):
    """voxel centres on multiples of 0.25 (x, y: -1.5 .. 1.5, z: 0.5 .. 2.75); tsdf = z0 - z of the centre: linear in z with its zero on the plane z = z0"""
    vol = tcm.volume((-1.625, -1.625, 0.375), 0.25, (13, 13, 10), 0.5, 4.0)
    zc = tm.centres(vol)[2]
    vol["tsdf"][:] = (F(z0) - zc)[:, None, None]
    vol["weight"][:] = 1.0
    return vol


def test_hand_case_with_exactly_representable_numbers():
    """identity pose, K = (8, 8, 3.5, 2.5) on 8 x 6: rx and ry are multiples of 1/16, the samples lie at multiples of 1/8, so p, q, the fractions and S = z0 - z
    are all exact. z0 = 1.3125 lies half way between the samples 1.25 and 1.375: s = 0.0625 / 0.125 = 0.5 and depth = 1.25 + 0.125 * 0.5 for every pixel."""
    vol = plane_volume(1.3125)
    for fn in (rm.raycast, rm.raycast_literal):
        r = fn(vol, 8, 6, (8.0, 8.0, 3.5, 2.5), EYE, 0.5, 2.5, 0.125, 1.0, True, False)
        assert r["n_steps"] == 17 and (r["depth"] == F(1.3125)).all()
        assert (r["normal"] == np.array([0.0, 0.0, -1.0], F)).all()               # G = (0, 0, -0.25 - 0.25), len 0.5: towards the camera
        assert (r["n_hit"], r["n_back"], r["n_normal"]) == (48, 0, 48)
    # the zero exactly on a sample: S_{n-1} = 0.125, S_n = 0 is no crossing (0 is outside), S_n = 0, S_{n+1} = -0.125 is one with s = 0
    r = rm.raycast(plane_volume(1.375), 8, 6, (8.0, 8.0, 3.5, 2.5), EYE, 0.5, 2.5, 0.125, 1.0)
    assert (r["depth"] == F(1.375)).all() and r["n_hit"] == 48
    # the camera moved back by 0.25 sees the same plane 0.25 further away; a max_depth one sample short of the crossing's far end misses everywhere
    r = rm.raycast(plane_volume(1.3125), 8, 6, (8.0, 8.0, 3.5, 2.5), pose(0, 0, 0, (0, 0, -0.25)), 0.5, 2.5, 0.125, 1.0)
    assert (r["depth"] == F(1.5625)).all()
    r = rm.raycast(plane_volume(1.3125), 8, 6, (8.0, 8.0, 3.5, 2.5), EYE, 0.5, 1.25, 0.125, 1.0)
    assert r["n_steps"] == 7 and r["n_hit"] == 0 and not r["depth"].any()
    # seen from behind (the camera beyond the plane, turned round): every ray meets the back face first
    r = rm.raycast(plane_volume(1.3125), 8, 6, (8.0, 8.0, 3.5, 2.5), pose(0, np.pi, 0, (0, 0, 2.75)), 0.5, 2.5, 0.125, 1.0, True)
    assert (r["n_hit"], r["n_back"], r["n_normal"]) == (0, 48, 0) and not r["depth"].any() and not r["normal"].any()


def cell(planes, weight=None):
    """a 2 x 2 x len(planes) grid around the z axis (centres x, y = -0.125, 0.125; z = 0.5, 0.75, ..) whose z plane k holds planes[k] at all four voxels"""
    vol = tcm.volume((-0.25, -0.25, 0.375), 0.25, (2, 2, len(planes)), 0.5, 4.0)
    vol["tsdf"][:] = np.asarray(planes, F)[:, None, None]
    vol["weight"][:] = 1.0 if weight is None else weight
    return vol


def axis_ray(vol, max_depth=1.5, normals=False):
    """one pixel whose ray is the z axis: q = (0.5, 0.5, (z - 0.375) / 0.25 - 0.5), samples every 0.0625 from 0.5: q_z = 0, 0.25, 0.5, 0.75 in the first cell"""
    a = rm.raycast(vol, 1, 1, (8.0, 8.0, 0.0, 0.0), EYE, 0.5, max_depth, 0.0625, 1.0, normals)
    b = rm.raycast_literal(vol, 1, 1, (8.0, 8.0, 0.0, 0.0), EYE, 0.5, max_depth, 0.0625, 1.0, normals)
    assert same(a, b)
    return a["depth"][0, 0], (a["n_hit"], a["n_back"])


def test_one_cell_by_hand_through_every_branch():
    # S = 0.375, 0.125, -0.125, -0.375: the front face between samples 1 and 2, s = 0.125 / 0.25, depth = 0.5625 + 0.0625 * 0.5
    assert axis_ray(cell([0.375, -0.625])) == (F(0.59375), (1, 0))
    # past the cell (q_z = 1 at z = 0.75) every sample is invalid: a crossing between the last valid sample and the first invalid one is none
    assert axis_ray(cell([0.875, -0.125])) == (F(0.0), (0, 0))                # S = 0.875, 0.625, 0.375, 0.125: no sign change inside the cell
    # an invalid corner (weight just below min_weight), a NaN corner, a NaN weight: no sample of the cell is valid
    for wgt, tv in ((np.nextafter(F(1.0), F(0.0)), None), (None, np.nan), (np.nan, None)):
        vol = cell([0.375, -0.625])
        if wgt is not None:
            vol["weight"][1, 1, 0] = wgt
        if tv is not None:
            vol["tsdf"][0, 1, 1] = tv
        assert axis_ray(vol) == (F(0.0), (0, 0))
    # an infinite corner: a = inf + 0.5 * (inf - inf) is NaN
    vol = cell([0.375, -0.625])
    vol["tsdf"][0, 0, 0] = np.inf
    assert axis_ray(vol) == (F(0.0), (0, 0))
    # a plane of -0.0f is outside like one of 0.0f (the interpolation along x already turns it into 0.0f): S = 0, -0.25, ..: a hit at n = 1 with s = 0
    assert axis_ray(cell([-0.0, -1.0])) == (F(0.5), (1, 0))
    assert axis_ray(cell([0.0, -1.0])) == (F(0.5), (1, 0))
    # a ray that starts inside and stays inside: a miss, and no back face either
    assert axis_ray(cell([-0.5, -1.0])) == (F(0.0), (0, 0))
    # a ray that starts inside and leaves: the back face ends it
    assert axis_ray(cell([-0.5, 0.5])) == (F(0.0), (0, 1))
    # a back face in front of a front face (two cells: -0.5, 0.5, -0.5): the ray ends at the back face, the front face behind it is never reached
    assert axis_ray(cell([-0.5, 0.5, -0.5])) == (F(0.0), (0, 1))
    assert axis_ray(cell([0.5, 0.5, -0.5])) == (F(0.875), (1, 0))               # the same front face alone: S = 0.5, 0.25, 0, -0.25 in the second cell, s = 0 / 0.25
    # N = 1 and N = 2: one sample is no pair; two samples whose signs differ are one
    assert axis_ray(cell([0.125, -0.875]), max_depth=0.5) == (F(0.0), (0, 0))
    assert axis_ray(cell([0.125, -0.875]), max_depth=0.5625) == (F(0.53125), (1, 0))   # S = 0.125, -0.125
    # the normal needs its six neighbours: in a single cell q* +- 1 leaves the grid, the normal is zero and the pixel stays a hit
    r = rm.raycast(cell([0.375, -0.625]), 1, 1, (8.0, 8.0, 0.0, 0.0), EYE, 0.5, 1.5, 0.0625, 1.0, True)
    assert (r["n_hit"], r["n_normal"]) == (1, 0) and not r["normal"].any()


SAN_MAIN = r'''
#include <cmath>
#include <cstdio>
#include "nalo_gpu.h"
static int run(float mn, float mx, float st) {
    int n = -7;
    const int rc = nalo_tsdf_raycast_steps(mn, mx, st, &n);
    std::printf("%d %d\n", rc, n);
    return (rc == 0) != (n >= 1 && n <= 4096) || (rc != 0 && n != 0);
}
int main() {
    int bad = 0;
    bad += run(0.5f, 2.5f, 0.125f) + run(0.f, 4095.f, 1.f) + run(0.f, 4096.f, 1.f) + run(0.f, 3e38f, 3e38f) + run(0.f, 3.4e38f, 1e35f) + run(3e38f, 3.4e38f, 3e38f);
    bad += run(0.f, 0.f, 1e-45f) + run(0.f, 1e-40f, 1e-45f) + run(-0.f, 0.f, 1.f) + run(1e30f, 1e30f, 1e-30f) + run(1.f, 2.f, 1e-30f);
    bad += run(NAN, 1.f, 1.f) + run(0.f, NAN, 1.f) + run(0.f, 1.f, NAN) + run(INFINITY, INFINITY, 1.f) + run(0.f, INFINITY, 1.f) + run(0.f, 1.f, INFINITY);
    bad += run(-1.f, 1.f, 1.f) + run(2.f, 1.f, 1.f) + run(0.f, 1.f, 0.f) + run(0.f, 1.f, -1.f);
    bad += nalo_tsdf_raycast_steps(0.f, 1.f, 1.f, nullptr) != NALO_ERR_ARG;
    return bad;
}
'''


def test_raycast_steps_under_the_sanitizers_on_degenerate_inputs(tmp_path):
    """nalo-slam_amd/csrc/host_tsdf.cpp is plain C++: built with a main of its own under -fsanitize=address,undefined it counts the samples of step sizes from
    a denormal to one that overflows, refuses what is not finite, and answers 1 .. 4096 or a refusal with 0"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_steps_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(ROOT, "nalo-slam_amd", "csrc", "host_tsdf.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    rows = [[int(v) for v in line.split()] for line in p.stdout.split("\n") if line]
    assert len(rows) == 21 and rows[0] == [0, 17] and rows[1] == [0, 4096] and rows[2] == [-1, 0] and [r[0] for r in rows[11:]] == [-1] * 10
