"""tests/tsdf_align_model.py against itself and by hand, and nalo_tsdf_align_step (nalo-slam_amd/csrc/host_tsdf.cpp, host only) against numpy and the model's
step. No device."""
import functools
import os
import subprocess

import numpy as np
import pytest

import tsdf_align_model as am
import tsdf_mesh_model as mm
import tsdf_model as tm
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth
from test_tsdf_raycast_cpu import plane_volume

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the fused volumes of tests/test_tsdf_gpu.py: its plane size, K, poses and grids
W0, H0, K0 = 64, 48, (70.0, 68.0, 31.5, 23.5)
POSES = [EYE, pose(0.15, -0.25, 0.1, (0.2, -0.1, 0.15)), pose(-0.3, 0.35, 1.2, (-0.25, 0.2, -0.1))]
GRIDS = [dict(origin=(-1.2, -0.9, 0.9), vs=0.075, dims=(32, 24, 40), trunc=0.25, mw=4.0), dict(origin=(-0.7, -0.5, 1.85), vs=0.055, dims=(33, 17, 5), trunc=0.2, mw=4.0)]
K86 = (8.0, 8.0, 3.5, 2.5)                                                      # the hand cases' plane: 8 x 6, rx and ry multiples of 1 / 16


@functools.lru_cache(maxsize=None)
def fused_model(gi):
    """grid gi after the three poses, twice, as test_tsdf_gpu.py's fixture fuses it: the model's volume, shared and never written"""
    g = GRIDS[gi]
    vol = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    for rnd in range(2):
        for pi, c2w in enumerate(POSES):
            tm.integrate(vol, wavy_depth(W0, H0, 10 * gi + pi, base=2.0 + 0.02 * rnd), K0, c2w, 0.5, 3.5)
    for a in (vol["tsdf"], vol["weight"]):
        a.setflags(write=False)
    return vol


def test_exports():
    L = binding.host_lib()
    for s in ("nalo_tsdf_align_eval", "nalo_tsdf_align_depth", "nalo_tsdf_align_frame", "nalo_tsdf_align_step"):
        assert s in binding.EXPORTS and hasattr(L, s), s


@pytest.mark.parametrize("gi,pi,step,dof,s", [(0, 0, 1, 6, 1.0), (0, 1, 2, 7, 1.03), (1, 2, 1, 7, 0.97), (1, 0, 5, 6, 1.0)])
def test_vectorised_model_equals_the_literal_one(gi, pi, step, dof, s):
    vol = fused_model(gi)
    depth = wavy_depth(W0, H0, 10 * gi + pi, base=2.01)
    a = am.records(vol, depth, K0, POSES[pi], s, 0.5, 3.5, 1.0, 0.02, step, dof)
    b = am.records_literal(vol, depth, K0, POSES[pi], s, 0.5, 3.5, 1.0, 0.02, step, dof)
    assert mm.same_floats(a, b)
    cnt = am.sums(a, 0.02, step)["count"]
    assert cnt[0] > (50, 5)[gi] and cnt[1] > 0 and cnt[2] > 0, cnt               # not vacuous: used (the thin grid is five voxels deep, the gradient needs four), holes in the depth, pixels off the data
    assert np.isnan(a[1::2, :, :]).all() if step == 2 else True                 # the words of pixels that are not visited keep the fill
    used = a[::step, ::step][a[::step, ::step, 9] == 0]
    assert gi == 1 or ((used[:, 1] < 1).any() and (used[:, 1] == 1).any())      # both Huber branches


def hand(D, huber=0.125, dof=7, z0=1.3125, u=0, v=0, c2w=EYE, s=1.0, vol=None):
    depth = np.zeros((6, 8), F)
    depth[v, u] = D
    vol = plane_volume(z0) if vol is None else vol
    a = am.records_literal(vol, depth, K86, c2w, s, 0.5, 3.0, 1.0, huber, 1, dof, pixels=[(u, v)])[v, u]
    b = am.records(vol, depth, K86, c2w, s, 0.5, 3.0, 1.0, huber, 1, dof)[v, u]
    assert mm.same_floats(a, b)
    return a


def test_one_pixel_by_hand_through_every_state_and_both_huber_branches():
    """plane_volume: tsdf = z0 - z, linear, voxel size 0.25, centres on multiples of 0.25. Identity pose, pixel (0, 0) of the 8 x 6 plane: rx = -0.4375,
    ry = -0.3125. D = 1.25: pw = (-0.546875, -0.390625, 1.25), every number exact; S = z0 - D = 0.0625; G = (0, 0, -0.5), g = G * (0.5 / 0.25) = (0, 0, -1);
    pw x g = (pw_y g_z - pw_z g_y, pw_z g_x - pw_x g_z, 0) = (0.390625, -0.546875, 0); g . (pw - 0) = -1.25."""
    want = np.array([0.0625, 1.0, 0, 0, -1, 0.390625, -0.546875, 0, -1.25, 0], F)
    assert (hand(1.25) == want).all()
    want6 = want.copy()
    want6[8] = 0
    assert (hand(1.25, dof=6) == want6).all()                                  # the seventh entry exists only for dof = 7
    wanth = want.copy()
    wanth[1] = 0.5
    assert (hand(1.25, huber=0.03125) == wanth).all()                           # |r| above huber: hw = 0.03125 / 0.0625
    assert hand(1.25, huber=0.0625)[1] == 1                                     # |r| exactly at huber: inside
    assert (hand(1.3125)[:2] == np.array([0.0, 1.0], F)).all()                  # r exactly 0
    # states: no depth (0 below min_depth, NaN, above max_depth), q outside the cells (z = 3: q_z = 10 > dims - 2), q_z = 8 valid but q_z + 1 not
    for D, st in ((0.0, 1), (np.nan, 1), (3.25, 1), (np.inf, 1), (3.0, 2), (2.5, 3), (0.5, 3), (0.75, 0), (2.25, 0)):
        rec = hand(D)
        assert rec[9] == st and (st == 0 or not rec[:9].any()), (D, rec)
    # a translation and a scale move the point: t = (0, 0, 0.25), s = 2, D = 0.5: pw = (2 * -0.21875, 2 * -0.15625, 1.25), J6 = g . (pw - t) = -1
    rec = hand(0.5, c2w=pose(0, 0, 0, (0, 0, 0.25)), s=2.0)
    assert (rec == np.array([0.0625, 1.0, 0, 0, -1, 0.3125, -0.4375, 0, -1.0, 0], F)).all()
    # the sums of one record: H = Jw J^T, b = Jw r, E = rho in both branches
    S = am.sums(hand(1.25, huber=0.03125)[None, None], 0.03125)
    J = wanth[2:9].astype(np.float64)
    assert (am.full(S["H"]) == 0.5 * np.outer(J, J)).all() and (S["b"] == 0.5 * J * 0.0625).all()
    assert S["E"] == 0.03125 * (2 * 0.0625 - 0.03125) and S["rr"] == 0.0625 ** 2 and S["count"] == (1, 0, 0, 0)
    assert am.sums(hand(1.25)[None, None], 0.125)["E"] == 0.0625 ** 2


def spd(rng, scale=1.0):
    A = rng.randn(12, 7)
    H = A.T @ A * scale
    return np.array([H[i, j] for i, j in am.PAIRS]), rng.randn(7) * scale


@pytest.mark.parametrize("dof", [6, 7])
def test_align_step_against_numpy_and_the_models_update(dof):
    rng = np.random.RandomState(7 + dof)
    for k in range(200):
        H28, b = spd(rng, 10.0 ** rng.uniform(-3, 6))
        lam = [0.0, 0.01, 4.0, 1e3][k % 4]
        T, s = pose(*rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3)), float(np.exp(rng.uniform(-0.2, 0.2)))
        inc, Tn, sn = binding.tsdf_align_step(H28, b, lam, dof, T, s)
        H = am.full(H28)[:dof, :dof]
        ref = np.linalg.solve(H + lam * np.diag(np.diag(H)), -b[:dof])
        assert np.abs(inc[:dof] - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-300) * np.linalg.cond(H) ** 0.5 and (dof == 7 or inc[6] == 0), (k, inc, ref)
        m_inc, m_T, m_s = am.step(H28, b, lam, dof, T, s)
        # the model's update from the LIBRARY's increment: what is compared is exp and the product, to a few ulps of entries of magnitude <= |t| + |inc|
        E = am.se3_exp(inc[:6])
        want = np.hstack([E[:, :3] @ T[:, :3], (E[:, :3] @ T[:, 3] + E[:, 3])[:, None]])
        assert np.abs(Tn - want).max() <= 1e-13 * (1 + np.abs(want).max() + np.abs(inc).max() ** 2), (k, np.abs(Tn - want).max())
        assert abs(sn - s * np.exp(inc[6])) <= 1e-15 * sn and (dof == 7 or sn == s)
        assert np.abs(m_T - Tn).max() <= 1e-6 * (1 + np.abs(Tn).max()) and abs(m_s - sn) <= 1e-6 * sn
        assert np.abs(Tn[:, :3] @ Tn[:, :3].T - np.eye(3)).max() < 1e-12           # still a rotation


def test_align_step_refusals():
    rng = np.random.RandomState(3)
    H28, b = spd(rng)
    ok = lambda **k: binding.tsdf_align_step(k.get("H", H28), k.get("b", b), k.get("lam", 0.01), k.get("dof", 7), k.get("T", EYE), k.get("s", 1.0))
    ok()
    bad = H28.copy(); bad[3] = np.nan
    neg = H28.copy(); neg[0] = -1.0                                              # H[0][0] < 0: not positive definite
    sing = np.zeros(28)
    low = np.array([(1.0 if i < 6 else 0.0) * (i == j) for i, j in am.PAIRS])    # H[6][6] = 0: good for dof 6, singular for dof 7
    bnan = b.copy(); bnan[2] = np.inf
    Tn = EYE.copy(); Tn[1, 3] = np.nan
    for kw in (dict(H=bad), dict(H=neg), dict(H=sing), dict(H=low), dict(b=bnan), dict(lam=-1.0), dict(lam=np.nan), dict(lam=np.inf), dict(dof=5), dict(dof=8), dict(T=Tn),
               dict(s=0.0), dict(s=-1.0), dict(s=np.nan), dict(H=H28 * 1e300, lam=1e300)):
        with pytest.raises(binding.NaloError):
            ok(**kw)
    inc, _, s = ok(H=low, dof=6)
    assert inc[6] == 0 and s == 1.0
    # a refusal writes nothing
    import ctypes as C
    e, out, incb = binding.tsdf_align_est(EYE), binding.tsdf_align_est(EYE * 5, 9.0), np.full(7, 77.0)
    assert binding.host_lib().nalo_tsdf_align_step(sing.ctypes.data_as(binding.c_dp), b.ctypes.data_as(binding.c_dp), C.c_double(0.01), 7, C.byref(e), incb.ctypes.data_as(binding.c_dp), C.byref(out)) == -1
    assert (incb == 77.0).all() and out.s == 9.0 and out.camToWorld[0] == 5.0
    assert binding.host_lib().nalo_tsdf_align_step(None, None, C.c_double(0.01), 7, None, None, None) == -1


SAN_MAIN = r'''
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "nalo_gpu.h"
int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    nalo_tsdf_align_est e{}, out{};
    e.camToWorld[0] = e.camToWorld[5] = e.camToWorld[10] = 1.0; e.s = 1.0;
    double H[28], b[7], inc[7];
    const double fill[] = {0.0, nan, inf, -inf, 1e300, -1e300, 1e-320, 1.0};
    for (double hv : fill)
        for (double bv : fill)
            for (int dof = 5; dof <= 8; ++dof)
                for (double lam : {0.0, 0.01, 1e300, nan, -1.0}) {
                    for (int i = 0; i < 28; ++i) H[i] = hv;
                    for (int i = 0; i < 7; ++i) b[i] = bv;
                    const int all = nalo_tsdf_align_step(H, b, lam, dof, &e, inc, &out);                 // every entry equal: singular
                    for (int i = 0, k = 0; i < 7; ++i) for (int j = i; j < 7; ++j, ++k) H[k] = i == j ? hv : 0.0;
                    const int diag = nalo_tsdf_align_step(H, b, lam, dof, &e, inc, &out);                // diagonal: positive definite iff hv > 0
                    std::printf("%d %d\n", all, diag);
                    if (diag == 0) for (int i = 0; i < 7; ++i) if (!std::isfinite(inc[i])) return 2;
                }
    // 1e300 everywhere it can go: the estimate, and an increment whose exp overflows
    for (int i = 0; i < 12; ++i) e.camToWorld[i] = 1e300;
    for (int i = 0, k = 0; i < 7; ++i) for (int j = i; j < 7; ++j, ++k) H[k] = i == j ? 1e-300 : 0.0;
    for (int i = 0; i < 7; ++i) b[i] = -1e300;
    std::printf("%d\n", nalo_tsdf_align_step(H, b, 0.0, 7, &e, inc, &out));
    e.s = 1e300;
    std::printf("%d\n", nalo_tsdf_align_step(H, b, 0.0, 7, &e, inc, &out));
    return 0;
}
'''


def test_align_step_under_the_sanitizers_on_degenerate_inputs(tmp_path):
    """nalo-slam_amd/csrc/host_tsdf.cpp is plain C++: built with a main of its own under -fsanitize=address,undefined, nalo_tsdf_align_step runs clean on
    singular, NaN, infinite, denormal and 1e300 systems, refuses all but the positive definite finite ones, and never hands out an increment that is not finite"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_align_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(ROOT, "nalo-slam_amd", "csrc", "host_tsdf.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    rows = [[int(v) for v in line.split()] for line in p.stdout.split("\n") if line]
    assert len(rows) == 8 * 8 * 4 * 5 + 2
    assert all(r[0] == -1 for r in rows[:-2:5])                                # lambda = 0 (every fifth row): a matrix of equal entries is not positive definite
    assert any(r[1] == 0 for r in rows[:-2]) and sum(r[1] == 0 for r in rows[:-2]) < len(rows) // 4
    assert rows[-2:] == [[-1], [-1]]


# ------------------------------------------------------------------------------------------------ the loop's scene (tests/test_tsdf_align_gpu.py runs it on the device)
CW, CH, CK = 96, 72, (80.0, 80.0, 47.5, 35.5)
LOOP = dict(min_depth=0.2, max_depth=4.0, min_weight=1.0, huber=0.25, step=1)


def corner_volume():
    """48 x 48 x 48 voxels of 0.05 around the origin; three orthogonal planes x = 0.6, y = 0.6, z = 0.6, the room on their low side: tsdf = clip(min(0.6 - x,
    0.6 - y, 0.6 - z) / trunc, -1, 1) at the voxel centres, every weight 1"""
    vol = tm.volume((-1.2, -1.2, -1.2), 0.05, (48, 48, 48), 0.2, 4.0)
    cx, cy, cz = tm.centres(vol)
    sdf = np.minimum(np.minimum((F(0.6) - cx)[None, None, :], (F(0.6) - cy)[None, :, None]), (F(0.6) - cz)[:, None, None])
    vol["tsdf"][:] = np.clip(sdf / vol["trunc"], F(-1), F(1))
    vol["weight"][:] = 1.0
    return vol


def look(eye, at):
    z = np.asarray(at, np.float64) - np.asarray(eye, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.hstack([np.stack([x, np.cross(z, x), z], 1), np.asarray(eye, np.float64)[:, None]])


def compose(xi, T):
    E = am.se3_exp(xi)
    return np.hstack([E[:, :3] @ T[:, :3], (E[:, :3] @ T[:, 3] + E[:, 3])[:, None]])


CORNER_TRUE = look((-0.5, -0.4, -0.6), (0.6, 0.6, 0.6))                          # in the room, looking into the corner: all three planes in view
DEG = np.pi / 180
CORNER_START = compose([0.06, -0.05, 0.06, 0.6 * DEG, -0.64 * DEG, 0.48 * DEG], CORNER_TRUE)      # 0.0986 off (two voxels) and one degree


def pose_error(T, s, true=CORNER_TRUE):
    """(distance of the camera centres, angle between the rotations in degrees, |s - 1|)"""
    dR = T[:, :3] @ true[:, :3].T
    return float(np.linalg.norm(T[:, 3] - true[:, 3])), float(np.degrees(np.arccos(min(1.0, (np.trace(dR) - 1) / 2)))), abs(s - 1.0)


@functools.lru_cache(maxsize=None)
def corner_model(dof):
    """the model's loop on the corner scene from CORNER_START (3 % off in scale for dof = 7), twelve iterations: (volume, depth plane, result)"""
    import tsdf_raycast_model as rm
    vol = corner_volume()
    depth = rm.raycast(vol, CW, CH, CK, CORNER_TRUE, 0.2, 4.0, 0.02, 1.0)["depth"]
    return vol, depth, am.align(vol, depth, CK, CORNER_START, 1.03 if dof == 7 else 1.0, step_px=LOOP["step"], dof=dof, max_iterations=12, min_used=100, lambda0=0.0, eps=1e-7,
                                **{k: LOOP[k] for k in ("min_depth", "max_depth", "min_weight", "huber")})


def test_model_loop_on_the_corner_scene():
    """dof = 6 ends within 3e-5 of the true camera centre and 0.0012 degrees of its rotation (the ray-cast's own interpolation error; measured 2.54e-5 and
    0.00111). dof = 7 cannot end near it: three planes through one point are unchanged by a scaling about that point, so scale and translation are free
    along one direction and only the residual says that the loop works - it falls by five orders of magnitude."""
    vol, depth, r = corner_model(6)
    assert (depth > 0).sum() == CW * CH and r["n_first"] == CW * CH
    e = pose_error(r["cam_to_world"], r["s"])
    assert r["status"] == am.CONVERGED and e[0] < 3e-5 and e[1] < 1.2e-3 and r["s"] == 1.0, (r["status"], e)
    assert pose_error(CORNER_START, 1.0)[0] > 0.098 and abs(pose_error(CORNER_START, 1.0)[1] - 1.0) < 1e-6
    for dof in (6, 7):
        r = corner_model(dof)[2]
        per = [t["E"] / t["count"][0] for t in r["trace"] if t["accepted"]]
        assert all(b < a for a, b in zip(per, per[1:])) and per[-1] < 1e-4 * per[0], (dof, per)
