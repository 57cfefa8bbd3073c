"""tests/tsdf_model.py on hand-worked inputs, its two forms against each other, and the host-only half of the TSDF section (nalo_tsdf_frustum_box) against the
model and under the address and undefined-behaviour sanitizers as a stand-alone program. No device."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_model as tm
from conftest import ROOT
from nalo_slam_amd import binding

F = np.float32
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def pose(rx, ry, rz, t):
    return np.concatenate([rot(rx, ry, rz), np.asarray(t, np.float64).reshape(3, 1)], 1)


def wavy_depth(w, h, seed, base=2.0):
    rng = np.random.RandomState(seed)
    v, u = np.mgrid[0:h, 0:w]
    d = base + 0.4 * np.sin(u * 0.3) * np.cos(v * 0.2) + 0.05 * rng.rand(h, w)
    d[rng.rand(h, w) < 0.05] = 0.0
    return d.astype(F)


def desc_of(vol):
    return binding.tsdf_desc(vol["origin"], vol["vs"], vol["dims"], vol["trunc"], vol["max_weight"])


def test_exports_and_entry_points():
    for s in ("nalo_tsdf_create", "nalo_tsdf_reset", "nalo_tsdf_destroy", "nalo_tsdf_integrate_depth", "nalo_tsdf_release", "nalo_tsdf_integrate_frame", "nalo_tsdf_last",
              "nalo_tsdf_get", "nalo_tsdf_set", "nalo_tsdf_view", "nalo_tsdf_surface_points", "nalo_tsdf_frustum_box"):
        assert s in binding.EXPORTS and hasattr(binding.host_lib(), s)
    for m in ("tsdf_create", "tsdf_reset", "tsdf_integrate_depth", "tsdf_integrate_frame", "tsdf_last", "tsdf_get", "tsdf_set", "tsdf_surface_points", "tsdf_view"):
        assert callable(getattr(binding.Context, m))


@pytest.mark.parametrize("c2w", [EYE, pose(0.2, -0.3, 0.1, (0.1, -0.2, 0.3)), pose(-0.4, 0.5, 2.0, (-0.3, 0.2, -0.1))])
def test_vectorised_model_equals_the_literal_one(c2w):
    K, w, h = (20.0, 19.0, 11.5, 8.5), 24, 18
    depth = wavy_depth(w, h, 3)
    a, b = (tm.volume((-1.1, -0.9, 0.8), 0.17, (13, 11, 12), 0.4, 3.0) for _ in range(2))
    for it in range(3):                                                        # a second and third pass run the weighted average on w0 > 0
        n, code = tm.integrate_literal(a, depth + F(0.03 * it), K, c2w, 0.5, 3.0)
        r = tm.integrate(b, depth + F(0.03 * it), K, c2w, 0.5, 3.0)
        assert n == r["updated"] and n > 50 and np.array_equal(code, r["code"])
        assert a["tsdf"].tobytes() == b["tsdf"].tobytes() and a["weight"].tobytes() == b["weight"].tobytes()
    assert {tm.UPDATED, tm.OUTSIDE, tm.NO_DEPTH, tm.OCCLUDED} <= set(np.unique(r["code"]).tolist())
    assert np.array_equal(tm.surface_points_literal(a, 1.0), tm.surface_points(b, 1.0)) and len(tm.surface_points(b, 1.0)) > 10


def one_voxel(depth_value, c2w=EYE, K=(10.0, 10.0, 8.0, 6.0), vol=None, min_depth=0.5, max_depth=4.0, at=(8, 6)):
    """a 1x1x1 grid whose voxel centre is (0, 0, 2): at the identity it projects to uf = 8.5, vf = 6.5, pixel (8, 6)"""
    vol = vol or tm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, 2.0)
    depth = np.full((12, 16), 9.0, F)
    depth[at[1], at[0]] = depth_value
    twin = dict(vol, tsdf=vol["tsdf"].copy(), weight=vol["weight"].copy())
    r = tm.integrate(vol, depth, K, c2w, min_depth, max_depth)
    n, code = tm.integrate_literal(twin, depth, K, c2w, min_depth, max_depth)
    assert n == r["updated"] and np.array_equal(code, r["code"]) and twin["tsdf"].tobytes() == vol["tsdf"].tobytes() and twin["weight"].tobytes() == vol["weight"].tobytes()
    return vol, r, int(r["code"][0, 0, 0])


def test_one_voxel_by_hand_through_every_branch():
    vol, r, code = one_voxel(2.25)
    assert (r["uf"][0, 0, 0], r["vf"][0, 0, 0], r["zc"][0, 0, 0]) == (8.5, 6.5, 2.0) and code == tm.UPDATED
    assert (vol["tsdf"][0, 0, 0], vol["weight"][0, 0, 0]) == (0.5, 1.0)                    # sdf 0.25 / trunc 0.5
    one_voxel(2.0, vol=vol)
    assert (vol["tsdf"][0, 0, 0], vol["weight"][0, 0, 0]) == (0.25, 2.0)                   # (0.5 * 1 + 0) / 2
    one_voxel(3.0, vol=vol)
    assert (vol["tsdf"][0, 0, 0], vol["weight"][0, 0, 0]) == (0.5, 2.0)                    # d = min(1, 2) = 1: (0.25 * 2 + 1) / 3; the weight saturates at 2
    before = (vol["tsdf"].copy(), vol["weight"].copy())
    for dv, want in ((1.4, tm.OCCLUDED), (0.0, tm.NO_DEPTH), (-1.0, tm.NO_DEPTH), (np.nan, tm.NO_DEPTH), (np.inf, tm.NO_DEPTH), (4.5, tm.NO_DEPTH), (0.25, tm.NO_DEPTH)):
        assert one_voxel(dv, vol=vol)[2] == want
    assert one_voxel(2.0, c2w=pose(0, np.pi, 0, (0, 0, 0)), vol=vol)[2] == tm.BEHIND      # the camera looks away
    assert one_voxel(2.0, c2w=pose(0, 0, 0, (0, 0, 2.0)), vol=vol)[2] == tm.BEHIND        # zc exactly 0
    assert one_voxel(2.0, c2w=pose(0, 0, 0, (3.0, 0, 0)), vol=vol)[2] == tm.OUTSIDE       # uf = 10 * (-3 / 2) + 8.5 < 0
    assert (vol["tsdf"].tobytes(), vol["weight"].tobytes()) == (before[0].tobytes(), before[1].tobytes())
    assert one_voxel(2.0, K=(10.0, 10.0, -0.5, 6.0), vol=vol, at=(0, 6))[2] == tm.UPDATED  # uf exactly 0 is inside ...
    vol2 = tm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, 2.0)
    assert one_voxel(2.0, K=(10.0, 10.0, 15.5, 6.0), vol=vol2)[2] == tm.OUTSIDE           # ... and uf exactly w is not
    assert vol2["weight"][0, 0, 0] == 0 and vol2["tsdf"][0, 0, 0] == 1
    # the two ends of the truncation band: sdf == -trunc is integrated (d = -1), sdf == trunc gives d = 1
    v3, _, c3 = one_voxel(1.5, vol=tm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, 2.0))
    assert c3 == tm.UPDATED and v3["tsdf"][0, 0, 0] == -1.0
    v4, _, c4 = one_voxel(2.5, vol=tm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, 2.0))
    assert c4 == tm.UPDATED and v4["tsdf"][0, 0, 0] == 1.0
    assert one_voxel(0.5, min_depth=0.5, vol=tm.volume((-0.5, -0.5, 0.0), 1.0, (1, 1, 1), 0.5, 2.0))[2] == tm.UPDATED     # depth exactly min_depth, centre z = 0.5


def test_fronto_parallel_plane_crossings_lie_within_half_a_voxel():
    vol = tm.volume((-0.6, -0.5, 1.0), 0.07, (17, 15, 30), 0.3, 8.0)
    depth = np.full((48, 64), 2.013, F)
    r = tm.integrate(vol, depth, (60.0, 60.0, 31.5, 23.5), EYE, 0.5, 5.0)
    assert r["updated"] > 1000
    pts = tm.surface_points(vol, 1.0)
    assert len(pts) > 100 and np.abs(pts[:, 2].astype(np.float64) - 2.013).max() <= 0.5 * 0.07
    assert np.array_equal(pts, tm.surface_points_literal(vol, 1.0))


def seeded_case(seed):
    rng = np.random.RandomState(seed)
    dims = tuple(int(v) for v in rng.randint(1, 14, 3))
    vol = tm.volume(rng.uniform(-2, 0, 3), rng.uniform(0.05, 0.4), dims, rng.uniform(0.05, 0.6), 4.0)
    # the camera stands 0.3 .. 2 behind the grid's centre along its own axis, a little off it, so that most poses see some of the grid
    R = rot(*rng.uniform(-0.8, 0.8, 3))
    centre = vol["origin"].astype(np.float64) + 0.5 * np.asarray(dims) * float(vol["vs"])
    c2w = np.concatenate([R, (centre - R[:, 2] * rng.uniform(0.3, 2.0) + rng.uniform(-0.3, 0.3, 3)).reshape(3, 1)], 1)
    w, h = int(rng.randint(4, 40)), int(rng.randint(4, 30))
    K = (float(rng.uniform(0.5, 1.5) * w), float(rng.uniform(0.5, 1.5) * w), float(rng.uniform(0.3, 0.7) * w), float(rng.uniform(0.3, 0.7) * h))
    max_depth = float(rng.uniform(0.5, 4.0))
    return vol, c2w, w, h, K, max_depth, rng


def test_frustum_box_equals_the_model_and_contains_every_updated_voxel():
    n_updated = n_boxes = 0
    for seed in range(200):
        vol, c2w, w, h, K, max_depth, rng = seeded_case(seed)
        lo, hi = binding.tsdf_frustum_box(desc_of(vol), w, h, K, c2w, max_depth)
        mlo, mhi = tm.frustum_box(vol, w, h, K, c2w, max_depth)
        assert (tuple(lo), tuple(hi)) == (mlo, mhi), seed
        depth = rng.uniform(0.1, max_depth * 1.2, (h, w)).astype(F)
        r = tm.integrate(vol, depth, K, c2w, 0.1, max_depth)
        box = tm.updated_box(r["code"])
        if box is not None:
            n_updated += 1
            assert all(lo[a] <= box[0][a] and box[1][a] <= hi[a] for a in range(3)), (seed, box, lo, hi)
        n_boxes += hi[0] > lo[0]
    assert n_updated >= 60 and n_boxes >= n_updated                            # the property was exercised, not vacuous


def test_frustum_box_refusals_and_degenerate_boxes():
    vol = tm.volume((0, 0, 0), 0.1, (8, 8, 8), 0.2, 4.0)
    K = (30.0, 30.0, 15.5, 11.5)
    for bad in (dict(c2w=pose(0, 0, 0, (np.nan, 0, 0))), dict(K=(np.inf, 30.0, 15.5, 11.5)), dict(max_depth=np.inf), dict(w=0)):
        a = dict(w=32, h=24, K=K, c2w=EYE, max_depth=2.0)
        a.update(bad)
        with pytest.raises(binding.NaloError):
            binding.tsdf_frustum_box(desc_of(vol), a["w"], a["h"], a["K"], a["c2w"], a["max_depth"])
    for d in (binding.tsdf_desc((0, 0, 0), 0.1, (0, 8, 8), 0.2, 4.0), binding.tsdf_desc((0, 0, 0), 0.1, (2049, 8, 8), 0.2, 4.0), binding.tsdf_desc((0, 0, 0), 0.1, (1024, 1024, 1024), 0.2, 4.0),
              binding.tsdf_desc((0, 0, 0), 0.0, (8, 8, 8), 0.2, 4.0), binding.tsdf_desc((0, 0, 0), 0.1, (8, 8, 8), np.nan, 4.0), binding.tsdf_desc((0, 0, 0), 0.1, (8, 8, 8), 0.2, -1.0),
              binding.tsdf_desc((0, np.inf, 0), 0.1, (8, 8, 8), 0.2, 4.0)):
        with pytest.raises(binding.NaloError):
            binding.tsdf_frustum_box(d, 32, 24, K, EYE, 2.0)
    # the apex inside the grid; the frustum entirely outside it; a far pose
    for c2w, empty in ((pose(0, 0, 0, (0.4, 0.4, 0.4)), False), (pose(0, 0, 0, (0.4, 0.4, 5.0)), True), (pose(0, 0, 0, (1e30, 0, 0)), True)):
        lo, hi = binding.tsdf_frustum_box(desc_of(vol), 32, 24, K, c2w, 2.0)
        assert (tuple(lo), tuple(hi)) == tm.frustum_box(vol, 32, 24, K, c2w, 2.0)
        assert (hi[0] == 0) == empty and (empty or all(0 <= lo[a] < hi[a] <= 8 for a in range(3)))


def test_surface_order_and_the_nan_and_zero_cases():
    vol = tm.volume((0, 0, 0), 0.5, (3, 2, 2), 0.2, 4.0)
    T, W = vol["tsdf"], vol["weight"]
    W[:] = 1.0
    T[:] = 1.0
    T[0, 0, 0] = -1.0                                                           # crossings of voxel (0,0,0) along x, y and z, in that order
    pts = tm.surface_points(vol, 1.0)
    assert pts.tolist() == [[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]]
    T[0, 0, 0], T[0, 0, 1], T[0, 0, 2] = 0.0, -1.0, 0.0                           # t0 == 0 against a negative: at v's centre; a negative against t1 == 0: at the neighbour's
    T[0, 1, 1] = T[1, 0, 1] = -1.0                                              # keeps (1,0,0) from crossing along y and z
    pts = tm.surface_points(vol, 1.0)
    assert pts[0].tolist() == [0.25, 0.25, 0.25] and [1.25, 0.25, 0.25] in pts.tolist()
    T[:] = 0.0
    assert len(tm.surface_points(vol, 1.0)) == 0                                # 0 against 0 is no crossing
    T[:] = 1.0
    T[0, 0, 0] = np.nan
    T[0, 0, 1] = -1.0
    W[1, 1, 1] = np.nan
    got = tm.surface_points(vol, 1.0)
    assert np.array_equal(got, tm.surface_points_literal(vol, 1.0)) and not np.isnan(got).any()
    assert [0.5, 0.25, 0.25] not in got.tolist() and [1.0, 0.25, 0.25] in got.tolist()     # NaN against -1 is none; -1 at (1,0,0) against +1 at (2,0,0) is one
    W[0, 0, 2] = 0.5
    assert [1.0, 0.25, 0.25] not in tm.surface_points(vol, 1.0).tolist() and [1.0, 0.25, 0.25] in tm.surface_points(vol, 0.5).tolist()
    # a sub-box has no neighbour outside itself
    rng = np.random.RandomState(1)
    big = tm.volume((-1, 0, 1), 0.1, (7, 6, 5), 0.2, 4.0)
    big["tsdf"][:] = rng.uniform(-1, 1, big["tsdf"].shape)
    big["weight"][:] = rng.randint(0, 3, big["weight"].shape)
    for lo, size in (((0, 0, 0), (7, 6, 5)), ((1, 2, 1), (4, 3, 2)), ((6, 5, 4), (1, 1, 1)), ((0, 0, 0), (1, 6, 5))):
        a, b = tm.surface_points(big, 1.0, lo, size), tm.surface_points_literal(big, 1.0, lo, size)
        assert np.array_equal(a, b) and (len(a) > 0 or size in ((1, 1, 1),))


def test_frame_plane_takes_the_last_record():
    pts = np.zeros(4, [("u", np.uint16), ("v", np.uint16), ("idepth", F)])
    pts["u"], pts["v"], pts["idepth"] = [1, 2, 1, 0], [0, 1, 0, 1], [0.5, 0.25, 0.125, 0.0]
    with np.errstate(all="ignore"):
        D = tm.frame_plane(pts, 3, 2)
    assert D.tolist() == [[0.0, 8.0, 0.0], [np.inf, 0.0, 4.0]]


SAN_MAIN = r'''
#include <cmath>
#include <cstdio>
#include "nalo_gpu.h"
static int run(const nalo_tsdf_desc& d, int w, int h, const double* c, float max_depth) {
    const float K[4] = {30.f, 30.f, 15.5f, 11.5f};
    int lo[3] = {-7, -7, -7}, hi[3] = {-7, -7, -7};
    const int rc = nalo_tsdf_frustum_box(&d, w, h, K, c, max_depth, lo, hi);
    std::printf("%d %d %d %d %d %d %d\n", rc, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    if (rc == 0) for (int a = 0; a < 3; ++a) if (lo[a] < 0 || hi[a] > d.dims[a] || lo[a] > hi[a]) return 1;
    return 0;
}
int main() {
    nalo_tsdf_desc d = {{0.f, 0.f, 0.f}, 0.1f, {8, 8, 8}, 0.2f, 4.f}, one = {{0.f, 0.f, 1.f}, 0.1f, {1, 1, 1}, 0.2f, 4.f}, far = {{-3e38f, 3e38f, 0.f}, 1e-30f, {2048, 1, 2048}, 1e30f, 1.f};
    double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    int bad = 0;
    double in[12], out[12], huge[12], mix[12];
    for (int i = 0; i < 12; ++i) { in[i] = out[i] = huge[i] = mix[i] = eye[i]; }
    in[3] = in[7] = in[11] = 0.4;                       /* the apex inside the grid */
    out[11] = 50.0;                                     /* the box entirely outside the grid */
    huge[3] = 1e30; huge[7] = -1e30; huge[11] = 1e30;   /* poses at 1e30 */
    for (int i = 0; i < 12; ++i) mix[i] = (i % 2 ? -1e30 : 1e30);
    bad += run(d, 32, 24, in, 2.f) + run(d, 32, 24, out, 2.f) + run(d, 32, 24, huge, 2.f) + run(d, 32, 24, mix, 3e38f);
    bad += run(one, 32, 24, eye, 2.f) + run(one, 1, 1, in, 1e-30f) + run(one, 32, 24, huge, 2.f) + run(one, 32, 24, mix, 3e38f);
    bad += run(far, 32, 24, eye, 3e38f) + run(far, 2000000000, 2000000000, mix, 3e38f) + run(far, 32, 24, huge, 2.f);
    double nanp[12]; for (int i = 0; i < 12; ++i) nanp[i] = eye[i]; nanp[5] = NAN;
    bad += run(d, 32, 24, nanp, 2.f) + run(d, 0, 24, eye, 2.f);
    nalo_tsdf_desc zero = d; zero.dims[1] = 0;
    bad += run(zero, 32, 24, eye, 2.f);
    return bad;
}
'''


def test_frustum_box_file_under_the_sanitizers_on_degenerate_inputs(tmp_path):
    """nalo-slam_amd/csrc/host_tsdf.cpp is plain C++: built with a main of its own under -fsanitize=address,undefined, it runs clean on the apex inside the grid,
    a box entirely outside it, 1-voxel grids and poses at 1e30, and every box it returns lies in the grid"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_box_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(ROOT, "nalo-slam_amd", "csrc", "host_tsdf.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    rows = [[int(v) for v in line.split()] for line in p.stdout.split("\n") if line]
    assert len(rows) == 14 and rows[0][0] == 0 and rows[0][4] > rows[0][1] and rows[1] == [0, 0, 0, 0, 0, 0, 0] and [r[0] for r in rows[-3:]] == [-1, -1, -1]
