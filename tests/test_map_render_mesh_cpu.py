"""tests/render_mesh_model.py against itself - the vectorised form against the literal one, a triangle worked by hand, the tiling property - and the host-only
half of nalo_map_render_mesh, nalo_view_triangle, against the model: seeded and planted triangles, and its file as a stand-alone program under the address and
undefined-behaviour sanitizers. No device."""
import os
import subprocess

import numpy as np
import pytest

import render_mesh_model as rmm
import render_model as rm
from conftest import ROOT
from nalo_slam_amd import binding

f32, f64 = np.float32, np.float64
EYE = np.eye(3, 4)
GREY = (40, 50, 60)
UNIT = dict(fx=1, fy=1, cx=0, cy=0)            # with z = 1 a vertex (x, y, 1) has u = x, v = y


def unit_cam(vw, vh, znear=0.5, zfar=100.0):
    return rm.make_cam(vw, vh, znear=znear, zfar=zfar, **UNIT)


def at(u, v, z=1.0):
    """the view-space point that projects to (u, v) under UNIT at depth z (exact for the dyadic values the tests use)"""
    return [u * z, v * z, z]


def test_exports_and_entry_points():
    for s in ("nalo_map_render_mesh", "nalo_view_triangle"):
        assert s in binding.EXPORTS and hasattr(binding.host_lib(), s)
    assert callable(binding.Context.map_render_mesh) and callable(binding.view_triangle)


def test_vectorised_model_equals_the_literal_one():
    view = rm.look_at((0.3, -0.4, -2.0), (0, 0, 3.0), (0, -1, 0))
    seen = dict.fromkeys(rmm.COUNTS, 0)
    for seed, (vw, vh) in enumerate(((16, 8), (70, 33), (16, 8), (64, 32))):
        cam = rm.make_cam(vw, vh, fx=20 + 7 * seed, fy=18 + 5 * seed, znear=0.7, zfar=5.0)
        mesh = rmm.seeded_mesh(seed, 90, cam, view, size=3.0 + seed)
        for mode in (0, 1):
            for box in (0, 40):
                a = rmm.render(cam, GREY, view, [mesh], mode, box, literal=True)
                b = rmm.render(cam, GREY, view, [mesh], mode, box, literal=False)
                assert rmm.same(a, b) == [], (seed, mode, box, rmm.same(a, b))
                for k in rmm.COUNTS:
                    seen[k] += a[k]
    assert all(v > 0 for v in seen.values()), seen                               # every class and some pixels occurred


def test_one_triangle_by_hand():
    """V0 = (0.5, 0.5) at z = 1, V1 = (4.5, 0.5) at z = 2, V2 = (0.5, 4.5) at z = 4: X, Y = 128 / 1152, A = 1024^2. Edge 0->1 (dy = 0, dx > 0) and edge 2->0 (dy < 0)
    are top-left, the hypotenuse (dy > 0) is not: the pixels with ix + iy < 4. With l_i the screen-space weights of a pixel, 1 / depth = l0 + l1 / 2 + l2 / 4"""
    cam = unit_cam(8, 8)
    P = np.array([at(0.5, 0.5, 1), at(4.5, 0.5, 2), at(0.5, 4.5, 4)], f32)
    T = rmm.classify(cam, P)
    assert T == dict(cls=0, X=[128, 1152, 128], Y=[128, 128, 1152], box=(0, 4, 0, 4), swapped=False)
    rgba = np.array([[30, 0, 7, 9], [255, 0, 7, 0], [0, 200, 7, 255]], np.uint8)
    tri = np.array([[0, 1, 2]], np.int32)
    for literal in (True, False):
        g = rmm.render(cam, GREY, EYE, [(P, tri, rgba)], 0, 0, literal=literal)
        covered = {(x, y) for y in range(8) for x in range(8) if np.isfinite(g["depth"][y, x])}
        assert covered == {(x, y) for y in range(4) for x in range(4) if x + y < 4} and g["n_tri_pixels"] == 10 and g["n_triangles"] == 1
        assert g["depth"][0, 0] == 1 and tuple(g["rgb"][0, 0]) == (30, 0, 7)                      # the vertex itself
        assert g["depth"][0, 2] == f32(4.0 / 3.0) and tuple(g["rgb"][0, 2]) == (105, 0, 7)        # l = (1/2, 1/2, 0): (15 + 63.75) / 0.75
        assert g["depth"][2, 0] == f32(1.6) and tuple(g["rgb"][2, 0]) == (24, 40, 7)              # l = (1/2, 0, 1/2): 1 / 0.625; 15 / 0.625, 25 / 0.625
        assert tuple(g["rgb"][5, 5]) == GREY and np.isinf(g["depth"][5, 5])
        # the exchange: submitted as (0, 2, 1) the area term is negative; the picture is the same
        h = rmm.render(cam, GREY, EYE, [(P, tri[:, [0, 2, 1]], rgba)], 0, 0, literal=literal)
        assert rmm.same(g, h) == []
        # depth exactly zfar at a pixel: zfar = 1.6 drops pixel (0, 2) and everything behind it
        far = rmm.render(dict(cam, zfar=f32(1.6)), GREY, EYE, [(P, tri, rgba)], 0, 0, literal=literal)
        assert np.isinf(far["depth"][2, 0]) and far["depth"][0, 2] == f32(4.0 / 3.0) and far["n_tri_pixels"] < 10
    Tx = rmm.classify(cam, P[[0, 2, 1]])
    assert Tx["swapped"] and Tx["X"] == T["X"] and Tx["Y"] == T["Y"]
    # colour_mode 1: normals (0, 0, 1), (0, 3, 4) and (0, 1, 0): s = 1, 0.8 and 0
    assert rmm.grey(np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2]], f32)) == 255
    assert rmm.grey(np.array([[0, 0, 5], [1, 0, 5], [0, 4, 2]], f32)) == 216                      # floor(64 + 152.8)
    assert rmm.grey(np.array([[0, 0, 1], [1, 0, 1], [0, 0, 3]], f32)) == 64                       # seen edge-on
    assert rmm.grey(np.array([[0, 0, 1], [0, 0, 1], [0, 0, 3]], f32)) == 64                       # no normal at all
    g1 = rmm.render(cam, GREY, EYE, [(P, tri, None)], 1, 0, literal=True)
    assert len({tuple(c) for c in g1["rgb"][np.isfinite(g1["depth"])]}) == 1 and g1["rgb"][0, 0, 0] == rmm.grey(P)


def coverage(cam, P, tris):
    cover = np.zeros((cam["vh"], cam["vw"]), np.int32)
    for t in tris:
        T = rmm.classify(cam, P[list(t)], cam["vw"] * cam["vh"])
        assert T["cls"] == rmm.DRAWN
        idx = [t[0], t[2], t[1]] if T["swapped"] else list(t)
        for iy in range(cam["vh"]):
            for ix in range(cam["vw"]):
                cover[iy, ix] += rmm.pixel(cam, T["X"], T["Y"], [P[i, 2] for i in idx], 200, ix, iy, 1) is not None
    return cover


def test_a_tiling_covers_every_pixel_exactly_once():
    """a lattice of vertices ON pixel centres, two pixels apart, from outside the viewport to outside it: lattice lines and every diagonal run through centres,
    every inner vertex is a centre. Random diagonals, random windings, random rotations of the index triple: every pixel is covered exactly once"""
    cam = unit_cam(16, 8)
    rng = np.random.RandomState(5)
    us, vs = np.arange(-1.5, 18, 2.0), np.arange(-1.5, 10, 2.0)
    P = np.array([at(u, v, 1.0 + 0.25 * ((i + 2 * j) % 3)) for j, v in enumerate(vs) for i, u in enumerate(us)], f32)
    n = len(us)
    tris = []
    for j in range(len(vs) - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            for t in (((a, b, d), (a, d, c)) if rng.randint(2) else ((a, b, c), (b, d, c))):
                t = t if rng.randint(2) else (t[0], t[2], t[1])
                r = rng.randint(3)
                tris.append(t[r:] + t[:r])
    cover = coverage(cam, P, tris)
    assert (cover == 1).all(), cover
    # a fan around a centre: eight triangles around (4.5, 3.5) with rim vertices on and off centres
    hub = at(4.5, 3.5)
    rim = [at(8.5, 3.5), at(7.25, 6.5), at(4.5, 7.5), at(1.5, 6.5), at(0.5, 3.5), at(1.75, 0.5), at(4.5, -0.5), at(7.5, 0.5)]
    Pf = np.array([hub] + rim, f32)
    fan = [(0, 1 + k, 1 + (k + 1) % 8) if k % 2 else (0, 1 + (k + 1) % 8, 1 + k) for k in range(8)]
    cf = coverage(cam, Pf, fan)
    assert cf.max() == 1 and cf[3, 4] == 1 and cf.sum() > 20
    # two triangles that share an edge through centres never both take a pixel, in either order and winding
    sq = np.array([at(2.5, 1.5), at(6.5, 1.5), at(6.5, 5.5), at(2.5, 5.5)], f32)
    for t0, t1 in (((0, 1, 2), (0, 2, 3)), ((0, 2, 1), (0, 3, 2)), ((2, 0, 1), (3, 0, 2))):
        c2 = coverage(cam, sq, [t0, t1])
        assert c2.max() == 1 and c2.sum() == 16 and c2[1:5, 2:6].all()                            # left and top edges in, right and bottom out


def cam_args(cam):
    return dict(fx=float(cam["fx"]), fy=float(cam["fy"]), cx=float(cam["cx"]), cy=float(cam["cy"]), znear=float(cam["znear"]))


def lib_triangle(cam, P, box=0):
    return binding.view_triangle(cam["vw"], cam["vh"], P, max_box_pixels=box, **cam_args(cam))


def agree(cam, P, box=0):
    want, got = rmm.classify(cam, P, box), lib_triangle(cam, P, box)
    assert got == dict(cls=want["cls"], X=want["X"], Y=want["Y"], box=want["box"]), (P, got, want)
    return got


def test_view_triangle_on_seeded_triangles():
    view = rm.look_at((0.3, -0.4, -2.0), (0, 0, 3.0), (0, -1, 0))
    cam = rm.make_cam(70, 33, fx=37.5, fy=31.25, znear=0.7, zfar=50)
    xyz, tri, _ = rmm.seeded_mesh(11, 2000, cam, view, size=5.0)
    P = rmm.view_vertices(view, xyz)
    seen = {}
    for k, t in enumerate(tri):
        if t.min() < 0 or t.max() >= len(P):
            continue
        g = agree(cam, P[t], 0 if k % 2 else 60)
        seen[g["cls"]] = seen.get(g["cls"], 0) + 1
    assert set(seen) == {0, 2, 3, 4, 5} and seen[0] > 1000, seen


def test_view_triangle_on_planted_triangles():
    cam = unit_cam(16, 8)
    tri = [at(2.5, 1.5), at(6.5, 1.5), at(2.5, 5.5)]
    assert agree(cam, tri) == dict(cls=0, X=[640, 1664, 640], Y=[384, 384, 1408], box=(2, 6, 1, 5))
    assert agree(cam, [tri[0], tri[2], tri[1]])["X"] == [640, 1664, 640]                             # after the exchange
    # near: zv exactly znear, below it, NaN, infinity
    for bad in ([1.0, 1.0, 0.5], [1.0, 1.0, 0.25], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, np.inf], [1.0, 1.0, -2.0]):
        for k in range(3):
            P = [list(p) for p in tri]
            P[k] = bad
            assert agree(cam, P) == dict(cls=2, X=[0, 0, 0], Y=[0, 0, 0], box=(0, -1, 0, -1))
    assert agree(cam, [tri[0], tri[1], [1.0, 1.0, float(np.nextafter(f32(0.5), f32(1)))]])["cls"] == 0   # just in front of the plane
    # the guard at exactly +-131072, and the last float inside it
    edge, inside = 131072.0, float(np.nextafter(f32(131072), f32(0)))
    for k in range(2):
        for sgn in (1.0, -1.0):
            P = [list(p) for p in tri]
            P[1][k] = sgn * edge
            assert agree(cam, P) == dict(cls=3, X=[0, 0, 0], Y=[0, 0, 0], box=(0, -1, 0, -1))
            P[1][k] = sgn * inside
            g = agree(cam, P)
            assert g["cls"] == 0 and int(sgn * inside * 256) in (g["X"], g["Y"])[k]               # 2^25 - 2: the largest snapped coordinate
    assert agree(cam, [tri[0], [3e38, 1.0, 1.0], tri[2]])["cls"] == 3 and agree(cam, [tri[0], [3e38, 1.0, 3e-38], tri[2]])["cls"] == 2      # u overflows; z below znear
    # u * 256 + 0.5 on a tie: u * 256 = 2^23 + 1 is odd and the float sum rounds to the even 2^23 + 2; exact arithmetic would floor 2^23 + 1.5 to 2^23 + 1
    u = (2 ** 23 + 1) / 256.0
    assert float(f32(u)) == u
    g = agree(cam, [tri[0], [u, 1.5, 1.0], tri[2]])
    assert 2 ** 23 + 2 in g["X"] and 2 ** 23 + 1 not in g["X"]
    # degenerate: a repeated vertex, three vertices on a line, two vertices inside one sub-pixel
    for P in ([tri[0], tri[0], tri[1]], [at(1.5, 1.5), at(3.5, 2.5), at(5.5, 3.5)], [tri[0], at(2.5 + 1 / 1024, 1.5), tri[2]]):
        g = agree(cam, P)
        assert g["cls"] == 4 and g["box"] == (0, -1, 0, -1)
    # large: a box of exactly max_box_pixels pixels is drawn, one more is not; the default is 65536
    assert agree(cam, tri, 25)["cls"] == 0 and agree(cam, tri, 24)["cls"] == 5 and agree(cam, tri, 24)["box"] == (2, 6, 1, 5)
    big = unit_cam(65536, 4)
    wide = [at(0.5, 0.5), at(16384.5, 0.5), at(0.5, 3.75)]                                           # 16385 x 4 centres = 65540 pixels; 16384 x 4 = 65536
    assert agree(big, wide)["cls"] == 5 and agree(big, [wide[0], at(16384.25, 0.5), wide[2]])["cls"] == 0
    # drawn with an empty box: a sliver between centres, a triangle outside the viewport
    assert agree(cam, [at(2.6, 1.6), at(3.4, 1.7), at(2.7, 2.4)]) == dict(cls=0, X=[666, 870, 691], Y=[410, 435, 614], box=(0, -1, 0, -1))
    assert agree(cam, [at(-9.5, 1.5), at(-3.5, 1.5), at(-9.5, 5.5)])["box"] == (0, -1, 0, -1)
    assert agree(cam, [at(0.5, 0.5), at(1.5, 0.5), at(0.5, 1.5)])["box"] == (0, 1, 0, 1)             # one pixel is covered; the box holds the centres on its border too
    # refusals write nothing
    L = binding.host_lib()
    a = binding.MapRenderArgs()
    a.vw, a.vh, a.fx, a.fy, a.znear = 16, 8, 1.0, 1.0, 0.5
    P = np.ascontiguousarray(tri, f32).reshape(9)
    out = [np.full(n, -7, np.int32) for n in (1, 3, 3, 4)]
    ptr = [binding._i(o) for o in out]
    import ctypes as C
    assert L.nalo_view_triangle(C.byref(a), binding._f(P), -1, *ptr) == -1
    assert L.nalo_view_triangle(None, binding._f(P), 0, *ptr) == -1 and L.nalo_view_triangle(C.byref(a), None, 0, *ptr) == -1
    assert L.nalo_view_triangle(C.byref(a), binding._f(P), 0, None, *ptr[1:]) == -1
    for vw, vh in ((0, 8), (16, 0), (65537, 8), (16, 65537)):
        a.vw, a.vh = vw, vh
        assert L.nalo_view_triangle(C.byref(a), binding._f(P), 0, *ptr) == -1
    assert all((o == -7).all() for o in out)
    a.vw, a.vh = 65536, 65536
    assert L.nalo_view_triangle(C.byref(a), binding._f(P), 0, *ptr) == 0 and out[0][0] == 0


SAN_MAIN = r'''
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "nalo_gpu.h"
int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float vals[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1e-38f, 1e38f, -1e38f, 3.4e38f, nan, inf, -inf, 131072.0f, -131072.0f, 65536.5f, 1e-45f};
    const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
    const float cams[][7] = {{1.f, 1.f, 0.f, 0.f, 0.5f}, {400.f, 400.f, 320.f, 240.f, 0.1f}, {1e38f, -1e38f, 1e38f, 0.f, 1e-38f}, {nan, inf, -inf, nan, nan}, {0.f, 0.f, 0.f, 0.f, 0.f}};
    const int sizes[][2] = {{1, 1}, {16, 8}, {65536, 65536}};
    int bad = 0;
    long long count[6] = {0, 0, 0, 0, 0, 0};
    for (const auto& cm : cams) for (const auto& sz : sizes) {
        nalo_map_render_args a = {};
        a.vw = sz[0]; a.vh = sz[1]; a.fx = cm[0]; a.fy = cm[1]; a.cx = cm[2]; a.cy = cm[3]; a.znear = cm[4];
        for (int i = 0; i < nv; ++i) for (int j = 0; j < nv; ++j) for (int k = 0; k < nv; ++k) for (long long box : {0ll, 1ll, 9223372036854775807ll}) {
            const float P[3][3] = {{vals[i], vals[j], 1.0f}, {vals[j], vals[k], vals[(i + k) % nv]}, {2.5f, vals[i], vals[k]}};
            int cls = -7, X[3] = {-7, -7, -7}, Y[3] = {-7, -7, -7}, box_out[4] = {-7, -7, -7, -7};
            const int rc = nalo_view_triangle(&a, P, box, &cls, X, Y, box_out);
            if (rc != 0 || cls < 0 || cls == 1 || cls > 5) { ++bad; continue; }
            ++count[cls];
            for (int q = 0; q < 3; ++q) if (X[q] < -(1 << 25) || X[q] > (1 << 25) || Y[q] < -(1 << 25) || Y[q] > (1 << 25)) ++bad;
            const bool empty = box_out[1] < box_out[0];
            if (!empty && (box_out[0] < 0 || box_out[1] >= a.vw || box_out[2] < 0 || box_out[3] >= a.vh || box_out[3] < box_out[2])) ++bad;
            if (empty && !(box_out[0] == 0 && box_out[1] == -1 && box_out[2] == 0 && box_out[3] == -1)) ++bad;
            if ((cls >= 2 && cls <= 4) && !empty) ++bad;
        }
    }
    std::printf("C %lld %lld %lld %lld %lld %lld\n", count[0], count[1], count[2], count[3], count[4], count[5]);
    return bad != 0;
}
'''


def test_view_triangle_under_the_sanitizers_on_degenerate_inputs(tmp_path):
    """nalo-slam_amd/csrc/host_map_render_mesh.cpp is plain C++: built with a main of its own under -fsanitize=address,undefined, nalo_view_triangle runs clean on
    NaN, infinities, 1e38 and denormal coordinates and cameras, every snapped coordinate stays inside the guard and every box inside the viewport"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "view_triangle_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(ROOT, "nalo-slam_amd", "csrc", "host_map_render_mesh.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    row = [line.split() for line in p.stdout.split("\n") if line.startswith("C ")][0]
    n = [int(v) for v in row[1:]]
    assert sum(n) == 5 * 3 * 16 ** 3 * 3 and n[1] == 0 and all(v > 0 for v in (n[0], n[2], n[3], n[4], n[5])), n
