"""tests/tsdf_color_model.py on hand-worked voxels and vertices and its two forms against each other, and the host-only half of the coloured mesh: the PLY writer
(nalo_io_write_ply_mesh_rgba) against the model's bytes, its refusals, and the writer under the address and undefined-behaviour sanitizers as a stand-alone
program. No device."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_color_model as cm
import tsdf_mesh_model as mm
import tsdf_model as tm
from conftest import ROOT
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth

F = np.float32


def bits_eq(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def test_exports_and_entry_points():
    for s in ("nalo_tsdf_color_enable", "nalo_tsdf_color_disable", "nalo_tsdf_integrate_depth_color", "nalo_tsdf_color_get", "nalo_tsdf_color_set", "nalo_tsdf_color_view",
              "nalo_tsdf_mesh_color", "nalo_tsdf_mesh_color_view"):
        assert s in binding.EXPORTS and hasattr(binding.host_lib(), s)
    assert hasattr(binding.host_lib(), "nalo_io_write_ply_mesh_rgba")
    for m in ("tsdf_color_enable", "tsdf_color_disable", "tsdf_color_get", "tsdf_color_set", "tsdf_color_view", "tsdf_mesh_color_view"):
        assert callable(getattr(binding.Context, m))
    assert "nalo_io_write_ply_mesh_rgba" in open(os.path.join(ROOT, "include", "nalo_io_mesh.h")).read()


@pytest.mark.parametrize("c2w", [EYE, pose(0.2, -0.3, 0.15, (0.2, -0.1, 0.1))])
def test_vectorised_integration_equals_the_literal_one(c2w):
    K, w, h = (20.0, 19.0, 11.5, 8.5), 24, 18
    depth = wavy_depth(w, h, 3)
    a, b = (cm.volume((-1.1, -0.9, 0.8), 0.17, (13, 11, 12), 0.4, 2.5) for _ in range(2))
    rng = np.random.RandomState(4)
    for it in range(4):                                                        # w0 = 0, 1, 2 and the saturated 2.5
        bgr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        n, code = cm.integrate_literal(a, depth + F(0.03 * it), bgr, K, c2w, 0.5, 3.0)
        r = cm.integrate(b, depth + F(0.03 * it), bgr, K, c2w, 0.5, 3.0)
        assert n == r["updated"] > 100 and np.array_equal(code, r["code"])
        assert bits_eq(a["tsdf"], b["tsdf"]) and bits_eq(a["weight"], b["weight"]) and bits_eq(a["colour"], b["colour"])
    assert a["weight"].max() == 2.5 and (a["colour"] > 0).sum() > 300
    never = a["weight"] == 0
    assert never.any() and not a["colour"][:, never].any()                      # a voxel that was never updated keeps 0.0


def test_one_voxel_by_hand_through_three_updates():
    """a 1x1x1 grid whose centre (0, 0, 2) projects to pixel (8, 6) at the identity: w0 = 0, 1, 2 with the colours (10, 20, 30), (40, 50, 61), (1, 2, 3)"""
    vol = cm.volume((-0.5, -0.5, 1.5), 1.0, (1, 1, 1), 0.5, 8.0)
    depth = np.full((12, 16), 2.0, F)
    K = (10.0, 10.0, 8.0, 6.0)
    want = []
    for w0, c in enumerate(((10, 20, 30), (40, 50, 61), (1, 2, 3))):
        bgr = np.full((12, 16, 3), 200, np.uint8)
        bgr[6, 8] = c
        twin = dict(vol, tsdf=vol["tsdf"].copy(), weight=vol["weight"].copy(), colour=vol["colour"].copy())
        r = cm.integrate(vol, depth, bgr, K, EYE, 0.5, 4.0)
        cm.integrate_literal(twin, depth, bgr, K, EYE, 0.5, 4.0)
        assert r["updated"] == 1 and vol["weight"][0, 0, 0] == w0 + 1 and bits_eq(vol["colour"], twin["colour"])
        want.append(vol["colour"][:, 0, 0, 0].tolist())
    assert want[0] == [10.0, 20.0, 30.0]                                        # (0 * 0 + x) / 1
    assert want[1] == [25.0, 35.0, 45.5]                                        # (x0 * 1 + x) / 2
    assert want[2] == [float(F(F(51.0) / F(3.0))), float(F(F(72.0) / F(3.0))), float(F(F(94.0) / F(3.0)))]       # (x0 * 2 + x) / 3
    # a pixel without a usable depth: the three words stay, bit for bit
    vol["colour"].view(np.uint32)[:, 0, 0, 0] = (0x7FC12345, 0xFFA00001, 0x00000001)
    before = vol["colour"].copy()
    depth[6, 8] = 0.0
    assert cm.integrate(vol, depth, bgr, K, EYE, 0.5, 4.0)["updated"] == 0 and bits_eq(vol["colour"], before)


def test_the_byte_conversion():
    got = cm.colour_byte(np.array([254.49, 254.5, 255.4, -0.3, np.nan, np.inf, -np.inf, 0.49, 0.5, 127.5], F))
    assert got.dtype == np.uint8 and got.tolist() == [254, 255, 255, 0, 0, 255, 0, 0, 1, 128]


def test_one_vertex_by_hand():
    """two voxels along x, t = (-0.25, 0.75): s = 0.25. B runs 100 -> 200 (125), G 10 -> 11 (10.25 -> 10), R 300 -> 100 (250); output order R, G, B, 255"""
    vol = cm.volume((0, 0, 0), 1.0, (2, 1, 1), 0.5, 4.0)
    vol["weight"][:] = 1.0
    vol["tsdf"][0, 0, :] = (-0.25, 0.75)
    vol["colour"][:, 0, 0, 0] = (100.0, 10.0, 300.0)
    vol["colour"][:, 0, 0, 1] = (200.0, 11.0, 100.0)
    xyz = mm.mesh_literal(vol, 1.0)[0]
    assert xyz.tolist() == [[0.75, 0.5, 0.5]]
    assert cm.mesh_colours_literal(vol, 1.0).tolist() == [[250, 10, 125, 255]] and cm.mesh_colours(vol, 1.0).tolist() == [[250, 10, 125, 255]]
    # an infinite far end: s = 0, and 0 * (inf - x) is not reached: X(n) - X(v) is finite, the colour is X(v); an infinite near end: s is NaN, the colour 0
    vol["tsdf"][0, 0, :] = (-0.25, np.inf)
    assert cm.mesh_colours_literal(vol, 1.0).tolist() == [[255, 10, 100, 255]]
    vol["tsdf"][0, 0, :] = (np.inf, -0.25)
    assert cm.mesh_colours_literal(vol, 1.0).tolist() == [[0, 0, 0, 255]] and cm.mesh_colours(vol, 1.0).tolist() == [[0, 0, 0, 255]]


def coloured_random_volume(dims, seed):
    rng = np.random.RandomState(seed)
    vol = cm.volume((-0.7, 0.3, 1.1), 0.125, dims, 0.4, 4.0)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["tsdf"].reshape(-1)[::37] = np.nan
    vol["tsdf"].reshape(-1)[5::41] = np.inf
    vol["weight"][:] = np.where(rng.rand(*vol["weight"].shape) < 0.05, 0.0, rng.randint(1, 4, vol["weight"].shape))
    vol["colour"][:] = rng.uniform(-40, 300, vol["colour"].shape)               # below 0 and above 255 among them
    vol["colour"].reshape(-1)[3::29] = np.nan
    return vol


@pytest.mark.parametrize("dims,lo,size", [((9, 7, 6), None, None), ((9, 7, 6), (1, 2, 1), (6, 4, 4)), ((5, 3, 2), None, None), ((2, 2, 2), None, None), ((1, 1, 1), None, None)])
def test_vectorised_vertex_colours_equal_the_literal_ones(dims, lo, size):
    vol = coloured_random_volume(dims, sum(dims))
    for mw in (2.0, 1.0):
        lit, vec = cm.mesh_colours_literal(vol, mw, lo, size), cm.mesh_colours(vol, mw, lo, size)
        assert lit.shape == vec.shape == (len(mm.mesh(vol, mw, lo, size)[0]), 4) and np.array_equal(lit, vec)
    if min(dims) > 2 and lo is None:
        assert len(lit) > 50 and (lit[:, :3] == 0).any() and (lit[:, :3] == 255).any() and (lit[:, 3] == 255).all()


def test_frame_colour_plane_takes_the_last_record():
    pts = np.zeros(4, binding.DENSE_POINT_DTYPE)
    pts["u"], pts["v"], pts["idepth"] = (3, 1, 3, 0), (2, 0, 2, 0), (0.5, 0.25, 1.0, 2.0)
    pts["bgr"] = ((1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))
    Cp = cm.frame_color_plane(pts, 5, 4)
    assert Cp[2, 3].tolist() == [7, 8, 9] and Cp[0, 1].tolist() == [4, 5, 6] and Cp[0, 0].tolist() == [10, 11, 12] and int((Cp != 0).any(2).sum()) == 3
    assert tm.frame_plane(pts, 5, 4)[2, 3] == 1.0                               # the same record supplies the depth


def test_ply_bytes_and_refusals(tmp_path):
    vol = mm.sphere(8, 2.3)
    xyz, tri = mm.mesh(vol, 1.0)
    rgba = np.random.RandomState(1).randint(0, 256, (len(xyz), 4)).astype(np.uint8)
    assert len(tri) > 50
    a = str(tmp_path / "lib.ply")
    binding.write_ply_mesh(a, xyz, tri, rgba)
    got = open(a, "rb").read()
    assert got == cm.ply_bytes(xyz, rgba, tri) and len(got) == got.index(b"end_header\n") + 11 + 16 * len(xyz) + 13 * len(tri)
    assert b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face" in got
    # without colours the file is the one it was
    binding.write_ply_mesh(a, xyz, tri)
    mm.write_ply(str(tmp_path / "plain.ply"), xyz, tri)
    assert open(a, "rb").read() == open(tmp_path / "plain.ply", "rb").read()
    # empty meshes, and vertices without faces
    none3, none4, nonet = np.zeros((0, 3), F), np.zeros((0, 4), np.uint8), np.zeros((0, 3), np.int32)
    binding.write_ply_mesh(a, none3, nonet, none4)
    assert open(a, "rb").read() == cm.ply_bytes(none3, none4, nonet)
    binding.write_ply_mesh(a, xyz, nonet, rgba)
    assert open(a, "rb").read() == cm.ply_bytes(xyz, rgba, nonet)
    # refusals: no file is touched
    L, fp, ip, up = binding.host_lib(), binding.c_fp, binding.c_ip, binding.c_u8p
    fresh = str(tmp_path / "never.ply")
    X, Cc, T = xyz.ctypes.data_as(fp), rgba.ctypes.data_as(up), tri.ctypes.data_as(ip)
    for bad in (len(xyz), -1):
        t = tri.copy()
        t[len(t) // 2, 1] = bad
        assert L.nalo_io_write_ply_mesh_rgba(fresh.encode(), len(xyz), X, Cc, len(t), t.ctypes.data_as(ip)) == -1 and not os.path.exists(fresh)
    assert L.nalo_io_write_ply_mesh_rgba(fresh.encode(), len(xyz), X, None, len(tri), T) == -1                    # colours missing
    assert L.nalo_io_write_ply_mesh_rgba(fresh.encode(), len(xyz), None, Cc, len(tri), T) == -1
    assert L.nalo_io_write_ply_mesh_rgba(fresh.encode(), 0, None, None, 1, T) == -1                               # a triangle without vertices
    assert L.nalo_io_write_ply_mesh_rgba(None, 0, None, None, 0, None) == -1 and L.nalo_io_write_ply_mesh_rgba(fresh.encode(), -1, None, None, 0, None) == -1
    assert L.nalo_io_write_ply_mesh_rgba(fresh.encode(), 0, None, None, 2, None) == -1 and L.nalo_io_write_ply_mesh_rgba(fresh.encode(), 0, None, None, -1, None) == -1
    assert not os.path.exists(fresh)
    assert L.nalo_io_write_ply_mesh_rgba(str(tmp_path / "no_such_dir" / "m.ply").encode(), len(xyz), X, Cc, len(tri), T) == -2
    with pytest.raises(binding.NaloError):
        binding.write_ply_mesh(str(tmp_path / "no_such_dir" / "m.ply"), xyz, tri, rgba)
    with pytest.raises(binding.NaloError):
        binding.write_ply_mesh(fresh, xyz, tri, rgba[:-1])
    assert not os.path.exists(fresh)


SAN_MAIN = r'''
#include <cstdio>
#include "nalo_io.h"
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    char path[4096];
    const float xyz[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    const unsigned char rgba[12] = {1, 2, 3, 255, 250, 128, 0, 255, 9, 8, 7, 255};
    int tri[6] = {0, 1, 2, 2, 1, 0};
    std::snprintf(path, sizeof path, "%s/empty.ply", argv[1]);
    std::printf("empty %d\n", nalo_io_write_ply_mesh_rgba(path, 0, nullptr, nullptr, 0, nullptr));
    std::snprintf(path, sizeof path, "%s/points.ply", argv[1]);
    std::printf("points %d\n", nalo_io_write_ply_mesh_rgba(path, 3, xyz, rgba, 0, nullptr));
    std::snprintf(path, sizeof path, "%s/two.ply", argv[1]);
    std::printf("two %d\n", nalo_io_write_ply_mesh_rgba(path, 3, xyz, rgba, 2, tri));
    std::snprintf(path, sizeof path, "%s/bad.ply", argv[1]);
    tri[4] = 3;
    std::printf("past %d\n", nalo_io_write_ply_mesh_rgba(path, 3, xyz, rgba, 2, tri));
    tri[4] = -2147483647 - 1;
    std::printf("negative %d\n", nalo_io_write_ply_mesh_rgba(path, 3, xyz, rgba, 2, tri));
    tri[4] = 2147483647;
    std::printf("huge %d\n", nalo_io_write_ply_mesh_rgba(path, 3, xyz, rgba, 2, tri));
    tri[4] = 0;
    std::printf("no vertices %d\n", nalo_io_write_ply_mesh_rgba(path, 0, nullptr, nullptr, 2, tri));
    std::printf("null %d %d %d\n", nalo_io_write_ply_mesh_rgba(nullptr, 0, nullptr, nullptr, 0, nullptr), nalo_io_write_ply_mesh_rgba(path, 3, nullptr, rgba, 2, tri),
                nalo_io_write_ply_mesh_rgba(path, 3, xyz, nullptr, 2, tri));
    std::snprintf(path, sizeof path, "%s/no_such_dir/m.ply", argv[1]);
    std::printf("dir %d\n", nalo_io_write_ply_mesh_rgba(path, 3, xyz, rgba, 2, tri));
    return 0;
}
'''


def test_coloured_ply_writer_under_the_sanitizers(tmp_path):
    """host_io.cpp is plain C++: built with a main of its own under -fsanitize=address,undefined, the coloured writer runs clean on an empty mesh, on vertices
    without faces, on a mesh of two triangles and on indices outside the vertices"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_color_san"
    csrc = os.path.join(ROOT, "nalo-slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(csrc, "host_tsdf.cpp"), os.path.join(csrc, "host_io.cpp"), "-lz", "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    assert p.stdout.split("\n")[:-1] == ["empty 0", "points 0", "two 0", "past -1", "negative -1", "huge -1", "no vertices -1", "null -1 -1 -1", "dir -2"]
    assert not os.path.exists(tmp_path / "bad.ply")
    xyz, tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    rgba = np.array([[1, 2, 3, 255], [250, 128, 0, 255], [9, 8, 7, 255]], np.uint8)
    assert open(tmp_path / "two.ply", "rb").read() == cm.ply_bytes(xyz, rgba, tri)
    assert open(tmp_path / "points.ply", "rb").read() == cm.ply_bytes(xyz, rgba, tri[:0])
    assert open(tmp_path / "empty.ply", "rb").read() == cm.ply_bytes(xyz[:0], rgba[:0], tri[:0])
