"""tests/tsdf_mesh_model.py on hand-worked cells, its two forms against each other, the closed-surface properties of the definition, and the host-only half of
nalo_tsdf_mesh: the triangle table (nalo_tsdf_mesh_table) against the rule-built one, the PLY writer (nalo_io_write_ply_mesh) against the model's bytes, and both
under the address and undefined-behaviour sanitizers as a stand-alone program. No device."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_mesh_model as mm
import tsdf_model as tm
from conftest import ROOT
from nalo_slam_amd import binding

F = np.float32


def random_volume(dims, seed, p_invalid=0.15):
    rng = np.random.RandomState(seed)
    vol = tm.volume((-0.7, 0.3, 1.1), 0.125, dims, 0.4, 4.0)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["weight"][:] = np.where(rng.rand(*vol["weight"].shape) < p_invalid, 0.0, rng.randint(1, 4, vol["weight"].shape))
    return vol


def test_exports_and_entry_points():
    for s in ("nalo_tsdf_mesh", "nalo_tsdf_mesh_view", "nalo_tsdf_mesh_table"):
        assert s in binding.EXPORTS and hasattr(binding.host_lib(), s)
    assert hasattr(binding.host_lib(), "nalo_io_write_ply_mesh")
    for m in ("tsdf_mesh", "tsdf_mesh_view"):
        assert callable(getattr(binding.Context, m))
    hdr = open(os.path.join(ROOT, "include", "nalo_gpu.h")).read()
    assert '"tsdf_mesh"' in hdr and "nalo_io_mesh.h" in open(os.path.join(ROOT, "include", "nalo_io.h")).read()


def test_library_table_equals_the_rule_built_table():
    tab = binding.tsdf_mesh_table()
    assert tab.dtype == np.int8 and tab.shape == (6, 16, 6) and np.array_equal(tab, mm.TABLE)
    assert int((tab[:, :, 0] >= 0).sum() + (tab[:, :, 3] >= 0).sum()) == 120
    assert (tab[:, 0] == -1).all() and (tab[:, 15] == -1).all()
    for t in range(6):
        for mask in range(1, 15):
            n = bin(mask).count("1")
            assert int((tab[t, mask] >= 0).sum()) == (6 if n == 2 else 3)
            for c in tab[t, mask][tab[t, mask] >= 0]:
                p, m = int(c) >> 3, int(c) & 7
                q = p ^ m
                assert p in mm.TETS[t] and q in mm.TETS[t] and p & q == p and m != 0
                assert ((mask >> mm.TETS[t].index(p)) & 1) != ((mask >> mm.TETS[t].index(q)) & 1)      # the edge is cut
    assert binding.host_lib().nalo_tsdf_mesh_table(None) == -1


def one_cell(inside_corners, invalid=()):
    vol = tm.volume((0, 0, 0), 1.0, (2, 2, 2), 0.5, 4.0)
    vol["weight"][:] = 1.0
    for b in range(8):
        vol["tsdf"][(b >> 2) & 1, (b >> 1) & 1, b & 1] = -1.0 if b in inside_corners else 1.0
    for b in invalid:
        vol["weight"][(b >> 2) & 1, (b >> 1) & 1, b & 1] = 0.0
    xyz, tri, owner = mm.mesh_literal(vol, 1.0)
    vx, vt = mm.mesh(vol, 1.0)
    assert mm.same_floats(xyz, vx) and np.array_equal(tri, vt)
    return xyz, tri, owner


def test_one_cell_by_hand():
    # corner 0 alone inside: seven vertices on voxel (0,0,0)'s seven edges, half way (t0 / (t0 - t1) = 0.5), a fan of six triangles round the body diagonal's vertex
    xyz, tri, owner = one_cell({0})
    assert owner == [(0, 0, 0, m) for m in range(1, 8)]
    assert xyz.tolist() == [[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [1.0, 1.0, 0.5], [0.5, 0.5, 1.0], [1.0, 0.5, 1.0], [0.5, 1.0, 1.0], [1.0, 1.0, 1.0]]
    assert tri.tolist() == [[0, 2, 6], [0, 6, 4], [1, 6, 2], [1, 5, 6], [3, 4, 6], [3, 6, 5]]
    # the same cell with the signs exchanged: the same vertices, every triangle turned over
    xyz2, tri2, _ = one_cell({1, 2, 3, 4, 5, 6, 7})
    assert mm.same_floats(xyz, xyz2) and tri2.tolist() == [[t[0], t[2], t[1]] for t in tri.tolist()]
    # two and two: corners 0 and 1 inside. Voxel (0,0,0) owns m = 2..7 (indices 0..5), voxel (1,0,0) owns m = 2, 4, 6 (indices 6, 7, 8)
    xyz, tri, owner = one_cell({0, 1})
    assert owner == [(0, 0, 0, m) for m in range(2, 8)] + [(1, 0, 0, m) for m in (2, 4, 6)]
    assert len(tri) == 8 and tri[:2].tolist() == [[1, 5, 8], [1, 8, 6]]          # T0 = (0,1,3,7): the quad 0.3, 0.7, 1.7, 1.3
    # every normal looks from the inside corners to the outside ones
    p = xyz.astype(np.float64)
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    assert (n[:, 1] + n[:, 2] > 0).all()                                        # the inside edge runs along x at y = z = 0.5
    # an invalid corner: the cell is not live, the vertices between valid corners stay
    xyz, tri, owner = one_cell({0}, invalid=(7,))
    assert len(tri) == 0 and owner == [(0, 0, 0, m) for m in range(1, 7)]
    xyz, tri, owner = one_cell({0}, invalid=(0,))
    assert len(tri) == 0 and len(xyz) == 0
    # 0.0f and -0.0f are outside, a NaN is not valid
    vol = tm.volume((0, 0, 0), 1.0, (2, 1, 1), 0.5, 4.0)
    vol["weight"][:] = 1.0
    for t1, n in ((0.0, 1), (-0.0, 1), (np.nan, 0), (-0.5, 0), (np.inf, 1)):
        vol["tsdf"][0, 0, :] = (-1.0, t1)
        xyz, tri, _ = mm.mesh_literal(vol, 1.0)
        assert len(xyz) == n and len(tri) == 0 and mm.same_floats(xyz, mm.mesh(vol, 1.0)[0])
        if n:
            assert xyz[0].tolist() == [0.5 + (0.0 if np.isinf(t1) else 1.0), 0.5, 0.5]


@pytest.mark.parametrize("dims,lo,size", [((9, 7, 6), None, None), ((9, 7, 6), (1, 2, 1), (6, 4, 4)), ((9, 7, 6), (8, 0, 0), (1, 7, 6)), ((5, 3, 2), None, None),
                                           ((2, 2, 2), None, None), ((1, 1, 1), None, None), ((13, 1, 4), None, None)])
def test_vectorised_model_equals_the_literal_one(dims, lo, size):
    vol = random_volume(dims, sum(dims), p_invalid=0.04)
    vol["tsdf"].reshape(-1)[::37] = np.nan
    vol["tsdf"].reshape(-1)[3::19] = 0.0
    vol["tsdf"].reshape(-1)[5::23] = -0.0
    for mw in (2.0, 1.0):
        xyz, tri, owner = mm.mesh_literal(vol, mw, lo, size)
        vx, vt, axis = mm.mesh(vol, mw, lo, size, with_axis=True)
        assert mm.same_floats(xyz, vx) and np.array_equal(tri, vt) and [o[3] for o in owner] == axis.tolist()
        assert len(tri) == 0 or (tri.min() >= 0 and tri.max() < len(xyz))
        # the axis edges, in order, are the surface points of tests/tsdf_model.py
        assert mm.same_floats(vx[np.isin(axis, (1, 2, 4))], tm.surface_points(vol, mw, lo, size))
    if min(dims) > 2 and lo is None:
        assert len(tri) > 20


def test_planted_sphere_is_closed_and_outward_and_its_complement_inward():
    vol = mm.sphere()
    xyz, tri, _ = mm.mesh_literal(vol, 1.0)
    vx, vt = mm.mesh(vol, 1.0)
    assert mm.same_floats(xyz, vx) and np.array_equal(tri, vt) and len(tri) > 500
    assert mm.is_closed_and_oriented(tri)
    v = mm.signed_volume(xyz, tri)
    want = 4.0 / 3.0 * np.pi * (3.6 * 0.25) ** 3
    assert v > 0 and abs(v - want) < 0.1 * want
    cx, ct = mm.mesh(mm.sphere(complement=True), 1.0)
    assert mm.is_closed_and_oriented(ct) and abs(mm.signed_volume(cx, ct) + v) < 1e-3 * v
    # a random sign field inside a positive shell: closed as well (no ambiguous case, the face diagonals of neighbours agree)
    rv = random_volume((10, 9, 8), 7, p_invalid=0.0)
    shell = np.ones(rv["tsdf"].shape, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    rv["tsdf"][shell] = 0.5
    rx, rt = mm.mesh(rv, 1.0)
    assert len(rt) > 500 and mm.is_closed_and_oriented(rt)
    # and an open one is told apart
    assert not mm.is_closed_and_oriented(tri[1:])


def test_ply_bytes_and_refusals(tmp_path):
    xyz, tri = mm.mesh(mm.sphere(8, 2.3), 1.0)
    assert len(tri) > 50
    a, b = str(tmp_path / "lib.ply"), str(tmp_path / "model.ply")
    binding.write_ply_mesh(a, xyz, tri)
    mm.write_ply(b, xyz, tri)
    got = open(a, "rb").read()
    assert got == open(b, "rb").read() and len(got) == got.index(b"end_header\n") + 11 + 12 * len(xyz) + 13 * len(tri)
    # empty meshes: a header and nothing else
    binding.write_ply_mesh(a, np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    mm.write_ply(b, np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    assert open(a, "rb").read() == open(b, "rb").read()
    binding.write_ply_mesh(a, xyz, np.zeros((0, 3), np.int32))
    assert len(open(a, "rb").read()) == len(open(a, "rb").read().split(b"end_header\n")[0]) + 11 + 12 * len(xyz)
    # refusals: an index outside [0, nv) leaves no file behind; a path that cannot be written is the I/O error
    L, fp, ip = binding.host_lib(), binding.c_fp, binding.c_ip
    fresh = str(tmp_path / "never.ply")
    for bad in (len(xyz), -1):
        t = tri.copy()
        t[len(t) // 2, 1] = bad
        assert L.nalo_io_write_ply_mesh(fresh.encode(), len(xyz), xyz.ctypes.data_as(fp), len(t), t.ctypes.data_as(ip)) == -1 and not os.path.exists(fresh)
    assert L.nalo_io_write_ply_mesh(fresh.encode(), 0, None, 1, tri.ctypes.data_as(ip)) == -1                    # a triangle without vertices
    assert L.nalo_io_write_ply_mesh(None, 0, None, 0, None) == -1 and L.nalo_io_write_ply_mesh(fresh.encode(), -1, None, 0, None) == -1
    assert L.nalo_io_write_ply_mesh(fresh.encode(), 2, None, 0, None) == -1 and L.nalo_io_write_ply_mesh(fresh.encode(), 0, None, 2, None) == -1
    assert not os.path.exists(fresh)
    assert L.nalo_io_write_ply_mesh(str(tmp_path / "no_such_dir" / "m.ply").encode(), len(xyz), xyz.ctypes.data_as(fp), len(tri), tri.ctypes.data_as(ip)) == -2
    with pytest.raises(binding.NaloError):
        binding.write_ply_mesh(str(tmp_path / "no_such_dir" / "m.ply"), xyz, tri)


SAN_MAIN = r'''
#include <cstdio>
#include <cstring>
#include "nalo_gpu.h"
#include "nalo_io.h"
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    signed char tab[6][16][6];
    std::memset(tab, 77, sizeof tab);
    int bad = nalo_tsdf_mesh_table(tab) != 0;
    bad += nalo_tsdf_mesh_table(nullptr) != NALO_ERR_ARG;
    int ntri = 0;
    for (int t = 0; t < 6; ++t)
        for (int m = 0; m < 16; ++m)
            for (int k = 0; k < 6; ++k) {
                const int c = tab[t][m][k];
                if (c < -1 || c > 55 || (c >= 0 && (c & 7) == 0)) ++bad;
                if (c >= 0 && k % 3 == 0) ++ntri;
            }
    std::printf("triangles %d\n", ntri);
    char path[4096];
    const float xyz[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    int tri[6] = {0, 1, 2, 2, 1, 0};
    std::snprintf(path, sizeof path, "%s/empty.ply", argv[1]);
    std::printf("empty %d\n", nalo_io_write_ply_mesh(path, 0, nullptr, 0, nullptr));
    std::snprintf(path, sizeof path, "%s/points.ply", argv[1]);
    std::printf("points %d\n", nalo_io_write_ply_mesh(path, 3, xyz, 0, nullptr));
    std::snprintf(path, sizeof path, "%s/two.ply", argv[1]);
    std::printf("two %d\n", nalo_io_write_ply_mesh(path, 3, xyz, 2, tri));
    std::snprintf(path, sizeof path, "%s/bad.ply", argv[1]);
    tri[4] = 3;
    std::printf("past %d\n", nalo_io_write_ply_mesh(path, 3, xyz, 2, tri));
    tri[4] = -2147483647 - 1;
    std::printf("negative %d\n", nalo_io_write_ply_mesh(path, 3, xyz, 2, tri));
    tri[4] = 2147483647;
    std::printf("huge %d\n", nalo_io_write_ply_mesh(path, 3, xyz, 2, tri));
    tri[4] = 0;
    std::printf("no vertices %d\n", nalo_io_write_ply_mesh(path, 0, nullptr, 2, tri));
    std::printf("null %d %d\n", nalo_io_write_ply_mesh(nullptr, 0, nullptr, 0, nullptr), nalo_io_write_ply_mesh(path, 3, nullptr, 2, tri));
    std::snprintf(path, sizeof path, "%s/no_such_dir/m.ply", argv[1]);
    std::printf("dir %d\n", nalo_io_write_ply_mesh(path, 3, xyz, 2, tri));
    return bad;
}
'''


def test_table_and_ply_writer_under_the_sanitizers(tmp_path):
    """host_tsdf.cpp and host_io.cpp are plain C++: built with a main of its own under -fsanitize=address,undefined, the table and the PLY writer run clean on
    empty meshes, a mesh of two triangles and indices outside the vertices"""
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "tsdf_mesh_san"
    csrc = os.path.join(ROOT, "nalo-slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(src), os.path.join(csrc, "host_tsdf.cpp"), os.path.join(csrc, "host_io.cpp"), "-lz", "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr
    assert p.stdout.split("\n")[:-1] == ["triangles 120", "empty 0", "points 0", "two 0", "past -1", "negative -1", "huge -1", "no vertices -1", "null -1 -1", "dir -2"]
    assert not os.path.exists(tmp_path / "bad.ply")
    two = open(tmp_path / "two.ply", "rb").read()
    mm.write_ply(str(tmp_path / "model.ply"), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2], [2, 1, 0]], np.int32))
    assert two == open(tmp_path / "model.ply", "rb").read()
