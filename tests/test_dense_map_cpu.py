"""tests/dense_map_model.py on hand-worked inputs: the semantics nalo_dense_update_map and the dense archive's consumers are held to
(tests/test_dense_map_gpu.py). No device."""
import numpy as np

import dense_map_model as dm
import map_model as mm
import plane_model as pm
from nalo_slam_amd import binding

F = np.float32
K = (16.0, 16.0, 8.0, 6.0)
W, H = 16, 12
C2W = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def tiny():
    """16x12: value 5 on rows 3..5 x cols 3..7 (four points on the wall Z = 2), value 9 on rows 6..9 x cols 8..12 (three points), value 0 elsewhere"""
    mask = np.zeros((H, W), F)
    mask[3:6, 3:8] = 5
    mask[6:10, 8:13] = 9
    img = np.arange(W * H, dtype=F).reshape(H, W)
    bgr = np.stack([np.arange(W * H) % 251, np.arange(W * H) % 13, np.arange(W * H) % 7], 1).astype(np.uint8).reshape(H, W, 3)
    u = np.array([3, 7, 3, 7, 8, 12, 9], F) + F(0.25)
    v = np.array([3, 3, 5, 5, 6, 6, 9], F) + F(0.5)
    return mask, img, bgr, u, v, np.full(7, 0.5, F)


def test_two_clusters_by_hand():
    mask, img, bgr, u, v, idp = tiny()
    r = dm.update_map(u, v, idp, mask, img, bgr, W, H, K, pm.make_draws(1), C2W, min_points=3)
    assert [float(c["mask_value"]) for c in r["clusters"]] == [5.0, 9.0] and all(c["fitted"] for c in r["clusters"])
    a, b = r["runs"]
    assert a["rect"] == [3, 7, 3, 5] and b["rect"] == [8, 12, 6, 9]
    # rows [miny, maxy) x columns [minx, maxx) with i % 3 == 0 || j % 3 == 0, raster order; cluster order first
    want = [(3, 3), (4, 3), (5, 3), (6, 3), (3, 4), (6, 4)] + [(8, 6), (9, 6), (10, 6), (11, 6), (9, 7), (9, 8)]
    got = list(zip(r["points"]["u"].tolist(), r["points"]["v"].tolist()))
    assert got == want
    assert (a["n"], a["accept"], a["first"], b["n"], b["accept"], b["first"]) == (6, 1, 0, 6, 1, 6)
    assert np.allclose(r["points"]["idepth"], 0.5, rtol=1e-5)
    assert np.array_equal(r["points"]["color"], np.array([img[y, x] for x, y in want], F))
    assert np.array_equal(r["points"]["bgr"], np.array([bgr[y, x] for x, y in want], np.uint8))


def test_own_pixels_on_the_max_row_and_column_are_excluded():
    mask, img, bgr, u, v, idp = tiny()
    r = dm.update_map(u, v, idp, mask, img, bgr, W, H, K, pm.make_draws(1), C2W, min_points=3)
    assert mask[5, 3] == 5 and mask[3, 7] == 5 and 5 % 3 != 0 and mask[6, 12] == 9 and 12 % 3 == 0       # (12, 6) is a candidate of the cluster's own colour
    pts = set(zip(r["points"]["u"].tolist(), r["points"]["v"].tolist()))
    assert not any(x == 7 or y == 5 for x, y in pts if x < 8) and (12, 6) not in pts and not any(y == 9 for x, y in pts)


def test_mask_value_zero_gets_its_box_only():
    mask, img, bgr, u, v, idp = tiny()
    u = np.concatenate([u, F([4, 12, 5, 10, 11]) + F(0.5)])
    v = np.concatenate([v, F([8, 3, 7, 4, 3]) + F(0.5)])
    r = dm.update_map(u, v, np.full(len(u), 0.5, F), mask, img, bgr, W, H, K, pm.make_draws(2), C2W, min_points=3)
    k = [float(c["mask_value"]) for c in r["clusters"]].index(0.0)
    assert r["clusters"][k]["fitted"] and r["runs"][k]["rect"] == [2, 13, 2, 9] and r["runs"][k]["n"] == 0 and r["runs"][k]["first"] == -1
    assert len(r["points"]["u"]) == 12                              # the other two appended as before


def test_unfitted_cluster_is_passed_over():
    mask, img, bgr, u, v, idp = tiny()
    r = dm.update_map(u, v, idp, mask, img, bgr, W, H, K, pm.make_draws(1), C2W, min_points=4)
    assert [c["fitted"] for c in r["clusters"]] == [1, 0]
    assert r["runs"][1] == dict(rect=[0, 0, 0, 0], n=0, accept=0, first=-1) and len(r["points"]["u"]) == 6


def test_far_plane_is_rejected_and_appends_nothing():
    mask = np.zeros((48, 64), F)
    mask[10:40, 5:60] = 7
    img, bgr = np.ones((48, 64), F), np.zeros((48, 64, 3), np.uint8)
    far = dm.make_map(mask, img, bgr, 64, 48, (40.0, 40.0, 31.5, 23.5), F([0.0, 0.02, 1.0, -60.0]), 7.0, dm.bbox(mask, 64, 48, 7.0), C2W)
    near = dm.make_map(mask, img, bgr, 64, 48, (40.0, 40.0, 31.5, 23.5), F([0.0, 0.0, 1.0, -2.0]), 7.0, dm.bbox(mask, 64, 48, 7.0), C2W)
    assert far["n"] == near["n"] > 300 and far["accept"] == 0 and near["accept"] == 1


def test_cloud_by_hand():
    ci = F([0.5, 0.25, -1.0, -2.0])
    u, v = np.array([4, 6, 8, 10], np.uint16), np.array([8, 8, 12, 12], np.uint16)
    idp = F([0.5, -1.0, np.nan, 2.0])
    bgr = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], np.uint8)
    xyz, rgb = dm.refresh_pc(u, v, idp, bgr, ci)
    assert len(xyz) == 3                                            # the negative one is skipped, the NaN one stays (NaN < 0 is false)
    assert np.array_equal(xyz[0], F([2.0, 0.0, 2.0])) and np.isnan(xyz[1]).all() and np.array_equal(xyz[2], F([2.0, 0.5, 0.5]))
    assert rgb.tolist() == [[3, 2, 1], [9, 8, 7], [12, 11, 10]]
    # the draw index is the output index: the survivor behind the skipped point takes draws[1], not draws[2]
    draws = np.array([dm.RAND_MAX, 0, dm.RAND_MAX, 12345], np.int32)
    xyz2, _ = dm.refresh_pc(u, v, idp, bgr, ci, draws)
    assert xyz2[0][2] == F(2.0) * (F(1) + F(2) * F(0.5) * F(0.5)) and xyz2[2][2] == F(0.5) * (F(1) + F(2) * F(0.5) * (F(1.0) - F(0.5)))
    assert np.array_equal(xyz2[:, :2][[0, 2]], xyz[:, :2][[0, 2]])


def test_fast_cloud_equals_the_literal_one():
    rng = np.random.RandomState(3)
    n = 3000
    u, v = rng.randint(0, 1224, n).astype(np.uint16), rng.randint(0, 368, n).astype(np.uint16)
    idp = rng.uniform(-0.2, 2.0, n).astype(F)
    idp[::97] = np.nan; idp[5::131] = np.inf; idp[7::113] = F(1e-40); idp[11::127] = 0
    bgr = rng.randint(0, 256, (n, 3)).astype(np.uint8)
    ci = F([1 / 718.856, 1 / 718.856, -607.19 / 718.856, -185.2 / 718.856])
    draws = rng.randint(0, 2 ** 31 - 1, n).astype(np.int32)
    for d in (None, draws):
        a, b = dm.refresh_pc(u, v, idp, bgr, ci, d), dm.refresh_pc_fast(u, v, idp, bgr, ci, d)
        assert mm.bits_equal(a[0], b[0])
        assert np.array_equal(a[1], b[1]) and 0 < len(a[0]) < n


def test_world_points_equal_the_shared_host_function():
    import ctypes as C
    rng = np.random.RandomState(4)
    n = 200
    u, v = rng.randint(0, 640, n).astype(F), rng.randint(0, 480, n).astype(F)
    idp = rng.uniform(-0.5, 2.0, n).astype(F)
    ci = F([1 / 500.0, 1 / 510.0, -0.64, -0.47])
    m = np.concatenate([np.linalg.qr(rng.randn(3, 3))[0], [[2.5e6], [-8e5], [42.0]]], 1)
    lib = C.CDLL(binding.lib_path())
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    out = np.zeros((n, 3))
    mc = np.ascontiguousarray(m.ravel())
    assert lib.nalo_map_world_points_host(n, u.ctypes.data_as(fp), v.ctypes.data_as(fp), idp.ctypes.data_as(fp), ci.ctypes.data_as(fp), mc.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    assert np.array_equal(out.view(np.uint64), dm.world_points(u, v, idp, ci, m).view(np.uint64))


def test_binding_lists_the_dense_map_entry_points():
    for s in ("nalo_dense_update_map", "nalo_map_dense_enable", "nalo_map_dense_counts", "nalo_map_dense_get", "nalo_map_dense_world_points", "nalo_map_dense_cloud"):
        assert s in binding.EXPORTS
    assert binding.DENSE_POINT_DTYPE.itemsize == 16 and binding.DENSE_RUN_DTYPE.itemsize == 32
