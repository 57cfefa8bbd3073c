"""tests/map_model.py on hand-worked inputs (no device): every clause of refreshPC's filter on both sides of its threshold, the double-precision + 0.01,
inverse depths of 0, below 0 and NaN, the colour conversion, the display modes, the draw indexing, the push-backs and addPoint's rewrite, and the world
points against the library's host function (the arithmetic nalo_map_world_points shares)."""
import ctypes as C

import numpy as np

import map_model as mm
from nalo_slam_amd import binding

f32, f64 = np.float32, np.float64
CI = mm.calib_inverse([500.0, 400.0, 320.0, 240.0])


def rec(idepth=0.5, H=100.0, bs=1.0, status=1, u=100.0, v=50.0, color=None):
    r = np.zeros(1, mm.RECORD)
    r["u"], r["v"], r["idepth"], r["idepth_hessian"], r["maxRelBaseline"], r["status"] = u, v, idepth, H, bs, status
    r["color"] = np.arange(8) * 10 if color is None else color
    return r


def n_out(r, scaledTH=1e10, absTH=1e10, mode=1, minBS=0.0, draws=None):
    return len(mm.refresh_pc(r, scaledTH, absTH, mode, minBS, CI, draws)[0])


def test_pattern_and_constants_are_the_librarys():
    k = binding.constants()
    assert [(k["patternP[%d].x" % i], k["patternP[%d].y" % i]) for i in range(8)] == [tuple(p) for p in mm.PATTERN.tolist()]
    assert k["setting_idepthFixPrior"] == mm.IDEPTH_FIX_PRIOR and k["setting_idepthFixPriorMargFac"] == mm.IDEPTH_FIX_PRIOR_MARG_FAC and k["SCALE_IDEPTH"] == 1
    assert binding.MAP_RECORD_DTYPE == mm.RECORD


def test_each_filter_clause_on_both_sides():
    r = rec(idepth=0.5, H=100.0, bs=0.25)                        # depth 2, depth4 16, var = float(1 / 100.01)
    var = f32(f64(1.0) / (f64(f32(100.0)) + f64(0.01)))
    assert n_out(r) == 8
    assert n_out(r, scaledTH=var * f32(16)) == 8 and n_out(r, scaledTH=np.nextafter(var * f32(16), f32(0))) == 0        # var * depth4 > scaledTH skips, == keeps
    assert n_out(r, absTH=var) == 8 and n_out(r, absTH=np.nextafter(var, f32(0))) == 0
    assert n_out(r, minBS=0.25) == 8 and n_out(r, minBS=np.nextafter(f32(0.25), f32(1))) == 0                           # relObsBaseline < minRelBS skips
    assert n_out(rec(status=0), mode=1) == 0 and n_out(rec(status=3), mode=1) == 0 and n_out(rec(status=2), mode=1) == 8
    assert n_out(rec(status=2), mode=2) == 0 and n_out(rec(status=1), mode=2) == 8
    assert all(n_out(rec(status=s), mode=0) == 8 and n_out(rec(status=s), mode=3) == 0 for s in range(4))


def test_the_literal_is_a_double():
    H = f32(50.0)
    var_d, var_f = f32(f64(1.0) / (f64(H) + f64(0.01))), f32(1) / (H + f32(0.01))
    assert var_d < var_f                                         # the float sum rounds 50.01 down: one ulp apart in var
    assert n_out(rec(H=H), absTH=var_d) == 8                     # a float-only model would skip this record


def test_inverse_depth_zero_negative_nan():
    assert n_out(rec(idepth=-1e-6)) == 0
    assert n_out(rec(idepth=-0.0)) == 0                          # -0 < 0 is false; depth = -inf, depth4 = inf: the scaled test skips it
    xyz = mm.refresh_pc(rec(idepth=0.0), 1e10, 1e10, 1, 0.0, CI)[0]
    assert len(xyz) == 0                                         # depth = inf, var * inf = inf > scaledTH
    xyz, rgb, nrec, nsur = mm.refresh_pc(rec(idepth=np.nan, status=0, H=1000.0, bs=0.0), 1e-3, 1e-2, 0, 0.0, CI)
    assert len(xyz) == 8 and np.isnan(xyz).all() and nsur.tolist() == [1, 0, 0, 0]      # every comparison with NaN is false: the record passes
    assert rgb.tolist() == [[0, 255, 255]] * 8


def test_colours():
    col = [-5.0, -0.5, 0.0, 0.99, 17.9, 255.0, 300.0, np.nan]
    rgb = mm.refresh_pc(rec(color=col), 1e10, 1e10, 1, 0.0, CI)[1]
    assert rgb[:, 0].tolist() == [0, 0, 0, 0, 17, 255, 255, 0] and (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 0] == rgb[:, 2]).all()
    for s, c in ((0, [0, 255, 255]), (1, [0, 255, 0]), (2, [0, 0, 255]), (3, [255, 0, 0])):
        assert mm.refresh_pc(rec(status=s, color=col), 1e10, 1e10, 0, 0.0, CI)[1].tolist() == [c] * 8


def test_vertices_and_draw_indexing():
    r = np.concatenate([rec(u=10.0, v=20.0, idepth=0.25), rec(idepth=-1.0), rec(u=30.0, v=40.0, idepth=2.0)])
    draws = np.arange(24, dtype=np.int64) * 89478485                       # one per possible vertex; the skipped record consumes none
    xyz = mm.refresh_pc(r, 1e10, 1e10, 1, 0.0, CI, draws)[0]
    assert xyz.shape == (16, 3)
    fxi, fyi, cxi, cyi = CI
    for k, (u, v, d) in enumerate(((10.0, 20.0, 4.0), (30.0, 40.0, 0.5))):
        for pnt in range(8):
            j = 8 * k + pnt
            dx, dy = mm.PATTERN[pnt]
            jit = f32(f32(draws[j]) / f32(2147483647)) - f32(0.5)
            want = [f32(f32(f32(f32(u + dx) * fxi) + cxi) * f32(d)), f32(f32(f32(f32(v + dy) * fyi) + cyi) * f32(d)), f32(f32(d) * f32(f32(1) + f32(f32(f32(2) * fxi) * jit)))]
            assert mm.bits_equal(xyz[j], np.array(want, f32)), (j, xyz[j], want)
    flat = mm.refresh_pc(r, 1e10, 1e10, 1, 0.0, CI, None)[0]
    assert mm.bits_equal(flat[:, 2], np.repeat(np.array([4.0, 0.5], f32), 8)) and mm.bits_equal(flat[:, :2], xyz[:, :2])
    assert mm.bits_equal(mm.refresh_pc(r, 1e10, 1e10, 1, 0.0, CI, np.full(24, 1 << 30))[0], flat)      # r / RAND_MAX == 0.5f: the bracket is exactly 1


def test_push_backs_and_add_point():
    host = np.array([0, 1, 0, 1, 0, 0])
    dec = np.array([3, 3, 0, 2, 1, 3])
    H = np.array([60, 70, 80, 10, 0, 90], f32)
    rb = np.array([.1, .2, .3, .4, .5, .6], f32)
    Hdd_post = np.array([5, 1e-12, 0, 0, 0, 7], f32)
    HdiF_post = np.array([0.2, 1e10, 0, 0, 0, 0], f32)                     # point 5: no active residual after the re-linearisation
    pr = np.array([1, 0, 0, 0, 0, 1])
    out = mm.flag_points_push(host, [10, 11], np.arange(6), np.arange(6) + 10, np.full(6, 0.5), np.zeros((6, 8)), dec, H, rb, Hdd_post, HdiF_post, pr)
    m0, o0 = out[10]
    m1, o1 = out[11]
    assert m0["u"].tolist() == [0, 5] and o0["u"].tolist() == [4] and m1["u"].tolist() == [1] and o1["u"].tolist() == [3]
    assert m0["idepth_hessian"].tolist() == [f32(5) + f32(2500) * f32(360000), 0] and m0["maxRelBaseline"].tolist() == [f32(.1), 0]
    assert m1["idepth_hessian"].tolist() == [f32(1e-10)] and m1["maxRelBaseline"].tolist() == [f32(.2)]
    assert o0["idepth_hessian"].tolist() == [0] and o1["idepth_hessian"].tolist() == [10] and o0["decision"].tolist() == [1] and o1["decision"].tolist() == [2]
    assert (m0["status"] == 2).all() and (o1["status"] == 3).all() and (m0["frame_id"] == 10).all() and (o1["frame_id"] == 11).all()
    allr = mm.set_from_kf(dict(u=[1.0], v=[2.0], idepth_min=[0.0], idepth_max=[np.nan], color=np.zeros((1, 8))), m0[:0], m0, o0)
    assert allr["status"].tolist() == [0, 2, 2, 3] and np.isnan(allr["idepth"][0]) and allr["idepth_hessian"][0] == 1000


def test_world_points_are_the_pcd_writers(tmp_path):
    rng = np.random.RandomState(3)
    n = 500
    u, v = rng.uniform(0, 640, n).astype(f32), rng.uniform(0, 480, n).astype(f32)
    idp = rng.uniform(0.01, 3, n).astype(f32)
    idp[:3] = [0.0, -0.5, np.nan]
    m = np.concatenate([np.linalg.qr(rng.randn(3, 3))[0], [[1e6 + 0.123], [-3e5], [7.0]]], 1)
    lib = C.CDLL(binding.lib_path())
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    got = np.zeros((n, 3))
    mc = np.ascontiguousarray(m.ravel())
    assert lib.nalo_map_world_points_host(n, u.ctypes.data_as(fp), v.ctypes.data_as(fp), idp.ctypes.data_as(fp), CI.ctypes.data_as(fp), mc.ctypes.data_as(dp), got.ctypes.data_as(dp)) == 0
    assert mm.bits_equal(got, mm.world_points(u, v, idp, CI, m))
    # and they are the numbers the PCD writer formats (default stream precision: %g)
    path = str(tmp_path / "pcl.pcd")
    assert lib.nalo_io_write_pcd_points(path.encode(), 0, n, u.ctypes.data_as(fp), v.ctypes.data_as(fp), idp.ctypes.data_as(fp), CI.ctypes.data_as(fp), mc.ctypes.data_as(dp)) == 0
    lines = open(path).read().splitlines()
    fin = np.isfinite(got).all(1)
    assert len(lines) == n and fin.sum() >= n - 3
    assert [lines[i] for i in np.nonzero(fin)[0]] == ["%g %g %g" % tuple(got[i]) for i in np.nonzero(fin)[0]]
