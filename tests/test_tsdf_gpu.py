"""The TSDF volume on the device (nalo_tsdf_*, include/nalo_gpu.h) against tests/tsdf_model.py. Every comparison is bit for bit: the definition contains only
correctly rounded float operations. The model evaluates EVERY voxel, the device only the culling box: equality is what shows the box to be conservative."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import tsdf_model as tm
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4
W0, H0 = 64, 48
K0 = (70.0, 68.0, 31.5, 23.5)
POSES = [EYE, pose(0.15, -0.25, 0.1, (0.2, -0.1, 0.15)), pose(-0.3, 0.35, 1.2, (-0.25, 0.2, -0.1))]
# the two grids: a partial workgroup along x (8 groups of four in 32), and an x extent that is no multiple of four under rows whose start is odd (33 x 17)
GRIDS = [dict(origin=(-1.2, -0.9, 0.9), vs=0.075, dims=(32, 24, 40), trunc=0.25, mw=4.0), dict(origin=(-0.7, -0.5, 1.85), vs=0.055, dims=(33, 17, 5), trunc=0.2, mw=4.0)]


def ctx(w=W0, h=H0, K=K0):
    return binding.Context(w, h, K, n_slots=1)


def make(c, g):
    c.tsdf_create(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    return tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])


def bits_eq(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def assert_volume(c, vol, tag=""):
    t, w = c.tsdf_get()
    assert bits_eq(t, vol["tsdf"]) and bits_eq(w, vol["weight"]), tag


def integrate_both(c, vol, depth, K, c2w, mn, mx, dev=None, tag=""):
    """one integration on the device (from `dev`, or a fresh contiguous tensor of depth) and in the model; box, counts and both arrays must agree"""
    d = torch.from_numpy(np.ascontiguousarray(depth)).cuda() if dev is None else dev
    c.tsdf_integrate_depth(d, K, c2w, mn, mx)
    r = tm.integrate(vol, depth, K, c2w, mn, mx)
    st = c.tsdf_last()
    h, w = depth.shape
    lo, hi = tm.frustum_box(vol, w, h, K, c2w, mx)
    assert (st["lo"], st["hi"]) == (lo, hi), (tag, st, lo, hi)
    assert st["visited"] == (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) and st["updated"] == r["updated"], (tag, st, r["updated"])
    box = tm.updated_box(r["code"])
    assert box is None or all(lo[a] <= box[0][a] and box[1][a] <= hi[a] for a in range(3)), tag
    assert_volume(c, vol, tag)
    return r, st


# ------------------------------------------------------------------------------------------------ integration against the model
@pytest.fixture(scope="module")
def fused():
    """both grids after the three poses (and a second round of them): (context, model volume) pairs the surface tests read"""
    out = []
    for gi, g in enumerate(GRIDS):
        c = ctx()
        vol = make(c, g)
        assert_volume(c, vol, "initial values")
        n = 0
        for rnd in range(2):
            for pi, c2w in enumerate(POSES):
                depth = wavy_depth(W0, H0, 10 * gi + pi, base=2.0 + 0.02 * rnd)
                r, st = integrate_both(c, vol, depth, K0, c2w, 0.5, 3.5, tag=(gi, rnd, pi))
                n += r["updated"]
                assert st["visited"] > 0
        assert n > 2000 and vol["weight"].max() > 2
        out.append((c, vol, g))
    yield out
    for c, _, _ in out:
        c.close()


def test_integration_equals_the_model(fused):
    (c0, v0, _), (c1, v1, _) = fused
    assert v0["weight"].max() == 4.0                                           # six integrations of overlapping views saturate max_weight = 4
    for c, vol in ((c0, v0), (c1, v1)):
        assert_volume(c, vol)


def test_box_whose_x_start_is_odd():
    """the camera is moved so that the culling box starts at an odd x: rows then begin 1, 2 or 3 voxels into a group of four (33 voxels a row) and end inside one"""
    g = GRIDS[1]
    seen = set()
    c = ctx()
    vol = make(c, g)
    for k, tx in enumerate((0.9, 0.93, 0.96, 0.99, 1.02, 1.05, -0.6, -0.63)):
        c2w = pose(0, 0, 0, (tx, 0.0, 0.0))
        r, st = integrate_both(c, vol, wavy_depth(W0, H0, 40 + k), (200.0, 200.0, 31.5, 23.5), c2w, 0.5, 3.5, tag=tx)
        seen.add(st["lo"][0] % 4)
        assert r["updated"] > 0 and (st["lo"][0] > 0 or st["hi"][0] < 33)
    assert len(seen) >= 3 and seen & {1, 3}, seen
    c.close()


def planted(c2w):
    """a grid whose voxel centres are multiples of 0.25: x = -5 + 0.25 i, y = -1 + 0.25 j, z = -0.5 + 0.25 k; K so that uf = 8 x / z + 16, vf = 8 y / z + 8 on 32 x 16"""
    g = dict(origin=(-5.125, -1.125, -0.625), vs=0.25, dims=(40, 9, 12), trunc=0.5, mw=4.0)
    K = (8.0, 8.0, 15.5, 7.5)
    depth = np.full((16, 32), 1.5, F)
    # the voxels (i, j = 4, k = 6) lie at y = 0, z = 1: pixel (16 + 2 (i - 20), 8)
    plant = {20: 0.0, 21: -1.0, 22: np.nan, 23: np.inf, 24: 0.5, 25: 2.0, 26: np.nextafter(F(0.5), F(0)), 27: np.nextafter(F(2.0), F(3))}
    for i, dv in plant.items():
        depth[8, 16 + 2 * (i - 20)] = dv
    # (i = 20, j = 4, k = 7): z = 1.25 reads pixel (16, 8) too - planted 0 above; (i = 20, j = 3, k = 7): y = -0.25, vf = 6.4 -> pixel (16, 6)
    depth[6, 16] = np.nextafter(F(0.75), F(0))                                  # sdf just below -trunc at zc = 1.25
    return g, K, depth


def test_planted_voxels_and_pixels():
    g, K, depth = planted(EYE)
    c = ctx(32, 16, K)
    vol = make(c, g)
    r, st = integrate_both(c, vol, depth, K, EYE, 0.5, 2.0, tag="planted, identity")
    code, uf, zc, sdf = r["code"], r["uf"], r["zc"], r["sdf"]
    assert st["lo"] == (0, 0, 1) and st["hi"][0] == 40                          # the whole x range is visited: the overflowing voxels below are evaluated on the device
    # uf exactly 0 is inside, exactly w is outside (x = -2 and x = 2 at z = 1)
    assert uf[6, 4, 12] == 0.0 and code[6, 4, 12] == tm.UPDATED and uf[6, 4, 28] == 32.0 and code[6, 4, 28] == tm.OUTSIDE
    # zc exactly 0 (k = 2) and negative (k = 0, 1)
    assert (zc[2] == 0).all() and (code[2] == tm.BEHIND).all() and (zc[:2] < 0).all() and (code[:2] == tm.BEHIND).all()
    # depth 0, negative, NaN, +inf, just outside either bound: no depth; exactly min_depth and exactly max_depth: integrated
    assert [int(code[6, 4, i]) for i in (20, 21, 22, 23, 26, 27)] == [tm.NO_DEPTH] * 6 and [int(code[6, 4, i]) for i in (24, 25)] == [tm.UPDATED] * 2
    # sdf exactly -trunc (depth 0.5 at zc 1): integrated with d = -1; just below -trunc: occluded; exactly trunc (depth 1.5 at zc 1): d = 1
    assert sdf[6, 4, 24] == -0.5 and vol["tsdf"][6, 4, 24] == -1.0
    assert sdf[7, 3, 20] < -0.5 and sdf[7, 3, 20] > -0.5000001 and code[7, 3, 20] == tm.OCCLUDED
    assert sdf[6, 4, 19] == 0.5 and code[6, 4, 19] == tm.UPDATED and vol["tsdf"][6, 4, 19] == 1.0
    assert sdf[6, 4, 25] == 1.0 and vol["tsdf"][6, 4, 25] == 1.0                  # fminf(1, 2)
    # an xc / zc that overflows: the camera 2^-126 behind the plane z = 0, so that zc = 2^-126 on k = 2 and x / zc = x 2^126 is infinite from |x| = 4 on
    tz = -math.ldexp(1.0, -126)
    c2w = pose(0, 0, 0, (0, 0, tz))
    r, st = integrate_both(c, vol, depth, K, c2w, 0.5, 2.0, tag="planted, overflow")
    assert r["zc"][2, 4, 0] == F(-tz) and np.isinf(r["xq"][2, 4, 0]) and np.isinf(r["xq"][2, 4, 39]) and np.isfinite(r["xq"][2, 4, 8])
    vis = np.zeros(r["code"][2].shape, bool)
    vis[4, 20] = True                                                           # x = y = 0 projects to the principal point whatever zc is; its pixel holds the planted 0
    assert (r["code"][2][~vis] == tm.OUTSIDE).all() and r["code"][2, 4, 20] == tm.NO_DEPTH
    assert st["lo"][0] == 0 and st["hi"][0] == 40 and st["lo"][2] <= 2
    c.close()


def test_box_inside_the_grid_leaves_its_outside_untouched():
    """a narrow view into a large grid: every face of the culling box is interior, the voxels beyond every face keep their planted (non-initial) values, and
    voxels inside it change"""
    g = dict(origin=(-1.5, -1.5, 0.0), vs=0.1, dims=(30, 30, 36), trunc=0.2, mw=4.0)
    K = (160.0, 160.0, 31.5, 23.5)
    c = ctx()
    vol = make(c, g)
    rng = np.random.RandomState(5)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["weight"][:] = rng.randint(0, 3, vol["weight"].shape)
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    before = vol["tsdf"].copy()
    c2w = pose(0.05, -0.04, 0.3, (0.1, -0.05, 0.55))
    depth = np.full((H0, W0), 1.9, F)
    r, st = integrate_both(c, vol, depth, K, c2w, 0.5, 2.0, tag="interior box")
    lo, hi = st["lo"], st["hi"]
    assert all(0 < lo[a] and hi[a] < g["dims"][a] for a in range(3)), st
    inside = np.zeros(vol["tsdf"].shape, bool)
    inside[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    t, _ = c.tsdf_get()
    assert bits_eq(t[~inside], before[~inside]) and r["updated"] > 200 and not bits_eq(t[inside], before[inside])
    c.close()


def test_weight_saturation_and_two_interleaved_frames():
    g = GRIDS[1]
    c = ctx()
    vol = make(c, g)
    a, b = wavy_depth(W0, H0, 1), wavy_depth(W0, H0, 2, base=2.1)
    for _ in range(int(g["mw"]) + 2):                                           # max_weight + 2 integrations of one frame
        integrate_both(c, vol, a, K0, POSES[0], 0.5, 3.5)
    assert vol["weight"].max() == g["mw"] and (vol["weight"] == g["mw"]).sum() > 100
    c.tsdf_reset()
    vol = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    assert_volume(c, vol, "reset")
    for k in range(4):                                                          # a, b, a, b from two poses
        integrate_both(c, vol, (a, b)[k % 2], K0, POSES[k % 2], 0.5, 3.5)
    c.close()


def test_strided_views_and_a_plane_of_another_size():
    """a pitched region and an x-strided view of larger tensors whose other elements are usable depths that WOULD change the result if one were read; then a
    depth plane of 40 x 30 with its own K in a context of 64 x 48"""
    g = GRIDS[0]
    c = ctx()
    vol = make(c, g)
    depth = wavy_depth(W0, H0, 7)
    big = torch.full((H0 + 6, W0 + 10), 1.3, device="cuda")
    big[3:3 + H0, 5:5 + W0] = torch.from_numpy(depth).cuda()
    view = big[3:3 + H0, 5:5 + W0]
    assert not view.is_contiguous()
    integrate_both(c, vol, depth, K0, POSES[1], 0.5, 3.5, dev=view, tag="pitched")
    wide = torch.full((H0, 3 * W0), 1.3, device="cuda")
    wide[:, 1::3] = torch.from_numpy(depth).cuda()
    xs = wide[:, 1::3]
    assert xs.stride() == (3 * W0, 3)
    integrate_both(c, vol, depth, K0, POSES[2], 0.5, 3.5, dev=xs, tag="x-strided")
    small = wavy_depth(40, 30, 8)
    integrate_both(c, vol, small, (44.0, 42.0, 19.5, 14.5), POSES[0], 0.5, 3.5, tag="another size")
    # the control: the surroundings do matter to a reader that ignores the strides
    ctl = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    ctl2 = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    tm.integrate(ctl, depth, K0, POSES[1], 0.5, 3.5)
    tm.integrate(ctl2, big.cpu().numpy().reshape(-1)[:H0 * W0].reshape(H0, W0), K0, POSES[1], 0.5, 3.5)
    assert not bits_eq(ctl["tsdf"], ctl2["tsdf"])
    c.close()


# ------------------------------------------------------------------------------------------------ surface points, get / set, the views
def surface_both(c, vol, mw, lo=None, size=None):
    got = c.tsdf_surface_points(mw, lo, size)
    want = tm.surface_points(vol, mw, lo, size)
    assert got.shape == want.shape and bits_eq(got, want), (mw, lo, size, got.shape, want.shape)
    return got


def test_surface_points_of_the_fused_volumes(fused):
    for c, vol, g in fused:
        n = len(surface_both(c, vol, 1.0))
        assert n > 100 and len(surface_both(c, vol, 3.0)) < n
        nx, ny, nz = g["dims"]
        surface_both(c, vol, 1.0, (1, 2, 1), (nx - 3, ny - 5, nz - 2))
        surface_both(c, vol, 1.0, (nx - 1, 0, 0), (1, ny, nz))
        assert bits_eq(tm.surface_points(vol, 1.0), tm.surface_points_literal(vol, 1.0)) if nz == 5 else True
        # the cap protocol: too little room is refused with the need reported and nothing written; exactly enough is taken
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_surface_points(1.0, cap=n - 1)
        assert c.tsdf_surface_needed == n
        xyz = np.full((n - 1, 3), 7.0, F)
        a = binding.TsdfSurfaceArgs()
        a.min_weight, a.cap, a.xyz = 1.0, n - 1, xyz.ctypes.data_as(binding.c_fp)
        assert c.L.nalo_tsdf_surface_points(c.h_, C.byref(a)) == ERR_ARG and (a.n, a.n_needed) == (0, n) and (xyz == 7.0).all()
        assert len(c.tsdf_surface_points(1.0, cap=n + 5)) == n


def test_surface_points_of_planted_volumes():
    g = dict(origin=(-1.0, 0.5, 2.0), vs=0.125, dims=(37, 9, 31), trunc=0.25, mw=4.0)   # 10323 voxels: eleven workgroups of the compaction, the last one partial
    c = ctx()
    vol = make(c, g)
    assert len(surface_both(c, vol, 0.0)) == 0                                   # no crossing at all: tsdf is 1 everywhere (and weight 0 >= 0)
    rng = np.random.RandomState(3)
    T = rng.choice(np.array([-1.0, -0.25, 0.0, -0.0, 0.5, 1.0, np.nan], F), vol["tsdf"].shape).astype(F)
    Wt = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, np.nan], F), vol["weight"].shape).astype(F)
    vol["tsdf"][:], vol["weight"][:] = T, Wt
    c.tsdf_set((0, 0, 0), T, Wt)
    n = len(surface_both(c, vol, 1.0))
    assert n > 1000 and len(surface_both(c, vol, 0.5)) > n and len(surface_both(c, vol, np.nextafter(F(1.0), F(2)))) < n   # weights either side of min_weight
    for lo, size in (((0, 0, 0), (37, 9, 31)), ((0, 0, 0), (1, 1, 1)), ((36, 8, 30), (1, 1, 1)), ((0, 0, 0), (37, 1, 1)), ((0, 0, 0), (1, 9, 1)), ((0, 0, 0), (1, 1, 31)),
                     ((3, 2, 5), (30, 6, 20)), ((35, 7, 29), (2, 2, 2))):
        surface_both(c, vol, 1.0, lo, size)
    # crossings on every face of a sub-box and of the grid: a sign change across each face is a crossing of the grid's and none of the sub-box's
    vol["tsdf"][:], vol["weight"][:] = 1.0, 2.0
    vol["tsdf"][4:8, 2:5, 3:9] = -0.5
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    inner = len(surface_both(c, vol, 1.0, (3, 2, 4), (6, 3, 4)))
    assert inner == 0 and len(surface_both(c, vol, 1.0, (2, 1, 3), (8, 5, 6))) == 2 * (6 * 3 + 6 * 4 + 3 * 4)
    vol["tsdf"][:] = -0.5
    vol["tsdf"][1:-1, 1:-1, 1:-1] = 0.75
    c.tsdf_set((0, 0, 0), vol["tsdf"], None)
    assert len(surface_both(c, vol, 1.0)) == 2 * (35 * 7 + 35 * 29 + 7 * 29)
    # t0 == 0 and t1 == 0
    vol["tsdf"][:] = 1.0
    vol["tsdf"][10, 4, 10], vol["tsdf"][10, 4, 11], vol["tsdf"][10, 4, 12] = 0.0, -1.0, 0.0
    c.tsdf_set((0, 0, 0), vol["tsdf"], None)
    pts = surface_both(c, vol, 1.0)
    cs = tm.centres(vol)
    assert [cs[0][10], cs[1][4], cs[2][10]] in pts.tolist() and [cs[0][12], cs[1][4], cs[2][10]] in pts.tolist()
    c.close()


def test_get_set_round_trips_and_the_views():
    g = GRIDS[1]
    nx, ny, nz = g["dims"]
    c = ctx()
    vol = make(c, g)
    rng = np.random.RandomState(11)
    for lo, size in (((0, 0, 0), (3, 2, 2)), ((nx - 5, ny - 3, nz - 1), (5, 3, 1)), ((0, ny - 1, 0), (nx, 1, nz)), ((nx - 1, 0, nz - 2), (1, ny, 2)), ((7, 3, 1), (9, 5, 3))):
        t = rng.randint(0, 2 ** 32, size[::-1], dtype=np.uint64).astype(np.uint32).view(F)          # every bit pattern, NaN payloads among them
        w = rng.randint(0, 2 ** 32, size[::-1], dtype=np.uint64).astype(np.uint32).view(F)
        t.view(np.uint32).reshape(-1)[:2] = (0x7FC12345, 0xFFA00001)                # a quiet and a signalling NaN with payloads
        w.view(np.uint32).reshape(-1)[-1] = 0x7F800001
        c.tsdf_set(lo, t, w)
        sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
        vol["tsdf"][sl], vol["weight"][sl] = t, w
        gt, gw = c.tsdf_get(lo, size)
        assert bits_eq(gt, t) and bits_eq(gw, w)
        assert_volume(c, vol, (lo, size))
    assert np.isnan(vol["tsdf"]).sum() > 0
    vt, vw = c.tsdf_view()
    assert vt.shape == (nz, ny, nx) and vt.stream == c.L.nalo_stream(c.h_)
    c.sync()
    tt, tw = torch.as_tensor(vt, device="cuda"), torch.as_tensor(vw, device="cuda")
    assert tt.shape == (nz, ny, nx) and tt.data_ptr() == vt.ptr and tw.data_ptr() == vw.ptr
    assert bits_eq(tt.cpu().numpy(), vol["tsdf"]) and bits_eq(tw.cpu().numpy(), vol["weight"])
    tt[0, 0, 0] = 0.125                                                         # zero-copy: a write through the tensor is the volume's
    torch.cuda.synchronize()
    assert c.tsdf_get((0, 0, 0), (1, 1, 1))[0][0, 0, 0] == 0.125
    c.close()


# ------------------------------------------------------------------------------------------------ stream order
def test_stream_order_without_a_host_wait():
    """the depth tensor is produced behind at least 0.2 s of matmuls on a torch stream: the call returns while they run, integrates the right data, and with the
    release the tensor is overwritten on that stream right after"""
    g = GRIDS[1]
    c = ctx()
    vol = make(c, g)
    right = wavy_depth(W0, H0, 21)
    wrong = (right + F(0.7)).astype(F)
    d_right, d_wrong = torch.from_numpy(right).cuda(), torch.from_numpy(wrong).cuda()
    t = torch.empty_like(d_right)
    integrate_both(c, vol, wrong, K0, POSES[0], 0.5, 3.5)                       # steady state: the events exist
    a = torch.randn(4096, 4096, device="cuda")
    out = torch.empty_like(a)
    S = torch.cuda.Stream()
    try:
        with torch.cuda.stream(S):
            torch.mm(a, a, out=out)
            S.synchronize()
            t0 = time.perf_counter()
            torch.mm(a, a, out=out)
            S.synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
            reps = min(int(math.ceil(0.25 / one)) + 1, 20000)
            for release in (False, True):
                t.copy_(d_wrong)
                for _ in range(reps):
                    torch.mm(a, a, out=out)
                t.copy_(d_right)
                behind = torch.cuda.Event()
                behind.record(S)
                c.tsdf_integrate_depth(t, K0, POSES[1], 0.5, 3.5, release=release)     # stream=None: torch's current stream, S
                returned_early = not behind.query()
                if release:
                    t.fill_(1.9)                                                 # a usable depth, on S, directly after the call
                else:
                    c.tsdf_release(S.cuda_stream)
                    t.fill_(1.8)
                assert returned_early, "nalo_tsdf_integrate_depth waited for the producer stream (release=%s, %d matmuls of %.2e s)" % (release, reps, one)
                r = tm.integrate(vol, right, K0, POSES[1], 0.5, 3.5)
                assert c.tsdf_last()["updated"] == r["updated"]
                assert_volume(c, vol, ("stream order", release))
                S.synchronize()
    finally:
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ refusals
def state(c):
    t, w = c.tsdf_get()
    return t.tobytes(), w.tobytes(), repr(c.tsdf_last())


def depth_rc(c, plane, K=K0, c2w=EYE, mn=0.5, mx=3.5):
    a = binding.TsdfIntegrateArgs()
    a.depth = plane
    a.K[:] = K
    a.camToWorld[:] = [float(v) for v in np.asarray(c2w, np.float64).reshape(-1)]
    a.min_depth, a.max_depth = mn, mx
    return c.L.nalo_tsdf_integrate_depth(c.h_, C.byref(a))


def test_refusals_leave_volume_and_context():
    c = ctx()
    d = torch.from_numpy(wavy_depth(W0, H0, 30)).cuda()
    good = binding.dev_plane(d)
    # no volume
    assert depth_rc(c, good) == ERR_STATE and c.L.nalo_tsdf_reset(c.h_) == ERR_STATE and c.L.nalo_tsdf_release(c.h_, None) == ERR_STATE
    st = binding.TsdfStats()
    assert c.L.nalo_tsdf_last(c.h_, C.byref(st)) == ERR_STATE and c.L.nalo_tsdf_destroy(c.h_) == 0
    for fn in (lambda: c.tsdf_get((0, 0, 0), (1, 1, 1)), lambda: c.tsdf_view(), lambda: c.tsdf_surface_points(1.0), lambda: c.tsdf_integrate_frame(1, EYE, K0, 0.5, 3.5)):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
            fn()
    g = GRIDS[1]
    vol = make(c, g)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_last()                                                           # nothing integrated yet
    integrate_both(c, vol, wavy_depth(W0, H0, 30), K0, POSES[0], 0.5, 3.5)
    before = state(c)
    # each bad field of the volume's descriptor: the volume in place stays
    o, vs, dims, tr, mw = g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"]
    for bad in ((o, vs, (0, 17, 5), tr, mw), (o, vs, (33, 2049, 5), tr, mw), (o, vs, (33, 17, -1), tr, mw), (o, vs, (1024, 1024, 1024), tr, mw), (o, 0.0, dims, tr, mw), (o, np.nan, dims, tr, mw),
                (o, vs, dims, -0.1, mw), (o, vs, dims, np.inf, mw), (o, vs, dims, tr, 0.0), (o, vs, dims, tr, np.nan), ((0.0, np.inf, 0.0), vs, dims, tr, mw), ((np.nan, 0.0, 0.0), vs, dims, tr, mw)):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_create(*bad)
    assert state(c) == before
    # each bad field of the integration's arguments
    nan_pose = np.array(EYE)
    nan_pose[1, 2] = np.nan
    inf_pose = np.array(EYE)
    inf_pose[0, 3] = np.inf
    for kw in (dict(c2w=nan_pose), dict(c2w=inf_pose), dict(mn=2.0, mx=1.0), dict(mn=np.nan), dict(mx=np.inf), dict(K=(np.nan, 68.0, 31.5, 23.5)), dict(K=(70.0, 68.0, 31.5, np.inf))):
        assert depth_rc(c, good, **kw) == ERR_ARG, kw
    host = np.zeros((H0, W0), F)
    u8 = torch.zeros((H0, W0), dtype=torch.uint8, device="cuda")
    i32 = torch.zeros((H0, W0), dtype=torch.int32, device="cuda")
    rgb = torch.zeros((H0, W0, 3), device="cuda")
    for p in (binding.DevPlane(host.ctypes.data, binding.DT_F32, W0, H0, 1, 4 * W0, 4, 0), binding.dev_plane(u8), binding.dev_plane(i32), binding.dev_plane(rgb, "hwc"),
              binding.DevPlane(None, binding.DT_F32, W0, H0, 1, 4 * W0, 4, 0),
              binding.DevPlane(d.data_ptr(), binding.DT_F32, W0, H0, 1, 4 * W0, 2, 0)):
        assert depth_rc(c, p) == ERR_ARG
    assert c.L.nalo_tsdf_integrate_depth(c.h_, None) == ERR_ARG
    # get / set / surface: blocks that leave the grid, no array, a negative cap
    nx, ny, nz = dims
    one = np.zeros((1, 1, 1), F)
    for lo, size in (((-1, 0, 0), (1, 1, 1)), ((nx, 0, 0), (1, 1, 1)), ((0, 0, 0), (nx + 1, 1, 1)), ((0, 0, 0), (1, 0, 1)), ((0, ny - 1, 0), (1, 2, 1)), ((0, 0, nz - 1), (1, 1, 2))):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_get(lo, size)
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_surface_points(1.0, lo, size)
    lo_a, sz_a = np.zeros(3, np.int32), np.ones(3, np.int32)
    assert c.L.nalo_tsdf_set(c.h_, lo_a.ctypes.data_as(binding.c_ip), sz_a.ctypes.data_as(binding.c_ip), None, None) == ERR_ARG
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_set((nx, 0, 0), one, one)
    a = binding.TsdfSurfaceArgs()
    a.min_weight, a.cap = 1.0, -1
    assert c.L.nalo_tsdf_surface_points(c.h_, C.byref(a)) == ERR_ARG
    # the frame route: no dense archive here
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_integrate_frame(500, EYE, K0, 0.5, 3.5)
    assert state(c) == before
    # the next legal call works
    integrate_both(c, vol, wavy_depth(W0, H0, 31), K0, POSES[1], 0.5, 3.5)
    # a second create replaces the volume; destroy frees it
    vol = make(c, GRIDS[0])
    assert_volume(c, vol, "second create")
    integrate_both(c, vol, wavy_depth(W0, H0, 32), K0, POSES[2], 0.5, 3.5)
    c.tsdf_destroy()
    assert depth_rc(c, good) == ERR_STATE
    c.close()


# ------------------------------------------------------------------------------------------------ nalo_tsdf_integrate_frame
def frame_scene(w, h, shift=0.0):
    """three walls under three mask values (two of the boxes overlap, one region is a checkerboard) over a background that no point lies on; shift moves every
    wall back, so that a second nalo_dense_update_map of the same frame appends other depths at the same pixels"""
    import test_dense_map_gpu as tdm
    K = tdm.small_K(w, h) if w < 100 else (256.0, 256.0, 160.0, 120.0)
    yy, xx = np.mgrid[0:h, 0:w]
    s = w / 80.0
    regions = [dict(value=3.0, sel=tdm.rect_sel(w, h, 3, int(30 * h / 48), 3, int(38 * s)), n=40, kind="wall", par=2.0 + shift),
               dict(value=4.0, sel=tdm.rect_sel(w, h, int(10 * h / 48), h - 3, int(30 * s), int(60 * s)) & ((xx + yy) % 2 == 0), n=40, kind="wall", par=2.6 + shift),
               dict(value=6.0, sel=tdm.rect_sel(w, h, 3, h - 3, int(62 * s), w - 3), n=30, kind="wall", par=3.0 + shift)]
    return tdm.scene(w, h, K, regions, seed=w, background=1.0)


FRAME_GRID = dict(origin=(-1.1, -1.1, 3.5), vs=0.08, dims=(40, 30, 31), trunc=0.3, mw=8.0)      # around the walls as C2W places them: camera at (0.5, 0.1, 2), looking along +z


def frame_against_depth(c, fid, K, w, h, c2w, expect_points):
    """nalo_tsdf_integrate_frame into a fresh volume against nalo_tsdf_integrate_depth of the plane the model builds from nalo_map_dense_get, and the model itself"""
    pts = c.map_dense_get(fid)
    assert (len(pts) > 0) == expect_points
    with np.errstate(all="ignore"):
        D = tm.frame_plane(pts, w, h)
    c.tsdf_reset()
    c.tsdf_integrate_frame(fid, c2w, K, 0.5, 8.0)
    st_f, (t_f, w_f) = c.tsdf_last(), c.tsdf_get()
    c.tsdf_reset()
    vol = tm.volume(FRAME_GRID["origin"], FRAME_GRID["vs"], FRAME_GRID["dims"], FRAME_GRID["trunc"], FRAME_GRID["mw"])
    r, st_d = integrate_both(c, vol, D, K, c2w, 0.5, 8.0, tag=("frame", fid))
    assert st_f == st_d and bits_eq(t_f, vol["tsdf"]) and bits_eq(w_f, vol["weight"])
    return D, r["updated"]


@pytest.mark.parametrize("w,h", [(80, 48), (320, 240)])
def test_integrate_frame_equals_integrate_depth_of_the_models_plane(w, h):
    import plane_model as pm
    import test_dense_map_gpu as tdm
    sc = frame_scene(w, h)
    c = tdm.context(sc)
    make(c, FRAME_GRID)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_integrate_frame(tdm.FID, tdm.C2W, sc["K"], 0.5, 8.0)             # the archive has not seen the frame yet
    recs, runs, napp = c.dense_update_map(0, pm.make_draws(w), tdm.C2W)
    assert napp > 1000 and (runs["accept"] == 1).sum() == 3
    D1, n1 = frame_against_depth(c, tdm.FID, sc["K"], w, h, tdm.C2W, True)
    assert n1 > 300 and (D1 > 0).sum() > 900
    # a second nalo_dense_update_map of the same frame, its points moved back by 0.4: the LAST record at a pixel is the second call's
    sc2 = frame_scene(w, h, shift=0.4)
    P = len(sc2["u"])
    c.ba_set_points(np.zeros(P, np.int32), sc2["u"], sc2["v"], sc2["idp"], np.full((P, 8), 100, F), np.ones((P, 8), F))
    recs, runs, napp2 = c.dense_update_map(0, pm.make_draws(w), tdm.C2W)
    assert napp2 == napp and c.map_dense_counts(tdm.FID) == (2 * napp, 6)
    D2, n2 = frame_against_depth(c, tdm.FID, sc["K"], w, h, tdm.C2W, True)
    both = (D1 > 0) & (D2 > 0)
    assert both.sum() > 900 and (D2[both] > D1[both] + F(0.3)).all()          # with the first record at a pixel the plane would still be D1
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_integrate_frame(tdm.FID + 7, tdm.C2W, sc["K"], 0.5, 8.0)         # unknown frame_id
    before = state(c)
    for bad in (dict(c2w=np.full((3, 4), np.nan)), dict(K=(np.nan, 1.0, 1.0, 1.0)), dict(mn=3.0, mx=1.0)):
        a = dict(c2w=tdm.C2W, K=sc["K"], mn=0.5, mx=8.0)
        a.update(bad)
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_integrate_frame(tdm.FID, a["c2w"], a["K"], a["mn"], a["mx"])
    c.ba_set_allreduce(lambda ptr, n: None)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_integrate_frame(tdm.FID, tdm.C2W, sc["K"], 0.5, 8.0)             # a sharded window
    assert state(c) == before
    c.close()


def test_integrate_frame_of_a_frame_whose_every_cluster_was_rejected():
    import plane_model as pm
    import test_dense_map_gpu as tdm
    w, h = 320, 240
    sc = tdm.scene(w, h, (256.0, 256.0, 160.0, 120.0), [dict(value=23.0, sel=tdm.rect_sel(w, h, 75, 110, 5, 110), n=60, kind="wall", par=100.0)], seed=4, background=1.0)
    c = tdm.context(sc)
    make(c, FRAME_GRID)
    recs, runs, napp = c.dense_update_map(0, pm.make_draws(4), tdm.C2W)
    assert napp == 0 and ((runs["n"] > 0) & (runs["accept"] == 0)).sum() >= 1 and c.map_dense_counts(tdm.FID)[0] == 0      # known to the archive, without a point
    D, n = frame_against_depth(c, tdm.FID, sc["K"], w, h, tdm.C2W, False)
    assert n == 0 and not D.any() and c.tsdf_last()["updated"] == 0 and c.tsdf_last()["visited"] > 0
    c.close()


def test_two_frames_back_to_back_behind_queued_work():
    """two frames of the dense archive, each in more than 32 pieces (chunks of 32 points), integrated one directly after the other while the main stream still
    waits behind 0.2 s of a producer's matmuls: neither call may leave anything staged that the next one rewrites. Against the model on the three planes."""
    import plane_model as pm
    import test_dense_map_gpu as tdm
    w, h = 80, 48
    sa, sb = frame_scene(w, h), frame_scene(w, h, shift=0.4)
    c = tdm.context(sa, chunk=32)
    na, nb = len(sa["u"]), len(sb["u"])
    cat = lambda k: np.concatenate([sa[k], sb[k]])
    c.ba_set_points(np.concatenate([np.zeros(na, np.int32), np.ones(nb, np.int32)]), cat("u"), cat("v"), cat("idp"), np.full((na + nb, 8), 100, F), np.ones((na + nb, 8), F))
    for hf in (0, 1):
        assert c.dense_update_map(hf, pm.make_draws(w + hf), tdm.C2W)[2] > 1000
    with np.errstate(all="ignore"):
        Da, Db = (tm.frame_plane(c.map_dense_get(tdm.FID + k), w, h) for k in (0, 1))
    both = (Da > 0) & (Db > 0)
    assert both.sum() > 900 and (Db[both] > Da[both] + F(0.3)).all() and len(c.map_dense_get(tdm.FID)) > 32 * 32
    vol = make(c, FRAME_GRID)
    K = sa["K"]
    pa, pb = tdm.C2W, np.concatenate([tdm.C2W[:, :3], tdm.C2W[:, 3:] + np.array([[0.1], [-0.05], [0.1]])], 1)
    d0 = wavy_depth(w, h, 50, base=2.5)
    c.tsdf_integrate_frame(tdm.FID + 1, pb, K, 0.5, 8.0)                        # steady state: the scratch planes exist
    tm.integrate(vol, Db, K, pb, 0.5, 8.0)
    assert_volume(c, vol, "warm-up")
    t = torch.empty((h, w), device="cuda")
    d0_dev = torch.from_numpy(d0).cuda()
    a = torch.randn(4096, 4096, device="cuda")
    out = torch.empty_like(a)
    S = torch.cuda.Stream()
    try:
        with torch.cuda.stream(S):
            torch.mm(a, a, out=out)
            S.synchronize()
            t0 = time.perf_counter()
            torch.mm(a, a, out=out)
            S.synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
            for _ in range(min(int(math.ceil(0.25 / one)) + 1, 20000)):
                torch.mm(a, a, out=out)
            t.copy_(d0_dev)                                                      # device to device: a copy from pageable host memory would wait for S
            behind = torch.cuda.Event()
            behind.record(S)
            c.tsdf_integrate_depth(t, K, pa, 0.5, 8.0)                           # the main stream now waits for S
            c.tsdf_integrate_frame(tdm.FID, pa, K, 0.5, 8.0)
            c.tsdf_integrate_frame(tdm.FID + 1, pb, K, 0.5, 8.0)
            c.tsdf_integrate_frame(tdm.FID, pb, K, 0.5, 8.0)
            assert not behind.query(), "the calls waited for the producer stream"
        for D, p in ((d0, pa), (Da, pa), (Db, pb), (Da, pb)):
            r = tm.integrate(vol, D, K, p, 0.5, 8.0)
        assert c.tsdf_last()["updated"] == r["updated"] > 300
        assert_volume(c, vol, "two frames back to back")
    finally:
        S.synchronize()
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the device chain
def run_chain(with_volume):
    """tests/test_dense_map_gpu.py's chain (marginalize_frame -> carry_window -> linearize -> nalo_dense_update_map on frameHessians[size - 3] -> flag ->
    marginalize_flagged; the last keyframe's points stay standing) at 1224x368, W = 8, three keyframes; with_volume: a 256x64x256 volume integrated after every nalo_dense_update_map"""
    import lifecycle_model as lm
    import lifecycle_scenes as lsc
    import plane_cases as pc
    import plane_model as pm
    from nalo_slam_amd import synth
    WW, KF, w, h, s = 8, 3, 1224, 368, 3e-4
    win = synth.make_window(w=w, h=h, W=WW, P=8000, seed=lsc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    nF = WW + KF
    srng = np.random.RandomState(lsc.SEED + 3)
    st6 = np.zeros((nF, 6))
    st6[1:, :3] = 0.004 * srng.randn(nF - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * srng.randn(nF - 1, 3)
    mask = pc.block_mask(w, h, 2, 1, [2.0, 0.0])
    mask[2 * h // 3:, :w // 2] = 6.0
    mask[2 * h // 3:, w // 2:] = 8.0
    bgr = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    c = binding.Context(w, h, win.K, n_slots=nF)
    fids = [200 + i for i in range(WW)]
    for i in range(nF):
        c.frame_upload(i, win.images[i], mask=mask, bgr=bgr)
    c.ba_set_prior_carry(True)
    c.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=st6[:WW], frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(win.exists)
    ng0, lt0, ls0 = lm.default_history(win.exists)
    ls0[win.host == WW - 1, 0] = lm.IN
    c.ba_set_point_history(ng0, lt0, ls0)
    c.map_enable()
    c.map_dense_enable(True, 65536)
    cur, dense, known, stats = list(fids), {}, set(), []
    for kf in range(KF):
        if kf:
            c.ba_marginalize_frame(0)
            c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            cur = cur[1:] + [200 + WW - 1 + kf]
        c.ba_linearize(False)
        c.ba_linearize(True)
        hf, slot = WW - 3, WW - 3 + kf
        T = synth.se3_inv(win.world_to_cam[slot])
        recs, runs, napp = c.dense_update_map(hf, pm.make_draws(60 + kf), T)
        dense[cur[hf]] = c.map_dense_get(cur[hf])
        if with_volume:
            if kf == 0:
                # the volume is laid around the first keyframe's dense points (their 2nd .. 98th percentiles), the depth range around their depths
                xyz = c.map_dense_world_points(cur[hf], T)
                ok = np.isfinite(xyz).all(1)
                lo, hi = np.percentile(xyz[ok], 2, axis=0), np.percentile(xyz[ok], 98, axis=0)
                vs = float(max((hi - lo) / np.array([256, 64, 256])) * 1.05)
                origin = 0.5 * (lo + hi) - 0.5 * vs * np.array([256, 64, 256])
                dep = 1.0 / dense[cur[hf]]["idepth"].astype(np.float64)
                dep = dep[np.isfinite(dep) & (dep > 0)]
                rng_d = (float(np.percentile(dep, 2)) * 0.5, float(np.percentile(dep, 98)) * 2.0)
                c.tsdf_create(origin, vs, (256, 64, 256), 4 * vs, 16.0)
            c.tsdf_integrate_frame(cur[hf], T, win.K, rng_d[0], rng_d[1])
            stats.append(c.tsdf_last())
        ff = np.zeros(WW, np.uint8)
        ff[0] = 1
        c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
        known |= set(cur)
    assert sum(len(d) for d in dense.values()) > 1000
    out = [c.ba_get_points()[k].tobytes() for k in ("idepth", "step", "HdiF", "bdSumF", "Hdd", "bd", "Hcd", "maxRelBaseline")]
    out += [np.ascontiguousarray(a).tobytes() for a in c.ba_get_residuals()]
    for f in sorted(known):
        out += [c.map_get_frame(f).tobytes(), repr(c.map_counts(f)).encode()]
    out += [dense[f].tobytes() for f in sorted(dense)]
    fr = c.ba_get_frames()
    out += [bytes(fr[0]), fr[1].tobytes(), fr[2].tobytes()]                          # the window's frames and poses
    vol = [a.tobytes() for a in c.tsdf_get()] if with_volume else None
    c.close()
    return out, vol, stats


def test_three_keyframes_of_the_device_chain_at_1224x368():
    a, vol_a, stats = run_chain(True)
    b, vol_b, _ = run_chain(False)
    assert a == b                                                               # the twin never creates a volume: window, archives and poses are equal bit for bit
    print("TSDF chain 1224x368 into 256x64x256:", stats)
    assert all(st["visited"] >= st["updated"] > 0 for st in stats) and sum(st["updated"] for st in stats) > 1000       # not vacuous: every keyframe changed voxels
    a2, vol_a2, stats2 = run_chain(True)
    assert vol_a == vol_a2 and stats == stats2 and a2 == a                      # two runs give the same volume bytes
