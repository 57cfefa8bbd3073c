"""nalo_init_depth_image - CoarseInitializer::debugPlot on the device - against the host model of tests/init_plot_model.py.

The model is fed with what the read-back route returns: nalo_init_get_points (u, v, iR, isGood of the level) and nalo_frame_download (the first frame's irradiance
at the level). "Equal" is byte for byte for the image and bit for bit for sum_iR and fac (a NaN equals a NaN: include/nalo_gpu.h leaves its sign and payload open).

  1  640x480, every level: after nalo_init_set_first and after three nalo_init_track_frame; the coarser levels overlap (asserted on the host); two calls, same bytes;
     a fresh context through its coarsest level, level 0 and the coarsest again (the key plane grows, then is used far below its capacity)
  2  states planted through nalo_init_set_points: no good point, one good point, alternating, the special values of iR, the sum-order set
  3  a first frame whose irradiance leaves [0, 255]
  4  level 0 at 1224x368 after a tracked frame; all ~61 k points of 1920x1072 in one call
  5  a twin context that never plots stays bit-equal through two more tracked frames
  6  every refusal of the header, with sentinel-filled outputs and a legal call afterwards

The first frame's slot without a pyramid cannot be reached through the public calls (nalo_init_set_first refuses an empty slot and nothing empties one), so that
refusal is not provoked."""
import ctypes as C

import numpy as np
import pytest

import init_plot_model as ip
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

F = np.float32
ERR_ARG, ERR_HIP, ERR_STATE = -1, -3, -4


def make(w, h, frames, seed=3):
    win = synth.make_window(w=w, h=h, W=2, P=20, seed=seed, n_extra=frames - 2, step_z=0.15, yaw_deg=0.1)
    c = binding.Context(w, h, win.K, n_slots=frames + 1)
    for i in range(frames):
        c.frame_upload(i, win.images[i])
    c.pixsel_set_random(np.random.RandomState(seed).randint(0, 256, w * h).astype(np.uint8))
    num, _ = c.init_set_first(0)
    return c, num


_CTX = {}


def ctx(key, w, h, frames):
    if key not in _CTX:
        _CTX[key] = make(w, h, frames)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for c, _ in _CTX.values():
        c.close()
    _CTX.clear()


def expect(c, lvl, scale=1.0):
    p = c.init_points(lvl)
    I = c.frame_download(0, lvl)[0][:, 0]
    return ip.fast(I, c.w >> lvl, c.h >> lvl, p["u"], p["v"], p["iR"], p["isGood"], scale), p


def check(c, lvl, scale=1.0, what=""):
    want, p = expect(c, lvl, scale)
    got = c.init_depth_image(lvl, scale)
    tag = "%s level %d" % (what, lvl)
    assert got["bgr"].shape == want["bgr"].shape, tag
    assert got["n_points"] == want["n_points"] and got["n_good"] == want["n_good"], tag
    assert ip.same_float(got["sum_iR"], want["sum_iR"]), (tag, got["sum_iR"], want["sum_iR"])
    assert ip.same_float(got["fac"], want["fac"]), (tag, got["fac"], want["fac"])
    bad = np.argwhere(np.any(got["bgr"] != want["bgr"], axis=2))
    assert bad.size == 0, (tag, len(bad), bad[:4].tolist())
    return got, p


def close_pairs(p, w, h):
    """pairs of points whose centres lie at Chebyshev distance <= 2: their squares share a pixel"""
    occ = np.zeros((h + 4, w + 4), np.int64)
    cu, cv = (p["u"] + F(0.5)).astype(np.int64), (p["v"] + F(0.5)).astype(np.int64)
    np.add.at(occ, (cv + 2, cu + 2), 1)
    n = int(np.sum(occ * (occ - 1) // 2))
    for dy in range(0, 3):
        for dx in range(-2, 3):
            if dy == 0 and dx <= 0:
                continue
            a = occ[2:h + 2, 2:w + 2]
            b = occ[2 + dy:h + 2 + dy, 2 + dx:w + 2 + dx]
            n += int(np.sum(a * b))
    return n


def test_every_level_after_set_first_and_after_three_frames():
    c, num = ctx("main", 640, 480, 6)
    assert c.levels >= 4 and int(num[0]) > 3000
    for lvl in range(c.levels):
        got, p = check(c, lvl, what="after set_first")
        assert got["n_good"] == got["n_points"] == int(num[lvl]) and got["fac"] == 1       # iR = 1 everywhere: the sum is the count
        if lvl >= 1:
            assert close_pairs(p, c.w >> lvl, c.h >> lvl) >= 100, "level %d does not exercise overlap" % lvl
    for i in (1, 2, 3):
        c.init_track_frame(i)
    for lvl in range(c.levels):
        got, p = check(c, lvl, what="after three frames")
        assert len(np.unique(p["iR"])) > 10
        again = c.init_depth_image(lvl)
        assert again["bgr"].tobytes() == got["bgr"].tobytes() and ip.same_float(again["fac"], got["fac"]) and ip.same_float(again["sum_iR"], got["sum_iR"])
    check(c, 0, scale=0.37, what="rainbow_scale 0.37")
    check(c, 1, scale=4.0, what="rainbow_scale 4")


def test_plane_cleans_itself():
    """a context that has painted nothing yet paints its coarsest level, then level 0, then the coarsest again: the key plane grows, then is used far below its
    capacity; every call's bytes and results equal the model's"""
    c, _ = ctx("walk", 640, 480, 2)
    top = c.levels - 1
    assert top >= 3
    for lvl in (top, 0, top):
        check(c, lvl, what="the plane's walk")


def plant(c, lvl, iR=None, good=None):
    n = len(c.init_points(lvl)["u"])
    a = None if iR is None else np.ascontiguousarray(iR, F)
    g = None if good is None else np.ascontiguousarray(good, np.uint8)
    assert (a is None or len(a) == n) and (g is None or len(g) == n)
    c._ck(c.L.nalo_init_set_points(c.h_, lvl, n, None, None, binding._f(a), binding._u8(g), None, None, None, None, None, None, None))


def test_planted_states():
    c, num = ctx("plant", 640, 480, 2)
    rng = np.random.RandomState(11)
    for lvl in (0, 2):
        n = int(num[lvl])
        base = rng.uniform(0.2, 3.0, n).astype(F)
        # no good point: black squares only, fac = 0 / 0
        plant(c, lvl, base, np.zeros(n, np.uint8))
        got, _ = check(c, lvl, what="no good point")
        assert got["n_good"] == 0 and got["sum_iR"] == 0 and np.isnan(got["fac"])
        # exactly one good point
        g = np.zeros(n, np.uint8); g[n // 2] = 1
        plant(c, lvl, base, g)
        got, _ = check(c, lvl, what="one good point")
        assert got["n_good"] == 1 and got["sum_iR"] == base[n // 2]
        # alternating good / bad
        g = (np.arange(n) % 2).astype(np.uint8)
        plant(c, lvl, base, g)
        assert check(c, lvl, what="alternating")[0]["n_good"] == n // 2
        # the special values, each in turn alone among ordinary values and then all together
        special = np.array([0.0, -0.0, -1.5, np.nan, np.inf, 1e30, 1e-42, 1e-45], F)
        for k, s in enumerate(special):
            iR = base.copy(); iR[k::97] = s
            plant(c, lvl, iR, np.ones(n, np.uint8))
            check(c, lvl, what="iR = %r" % float(s))
        iR = base.copy(); iR[:8 * (n // 8)] = np.tile(special, n // 8)
        plant(c, lvl, iR, g)
        check(c, lvl, what="all special values")
        # sum_iR = 0 with good points: fac = inf
        plant(c, lvl, np.zeros(n, F), np.ones(n, np.uint8))
        assert np.isposinf(check(c, lvl, what="zero sum")[0]["fac"])
        # the sum-order set of the CPU test
        iR = ip.sum_order_set(n)
        plant(c, lvl, iR, np.ones(n, np.uint8))
        got, _ = check(c, lvl, what="sum order")
        assert got["sum_iR"] != F(np.sum(iR.astype(np.float64))) and got["sum_iR"] != np.sum(iR, dtype=F)


def test_irradiance_outside_the_byte_range():
    c, num = ctx("plant", 640, 480, 2)
    w, h = c.w, c.h
    img = np.array(c.frame_download(0, 0)[0][:, 0]).reshape(h, w)
    img[40:80, 40:120] = -20.5
    img[100:140, 40:120] = 300.0
    img[160:200, 40:120] = 255.5
    img[220:224, 40:44] = np.nan
    img[260:264, 40:44] = np.inf
    img[300:304, 40:44] = -np.inf
    img[340:344, 40:44] = 1e20
    c.frame_upload(0, img)                                                       # the initialiser's points stay; the slot now holds this irradiance
    plant(c, 0, np.random.RandomState(2).uniform(0.2, 3.0, int(num[0])).astype(F), np.ones(int(num[0]), np.uint8))
    for lvl in range(c.levels):
        check(c, lvl, what="wild irradiance")
    lv0 = np.array(c.frame_download(0, 0)[0][:, 0])                             # the cases are there as they were sent
    assert np.isnan(lv0).any() and np.isposinf(lv0).any() and (lv0 < 0).any() and (lv0 > 255).any()


def test_level0_at_1224x368_after_a_tracked_frame():
    c, num = ctx("kitti", 1224, 368, 2)
    c.init_track_frame(1)
    got, _ = check(c, 0, what="1224x368")
    assert got["n_points"] == int(num[0]) > 5000


def test_all_points_of_1920x1072_in_one_call():
    c, num = ctx("hd", 1920, 1072, 2)
    n = int(num[0])
    assert n > 50000
    plant(c, 0, np.random.RandomState(4).uniform(0.2, 3.0, n).astype(F), (np.arange(n) % 5 != 0).astype(np.uint8))
    got, _ = check(c, 0, what="1920x1072")
    assert got["n_points"] == n and got["n_good"] == n - (n + 4) // 5


def init_bits(c):
    s = c.init_state()
    out = [s["thisToNext"].tobytes(), s["aff"].tobytes(), repr((s["snapped"], s["frameID"], s["snappedAt"], s["n_evals"]))]
    for lvl in range(c.levels):
        for d in (c.init_points(lvl), c.init_carried(lvl)):
            out += [k + ":" + str(np.ascontiguousarray(v).tobytes()) for k, v in sorted(d.items())]
    return out


def test_a_twin_that_never_plots_stays_bit_equal():
    a, _ = make(640, 480, 6)
    b, _ = make(640, 480, 6)
    for i in (1, 2, 3):
        for c in (a, b):
            c.init_track_frame(i)
    assert init_bits(a) == init_bits(b)
    for i in (4, 5):
        for lvl in range(a.levels):
            a.init_depth_image(lvl)
        for c in (a, b):
            c.init_track_frame(i)
        a.init_depth_image(0)
        assert init_bits(a) == init_bits(b), "after frame %d" % i
    a.close()
    b.close()


def _raw(c, bgr, lvl=0, rs=1.0, null_args=False, null_ctx=False):
    a = binding.InitPlotArgs()
    a.lvl, a.rainbow_scale = lvl, rs
    a.bgr = None if bgr is None else bgr.ctypes.data_as(binding.c_u8p)
    a.w = a.h = a.n_points = a.n_good = -7
    a.sum_iR = a.fac = -7.0
    rc = c.L.nalo_init_depth_image(None if null_ctx else c.h_, None if null_args else C.byref(a))
    return rc, a


def test_refusals_leave_the_outputs_untouched():
    w, h = 640, 480
    bgr = np.full(3 * w * h, 0xA5, np.uint8)

    def untouched(a=None):
        return (bgr == 0xA5).all() and (a is None or (a.w, a.h, a.n_points, a.n_good, a.sum_iR, a.fac) == (-7, -7, -7, -7, -7.0, -7.0))
    # no initialiser
    c0 = binding.Context(w, h, (330.0, 330.0, 319.5, 239.5), n_slots=1)
    rc, a = _raw(c0, bgr)
    assert rc == ERR_STATE and untouched(a)
    c0.close()
    c, _ = make(w, h, 2)
    before = init_bits(c)
    assert _raw(c, bgr, null_ctx=True)[0] == ERR_ARG and _raw(c, bgr, null_args=True)[0] == ERR_ARG
    for kw in (dict(lvl=-1), dict(lvl=c.levels), dict(lvl=6), dict(rs=np.nan), dict(rs=np.inf), dict(rs=-np.inf)):
        rc, a = _raw(c, bgr, **kw)
        assert rc == ERR_ARG and untouched(a), kw
    rc, a = _raw(c, None)
    assert rc == ERR_ARG and untouched(a)
    assert init_bits(c) == before
    # the call works after the refusals and writes only the level's bytes
    rc, a = _raw(c, bgr, lvl=1)
    want, _ = expect(c, 1)
    npx = 3 * (w >> 1) * (h >> 1)
    assert rc == 0 and (a.w, a.h) == (w >> 1, h >> 1) and bgr[:npx].tobytes() == want["bgr"].tobytes() and (bgr[npx:] == 0xA5).all()
    bgr[:] = 0xA5
    # a context whose cross-rank exchange failed
    c.ba_exchange_failed("link down (init plot test)")
    rc, a = _raw(c, bgr)
    assert rc == ERR_HIP and untouched(a)
    c.close()
