"""nalo_trk_depth_image: CoarseTracker::debugPlotIDepthMap (CoarseTracker.cpp:1263-1359) on the device, and nalo_trk_set_depth that plants its input.

Every comparison is exact: np.array_equal on the image's bytes, bit equality on the floats. The expected result comes from tests/depth_image_model.py:
`literal` is the reference's loops one to one, `fast` its vectorised twin (tests/test_depth_image_cpu.py shows fast == literal on the planted maps used here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import depth_image_cases as cases
import depth_image_model as model
from conftest import ROOT
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

F = np.float32
ERR_ARG, ERR_HIP, ERR_STATE = -1, -3, -4
# the paint kernel's tile of outputs per workgroup, read from the kernel's source so the straddling test follows it
_src = open(os.path.join(ROOT, "nalo-slam_amd", "csrc", "kernels_depth_image.hip")).read()
TILE_W, TILE_H = [int(v) for v in re.search(r"kDiTW = (\d+), kDiTH = (\d+);", _src).groups()]


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def same(dev, want, what=""):
    assert want is not None
    assert dev["bgr"].shape == want["bgr"].shape
    bad = (dev["bgr"] != want["bgr"]).any(axis=2)
    assert not bad.any(), "%s: %d pixels differ, first at (x, y) = %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0][::-1]))
    assert dev["n_positive"] == want["n_positive"], what
    for k in ("min_new", "max_new", "min_used", "max_used"):
        assert bits(dev[k]) == bits(want[k]), (what, k, dev[k], want[k])
    assert (dev["minmax"] is None) == (want["minmax"] is None)
    if want["minmax"] is not None:
        assert np.array_equal(bits(dev["minmax"]), bits(want["minmax"])), (what, dev["minmax"], want["minmax"])


def planted_ctx(w, h):
    c = binding.Context(w, h, (0.5 * w, 0.5 * w, (w - 1) / 2.0, (h - 1) / 2.0), n_slots=1)
    I = cases.image(w, h)
    c.frame_upload(0, I)
    return c, I


def run(c, m, minmax, want_idepth=False):
    c.trk_set_depth(0, 0, m)
    return c.trk_depth_image(minmax, want_idepth)


def test_planted_sizes_end_in_partial_tiles():
    assert 80 % TILE_W and 40 % TILE_H


@pytest.mark.parametrize("w,h", [(64, 32), (80, 48), (72, 40)])
def test_planted_maps(w, h):
    """every planted map: first call (-1, -1), a second different map on the returned pair, and NULL pointers. 64 x 32 is whole tiles of the paint kernel, 80 x 48
    ends in a partial tile in x, 72 x 40 in both directions"""
    c, I = planted_ctx(w, h)
    maps = cases.planted(w, h)
    full = dict(maps)["full_distinct"]
    for name, m in maps:
        want = model.fast(m, I, w, h, (-1.0, -1.0))
        got = run(c, m, (-1.0, -1.0), want_idepth=True)
        same(got, want, name)
        assert np.array_equal(bits(got["idepth"]), bits(m).reshape(-1)), name
        assert np.array_equal(bits(got["minmax"]), bits([want["min_new"], want["max_new"]]))
        m2 = (full * F(8)).astype(F) if name != "full_distinct" else (m * F(0.05)).astype(F)
        same(run(c, m2, got["minmax"]), model.fast(m2, I, w, h, want["minmax"]), name + " / second map")
        same(run(c, m, None), model.fast(m, I, w, h, None), name + " / NULL")
    c.close()


def test_all_four_clamps_and_negative_span():
    """pairs chosen so that each of the four ifs of :1299-1308 fires, checked against the formula itself, then against the model"""
    w, h = 64, 32
    c, I = planted_ctx(w, h)
    m = dict(cases.planted(w, h))["full_distinct"]
    free = model.fast(m, I, w, h, None)
    mn_new, mx_new = free["min_new"], free["max_new"]
    fired = set()
    for pair in [(F(10.0), F(11.0)), (F(1e-4), F(2e-4)), (F(2.0), F(1.0)), (F(0.0), F(0.0)), (mn_new, mx_new), (F(np.inf), F(np.inf)), (F(np.nan), F(1.0))]:
        got = run(c, m, pair)
        same(got, model.fast(m, I, w, h, pair), str(pair))
        with np.errstate(all="ignore"):
            mc = F(0.3 * float(F(pair[1] - pair[0])))
            if mn_new < F(pair[0] - mc):
                fired.add(1)
            if max(mn_new, F(pair[0] - mc)) > F(pair[0] + mc):
                fired.add(2)
            if mx_new < F(pair[1] - mc):
                fired.add(3)
            if max(mx_new, F(pair[1] - mc)) > F(pair[1] + mc):
                fired.add(4)
    assert fired == {1, 2, 3, 4}
    c.close()


def test_sources_straddling_tile_borders():
    """plotting sources 3, 2, 1 pixels before and 0, 1, 2 pixels after every tile edge of di_paint_kernel (TILE_W x TILE_H outputs per workgroup, read from its
    source above), in x and in y: a ring then crosses the edge by 2 and 3 pixels either way and the output's winner lies in the neighbour's halo. Against `literal`."""
    w, h = 2 * TILE_W + 16, 3 * TILE_H
    c, I = planted_ctx(w, h)
    for o in (-3, -2, -1, 0, 1, 2):
        m = np.zeros((h, w), F)
        k = 0
        for ex in range(TILE_W, w - 3, TILE_W):
            for y in range(3, h - 3, 5):
                k += 1
                m[y, ex + o] = 0.05 * k
        for ey in range(TILE_H, h - 3, TILE_H):
            for x in range(3, w - 3, 5):
                k += 1
                m[ey + o, x] = 0.05 * k
        same(run(c, m, (-1.0, -1.0)), model.literal(m, I, w, h, (-1.0, -1.0)), "offset %d" % o)
    c.close()


def _keyframes(w, h, n_pts):
    """two rendered frames and three sets of setCoarseTrackingRef inputs (keyframe i uses frame i % 2, its depths scaled so the quantiles move between keyframes)"""
    win = synth.make_window(w=w, h=h, W=2, P=8, seed=3, n_extra=0)
    rng = np.random.RandomState(1)
    refs = []
    for i in range(3):
        Ku = rng.uniform(5, w - 6, n_pts).astype(F)
        Kv = rng.uniform(5, h - 6, n_pts).astype(F)
        d = win.depth[i % 2][(Kv + 0.5).astype(int), (Ku + 0.5).astype(int)]
        ok = np.isfinite(d)
        refs.append((Ku[ok], Kv[ok], (1.0 / d[ok]).astype(F) * F(1.0 + 0.3 * i), np.full(int(ok.sum()), 1e-4, F)))
    return win, refs


@pytest.mark.parametrize("w,h,n_pts", [(1224, 368, 3000), (1920, 1072, 12000)])
def test_real_shapes_three_keyframes(w, h, n_pts):
    """nalo_trk_set_ref on synthetic keyframes, three in a row with the pair carried as FullSystem carries minIdJetVisTracker / maxIdJetVisTracker; the model is fed
    from nalo_trk_get_depth(0) and nalo_frame_download(slot, 0)"""
    win, refs = _keyframes(w, h, n_pts)
    c = binding.Context(w, h, win.K, n_slots=3)
    pair_dev, pair_model = (-1.0, -1.0), (-1.0, -1.0)
    for i in range(3):
        c.frame_upload(i, win.images[i % 2])
        c.trk_set_ref(i, *refs[i])
        got = c.trk_depth_image(pair_dev, want_idepth=True)
        idepth0 = c.trk_get_depth(0)[0]
        I0 = c.frame_download(i, 0)[0][:, 0]
        want = model.fast(idepth0, I0, w, h, pair_model)
        same(got, want, "keyframe %d" % i)
        assert np.array_equal(bits(got["idepth"]), bits(idepth0))
        assert got["n_positive"] == int((idepth0 > 0).sum()) > 1000
        pair_dev, pair_model = got["minmax"], want["minmax"]
    c.close()


def test_no_side_effects_and_repeatable():
    win, refs = _keyframes(320, 240, 1500)
    c = binding.Context(320, 240, win.K, n_slots=2)
    c.frame_upload(0, win.images[0])
    c.frame_upload(1, win.images[1])
    c.trk_set_ref(0, *refs[0])
    T0 = synth.se3_mul(win.world_to_cam[1], synth.se3_inv(win.world_to_cam[0]))

    def state():
        out = []
        for l in range(c.levels):
            out += list(c.trk_get_pc(l)) + list(c.trk_get_depth(l))
        trk = c.trk_track(1, T0, [0, 0], [0, 0], [1, 1], c.levels - 1)
        return out + [np.asarray(trk[0], np.float64), np.asarray(trk[1], np.float64), np.asarray(trk[2], np.float64)]
    before = state()
    a = c.trk_depth_image((0.01, 0.2))
    b = c.trk_depth_image((0.01, 0.2))
    assert np.array_equal(a["bgr"], b["bgr"]) and np.array_equal(bits(a["minmax"]), bits(b["minmax"]))
    after = state()
    assert len(before) == len(after)
    for x, y in zip(before, after):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    # a sharded tracker holds the whole reference on every rank: the same bytes
    c.trk_set_shard(0, 2, lambda ptr, n: None)
    s = c.trk_depth_image((0.01, 0.2))
    assert np.array_equal(a["bgr"], s["bgr"]) and np.array_equal(bits(a["minmax"]), bits(s["minmax"]))
    c.close()


def test_set_depth():
    w, h = 320, 240                                                # three pyramid levels
    win, refs = _keyframes(w, h, 1500)
    c = binding.Context(w, h, win.K, n_slots=1)
    assert c.levels == 3
    c.frame_upload(0, win.images[0])
    c.trk_set_ref(0, *refs[0])
    clouds = [c.trk_get_pc(l) for l in range(c.levels)]
    maps = [c.trk_get_depth(l) for l in range(c.levels)]
    rng = np.random.RandomState(2)
    lvl = 1
    n = (w >> lvl) * (h >> lvl)
    a, b = rng.randn(n).astype(F), rng.rand(n).astype(F)
    a[3], b[5] = np.nan, np.inf
    c.trk_set_depth(0, lvl, a, b)
    ga, gb = c.trk_get_depth(lvl)
    assert np.array_equal(bits(ga), bits(a)) and np.array_equal(bits(gb), bits(b))
    a2 = rng.randn(n).astype(F)
    c.trk_set_depth(0, lvl, a2, None)                              # NULL weight sums: untouched
    ga, gb = c.trk_get_depth(lvl)
    assert np.array_equal(bits(ga), bits(a2)) and np.array_equal(bits(gb), bits(b))
    b2 = rng.rand(n).astype(F)
    c.trk_set_depth(0, lvl, None, b2)                              # NULL inverse depths: untouched
    ga, gb = c.trk_get_depth(lvl)
    assert np.array_equal(bits(ga), bits(a2)) and np.array_equal(bits(gb), bits(b2))
    c.trk_set_depth(0, lvl, None, None)
    ga, gb = c.trk_get_depth(lvl)
    assert np.array_equal(bits(ga), bits(a2)) and np.array_equal(bits(gb), bits(b2))
    for l in range(c.levels):                                      # other levels and every cloud unchanged
        for x, y in zip(clouds[l], c.trk_get_pc(l)):
            assert x.tobytes() == y.tobytes()
        if l != lvl:
            for x, y in zip(maps[l], c.trk_get_depth(l)):
                assert x.tobytes() == y.tobytes()
    c.close()


def test_set_depth_on_a_fresh_context_then_depth_image():
    w, h = 64, 32
    c, I = planted_ctx(w, h)
    c2 = binding.Context(w, h, c.K, n_slots=2)                     # no reference was ever set here; the frame sits in slot 1
    c2.frame_upload(1, I)
    m = dict(cases.planted(w, h))["checkerboard"]
    c2.trk_set_depth(1, 0, m)
    ga, gb = c2.trk_get_depth(0)
    assert np.array_equal(bits(ga), bits(m).reshape(-1)) and not gb.any()      # the half that was not given reads as zeros
    same(c2.trk_depth_image((-1.0, -1.0)), model.fast(m, I, w, h, (-1.0, -1.0)))
    c.close()
    c2.close()


def _raw(c, bgr, mm, null_args=False, null_ctx=False):
    a = binding.DepthImageArgs()
    a.minmax_io = None if mm is None else mm.ctypes.data_as(binding.c_fp)
    a.bgr = None if bgr is None else bgr.ctypes.data_as(binding.c_u8p)
    a.idepth = None
    rc = c.L.nalo_trk_depth_image(None if null_ctx else c.h_, None if null_args else C.byref(a))
    return rc, a


def test_refusals_leave_the_outputs_untouched():
    w, h = 64, 32
    c, I = planted_ctx(w, h)
    bgr = np.full((h, w, 3), 0xA5, np.uint8)
    mm = np.array([0.25, 0.75], F)

    def untouched():
        return (bgr == 0xA5).all() and mm.tolist() == [0.25, 0.75]
    # no tracking reference yet: slot_ref < 0
    assert _raw(c, bgr, mm)[0] == ERR_STATE and untouched()
    # bad arguments
    assert _raw(c, bgr, mm, null_ctx=True)[0] == ERR_ARG and _raw(c, bgr, mm, null_args=True)[0] == ERR_ARG and _raw(c, None, mm)[0] == ERR_ARG and untouched()
    # a reference slot that holds no frame
    c2 = binding.Context(w, h, c.K, n_slots=2)
    c2.trk_set_depth(1, 0, np.ones((h, w), F))
    assert _raw(c2, bgr, mm)[0] == ERR_STATE and untouched()
    c2.close()
    # slot_ref set and its frame uploaded, but no level-0 map (160 x 120 has two pyramid levels; only level 1 was planted)
    c3 = binding.Context(160, 120, (80.0, 80.0, 79.5, 59.5), n_slots=1)
    assert c3.levels == 2
    c3.frame_upload(0, cases.image(160, 120))
    c3.trk_set_depth(0, 1, None, None)
    big = np.full((120, 160, 3), 0xA5, np.uint8)
    assert _raw(c3, big, mm)[0] == ERR_STATE and (big == 0xA5).all() and untouched()
    c3.close()
    # no positive value: nothing painted, the pair left as it was
    m = np.zeros((h, w), F)
    m[5, 5], m[6, 6], m[7, 7] = -1.0, np.nan, -0.0
    c.trk_set_depth(0, 0, m)
    rc, a = _raw(c, bgr, mm)
    assert rc == ERR_STATE and a.n_positive == 0 and untouched()
    assert b"no positive" in c.L.nalo_last_error(c.h_)
    # the call works again once the map holds a positive value
    m[9, 9] = 0.5
    same(run(c, m, (-1.0, -1.0)), model.fast(m, I, w, h, (-1.0, -1.0)))
    # a context whose cross-rank exchange failed
    c.ba_exchange_failed("link down (depth image test)")
    assert _raw(c, bgr, mm)[0] == ERR_HIP and untouched()
    c.close()
