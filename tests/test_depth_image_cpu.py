"""The host models of nalo_trk_depth_image (tests/depth_image_model.py), no GPU: the vectorised model equals the literal transliteration of
CoarseTracker::debugPlotIDepthMap byte for byte on the planted maps, and hand-worked cases pin the literal one down."""
import numpy as np
import pytest

import depth_image_cases as cases
import depth_image_model as model

F = np.float32
W, H = 64, 32


def same(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    assert np.array_equal(a["bgr"], b["bgr"]), "%d bytes differ" % int((a["bgr"] != b["bgr"]).sum())
    for k in ("n_positive", "min_new", "max_new", "min_used", "max_used"):
        assert np.array(a[k]).tobytes() == np.array(b[k]).tobytes(), k
    assert (a["minmax"] is None) == (b["minmax"] is None)
    if a["minmax"] is not None:
        assert a["minmax"].tobytes() == b["minmax"].tobytes()


PLANTED = cases.planted(W, H)


@pytest.mark.parametrize("name", [n for n, _ in PLANTED])
def test_fast_equals_literal(name):
    m = dict(PLANTED)[name]
    I = cases.image(W, H)
    a = model.literal(m, I, W, H, (-1.0, -1.0))
    same(model.fast(m, I, W, H, (-1.0, -1.0)), a)
    # a second, different map on the returned pair (the smoothing's clamps), and the NULL pointers
    m2 = (dict(PLANTED)["full_distinct"] * F(8)).astype(F) if name != "full_distinct" else (m * F(0.05)).astype(F)
    same(model.fast(m2, I, W, H, a["minmax"]), model.literal(m2, I, W, H, a["minmax"]))
    same(model.fast(m, I, W, H, None), model.literal(m, I, W, H, None))


def test_no_positive_value():
    m = np.zeros((H, W), F)
    m[4, 4], m[5, 5] = -1.0, np.nan
    assert model.literal(m, cases.image(W, H), W, H) is None and model.fast(m, cases.image(W, H), W, H) is None


def test_isolated_pixel_ring_of_40():
    m = np.zeros((H, W), F)
    m[12, 20] = 0.7
    I = np.full((H, W), 100.0, F)                                    # grey 90
    out = model.literal(m, I, W, H)
    assert out["n_positive"] == 1 and out["min_new"] == F(0.7) and out["max_new"] == F(0.7)
    col = out["bgr"]
    ring = (col != 90).any(axis=2)
    ys, xs = np.nonzero(ring)
    assert len(ys) == 40
    assert all(2 <= max(abs(x - 20), abs(y - 12)) <= 3 for x, y in zip(xs, ys))
    assert (col[ring] == (255, 255, 255)).all()                     # maxID == minID and sid / nid == minID: 0 / 0, the defined white
    assert (col[11:14, 19:22] == 90).all()                          # the source and its eight neighbours stay grey


def test_two_sources_two_apart():
    m = np.zeros((H, W), F)
    m[12, 20], m[12, 22] = 0.2, 0.8                                  # ranks for n = 1: both (int)0 -> min = max = 0.2
    I = np.full((H, W), 100.0, F)
    out = model.literal(m, I, W, H, None)
    assert out["min_used"] == F(0.2) and out["max_used"] == F(0.2)
    first, second = model.jet(np.nan), model.jet(np.inf)             # (0.2 - 0.2) / 0 = NaN -> white; (0.8 - 0.2) / 0 = +inf -> (0, 0, 128)
    assert first == (255, 255, 255) and second == (0, 0, 128)
    col = out["bgr"]
    assert tuple(col[12, 22]) == first                               # the earlier source's ring colours the later source's own pixel ...
    assert tuple(col[12, 20]) == second                              # ... and the later one's ring the earlier source's
    assert tuple(col[12, 24]) == second and tuple(col[12, 25]) == second
    assert tuple(col[12, 23]) == first                               # 3 right of the first, 1 right of the second (which does not write it)
    assert tuple(col[12, 18]) == first and tuple(col[12, 17]) == first and tuple(col[12, 19]) == second
    assert tuple(col[9, 22]) == second and tuple(col[9, 19]) == second and tuple(col[9, 18]) == first   # shared rows: the later one overwrites where both reach
    same(model.fast(m, I, W, H, None), out)


def below(x):
    return np.nextafter(F(x), F(-1))


def test_jet_branches():
    assert model.jet(-1.0) == (128, 0, 0) and model.jet(0.0) == (128, 0, 0) and model.jet(-0.0) == (128, 0, 0)
    assert model.jet(1.0) == (0, 0, 128) and model.jet(2.0) == (0, 0, 128)
    assert model.jet(np.nan) == (255, 255, 255)
    assert model.jet(np.inf) == (0, 0, 128) and model.jet(-np.inf) == (128, 0, 0)
    # at k / 8 the fraction is 0; just below it the fraction is 1 - 2^-21 or closer to 1 (8 * id is exact)
    want_at = {1: (255, 0, 0), 2: (255, 127, 0), 3: (255, 255, 0), 4: (127, 255, 127), 5: (0, 255, 255), 6: (0, 127, 255), 7: (0, 0, 255)}
    want_below = {1: (254, 0, 0), 2: (255, 127, 0), 3: (255, 254, 0), 4: (127, 255, 127), 5: (0, 255, 254), 6: (0, 127, 255), 7: (0, 0, 255), 8: (0, 0, 127)}
    for k, c in want_at.items():
        assert model.jet(F(k / 8.0)) == c, k
    for k, c in want_below.items():
        assert model.jet(below(k / 8.0)) == c, k
    assert model.jet(np.nextafter(F(0), F(1))) == (127, 0, 0)        # the smallest positive id: 255 * 0.5 = 127.5
    ids = np.array([-1, 0, 1, 2, np.nan, np.inf, -np.inf] + [k / 8.0 for k in range(1, 8)] + [below(k / 8.0) for k in range(1, 9)], F)
    assert [tuple(r) for r in model._jet_vec(ids)] == [model.jet(i) for i in ids]


def test_ranks():
    # size = n + 1; (int)(n * 0.05), (int)(n * 0.95) with the product in double
    assert [model.ranks(n + 1) for n in (0, 1, 19, 20, 21, 100)] == [(0, 0), (0, 0), (0, 18), (1, 19), (1, 19), (5, 95)]


def test_grey_byte():
    assert [model.grey_byte(v) for v in cases.SPECIAL_I] == [0, 254, 255, 255, 255, 0, 254, 0, 255]
    assert model.grey_byte(-np.inf) == 0 and model.grey_byte(-1.2) == 255 and model.grey_byte(-3e9) == 0


def test_smoothing():
    # first call: the pair takes the new values
    mn, mx, pair = model.smooth(0.2, 0.9, (-1.0, -1.0))
    assert (mn, mx) == (F(0.2), F(0.9)) and pair.tolist() == [F(0.2), F(0.9)]
    assert model.smooth(0.2, 0.9, None) == (F(0.2), F(0.9), None)
    old = (F(1.0), F(2.0))
    mc = F(0.3 * float(F(2.0) - F(1.0)))
    # clamped up: the new values lie far below, each may fall by maxChange only
    mn, mx, pair = model.smooth(0.1, 0.2, old)
    assert (mn, mx) == (F(F(1.0) - mc), F(F(2.0) - mc)) and pair.tolist() == [mn, mx]
    # clamped down: far above
    mn, mx, pair = model.smooth(5.0, 9.0, old)
    assert (mn, mx) == (F(F(1.0) + mc), F(F(2.0) + mc)) and pair.tolist() == [mn, mx]
    # inside the band: unchanged
    mn, mx, _ = model.smooth(1.1, 2.1, old)
    assert (mn, mx) == (F(1.1), F(2.1))
    # negative span: maxChange < 0, so `minID < min - maxChange` moves minID UP to min - maxChange and the second if then pulls it to min + maxChange
    neg = (F(2.0), F(1.0))
    mcn = F(0.3 * float(F(1.0) - F(2.0)))
    mn, mx, _ = model.smooth(1.5, 1.6, neg)
    assert mcn < 0 and mn == F(F(2.0) + mcn) and mx == F(F(1.0) + mcn)
