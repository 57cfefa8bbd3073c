"""tests/window_plot_model.py, the host model of FullSystem::debugPlot that tests/test_window_plot_gpu.py holds nalo_map_window_plot against: the vectorised form
against the literal one, and hand-worked cases of every rule the literal form states."""
import numpy as np
import pytest

import window_plot_model as model

F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def pts(u, v, idepth):
    return dict(u=np.asarray(u, F), v=np.asarray(v, F), idepth=np.asarray(idepth, F))


def imm(u, v, idmin, idmax, status, quality):
    return dict(u=np.asarray(u, F), v=np.asarray(v, F), idmin=np.asarray(idmin, F), idmax=np.asarray(idmax, F), status=np.asarray(status, np.int32),
                quality=np.asarray(quality, F))


def flat(w, h, value=100.0):
    return np.full(w * h, value, F)


def random_window(w, h, n_frames, n, seed):
    """frames with every class, centres up to 5 pixels outside the image, special inverse depths and irradiances"""
    rng = np.random.RandomState(seed)
    special = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, 1e-42, 2147483648.0, 3e9, 0.99999994, 1.0000001, 2.0, 2.9999998], F)

    def some(k):
        d = rng.uniform(0.01, 6.0, k).astype(F)
        m = rng.rand(k) < 0.3
        d[m] = special[rng.randint(0, len(special), int(m.sum()))]
        return pts(rng.uniform(-5, w + 5, k), rng.uniform(-5, h + 5, k), d)
    frames = []
    for _ in range(n_frames):
        I = rng.uniform(-20, 330, w * h).astype(F)
        I[rng.rand(w * h) < 0.02] = np.nan
        q = rng.uniform(0.2, 6.0, n).astype(F)
        m = rng.rand(n) < 0.2
        q[m] = special[rng.randint(0, len(special), int(m.sum()))]
        idmax = rng.uniform(0.5, 3.0, n).astype(F)
        idmax[rng.rand(n) < 0.2] = np.nan
        frames.append(dict(I=I, active=some(n), marg=some(n // 2), out=some(n // 3),
                           imm=imm(rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n), rng.uniform(-0.5, 1.0, n), idmax, rng.randint(0, 7, n), q)))
    return frames


def same(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    assert np.array_equal(a["bgr"], b["bgr"]) and np.array_equal(a["sources"], b["sources"]) and a["frames"] == b["frames"] and a["n_values"] == b["n_values"]
    for k in ("min_new", "max_new", "min_used", "max_used"):
        assert np.asarray(a[k], F).view(np.uint32) == np.asarray(b[k], F).view(np.uint32), k
    assert (a["minmax"] is None) == (b["minmax"] is None)
    if a["minmax"] is not None:
        assert np.array_equal(np.asarray(a["minmax"], F).view(np.uint32), np.asarray(b["minmax"], F).view(np.uint32))


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5, 7, 8, 9])
def test_fast_equals_literal(mode):
    w, h = 40, 24
    frames = random_window(w, h, 3, 30, seed=mode)
    for mask, mm, rs, qs in ((0, (-1.0, -1.0), 1.0, 1.0), (0b101, (0.5, 1.5), 0.37, 2.5), (0b010, None, 1e9, -1.0)):
        same(model.fast(frames, w, h, mode, mask, mm, rs, qs), model.literal(frames, w, h, mode, mask, mm, rs, qs))


def test_the_ring_is_40_pixels():
    w, h = 16, 16
    f = dict(I=flat(w, h, 0.0), active=pts([8], [8], [0.5]))
    img = model.literal([f], w, h, 1)["bgr"][0]
    hit = img.any(axis=2)
    want = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            want[y, x] = 2 <= max(abs(x - 8), abs(y - 8)) <= 3
    assert hit.sum() == 40 and np.array_equal(hit, want)
    assert not hit[8, 8] and not hit[7:10, 7:10].any()
    # u + 0.5f truncated: 7.5 is pixel 8, 7.4999 pixel 7
    a = model.literal([dict(I=flat(w, h, 0.0), active=pts([7.5], [8.49], [0.5]))], w, h, 1)["bgr"][0].any(axis=2)
    assert np.array_equal(a, want)
    b = model.literal([dict(I=flat(w, h, 0.0), active=pts([7.4999], [8.5], [0.5]))], w, h, 1)["bgr"][0].any(axis=2)
    assert np.array_equal(b[1:, :-1], want[:-1, 1:])


@pytest.mark.parametrize("cu,cv,n", [(0, 8, 22), (8, 0, 22), (15, 8, 22), (8, 15, 22), (0, 0, 12), (-3, 8, 7), (8, 18, 7), (-4, 8, 0), (8, 19, 0), (-3, -3, 1), (1, 8, 26), (2, 8, 33), (3, 8, 40)])
def test_rings_clip_at_every_border(cu, cv, n):
    """a ring centred on pixel (cu, cv) of a 16 x 16 image. (int)(u + 0.5f) truncates toward zero, so a negative centre c comes from u = c - 1"""
    w, h = 16, 16
    u, v = (cu if cu >= 0 else cu - 1), (cv if cv >= 0 else cv - 1)
    assert (model.centre(u), model.centre(v)) == (cu, cv)
    img = model.literal([dict(I=flat(w, h, 0.0), active=pts([u], [v], [0.5]))], w, h, 1)
    assert img["bgr"][0].any(axis=2).sum() == n and img["sources"].tolist() == [[0, 1, 0, 0]]


def test_centre_conversion():
    assert [model.centre(x) for x in (-1.4, -0.6, 0.0, 0.49, 0.5, 7.4999, 7.5)] == [0, 0, 0, 0, 1, 7, 8]      # truncation toward zero: (-1.5, 0.5) is pixel 0
    assert [model.centre(x) for x in (NAN, INF, -INF, 3e9, -3e9)] == [0, 2147483647, -2147483648, 2147483647, -2147483648]


def test_rainbow_branches_and_special_ids():
    assert model.rainbow(0.25) == (191, 63, 0)                       # icP 0: 255 * 0.75 = 191.25, 255 * 0.25 = 63.75
    assert model.rainbow(1.5) == (0, 127, 127)                       # icP 1
    assert model.rainbow(2.75) == (191, 0, 63)                       # icP 2
    assert model.rainbow(3.0) == (255, 0, 0) and model.rainbow(4.0) == (0, 255, 0) and model.rainbow(5.0) == (0, 0, 255)
    assert model.rainbow(0.5, 3.0) == (0, 127, 127)                  # freeDebugParam3 multiplies first
    for x in (0.0, -0.0, -2.0, NAN, -INF):
        assert model.rainbow(x) == model.WHITE                       # !(id > 0)
    for x in (F(2147483648.0), F(3e9), INF):
        assert model.rainbow(x) == model.WHITE                       # INT_MIN % 3 matches no branch
    assert model.rainbow(F(2147483520.0)) == (255, 0, 0)             # the largest float below 2^31: (2^31 - 128) % 3 = 0, ifP = 0
    assert model.rainbow(F(1e-42)) == (255, 0, 0)                    # a denormal: icP 0, 255 * ifP truncates to 0
    assert model.rainbow(1.0, -1.0) == model.WHITE


def test_overlap_order_between_and_inside_lists():
    w, h = 24, 16
    I = flat(w, h, 0.0)
    a, b = model.rainbow(0.25), model.rainbow(1.5)
    # two active rings of different colours, the second two pixels to the right: rows 5, 6, 10, 11 overlap in x = 7..11 and take the second's colour
    img = model.literal([dict(I=I, active=pts([8, 10], [8, 8], [0.25, 1.5]))], w, h, 1)["bgr"][0]
    assert tuple(img[8, 11]) == a and tuple(img[8, 12]) == b and tuple(img[5, 6]) == a and tuple(img[5, 12]) == b
    assert all(tuple(img[y, x]) == b for y in (5, 6, 10, 11) for x in range(7, 12))
    img = model.literal([dict(I=I, active=pts([10, 8], [8, 8], [1.5, 0.25]))], w, h, 1)["bgr"][0]
    assert tuple(img[5, 6]) == a and tuple(img[5, 12]) == b and all(tuple(img[y, x]) == a for y in (5, 6, 10, 11) for x in range(7, 12))
    # active under marginalised under out, whatever the indices
    f = dict(I=I, active=pts([8], [8], [0.25]), marg=pts([8], [8], [0.25]), out=pts([8], [8], [0.25]))
    assert tuple(model.literal([f], w, h, 1)["bgr"][0][8, 11]) == model.WHITE
    f = dict(I=I, active=pts([8], [8], [0.25]), marg=pts([8], [8], [1.5]))
    assert tuple(model.literal([f], w, h, 1)["bgr"][0][8, 11]) == model.BLACK and tuple(model.literal([f], w, h, 0)["bgr"][0][8, 11]) == b
    f = dict(I=I, active=pts([8], [8], [0.25]), out=pts([9], [8], [0.25]))
    img = model.literal([f], w, h, 0)["bgr"][0]
    assert tuple(img[8, 11]) == model.WHITE and tuple(img[8, 5]) == a and tuple(img[8, 10]) == a     # (10, 8) is inside the out ring's hole
    same(model.fast([f], w, h, 0), model.literal([f], w, h, 0))


def test_mode_table():
    w, h = 36, 16
    I = flat(w, h, 100.0)
    f = dict(I=I, active=pts([5], [8], [0.25]), marg=pts([13], [8], [1.5]), out=pts([21], [8], [0.25]),
             imm=imm([5, 9, 13, 17, 21, 25, 29], [8] * 7, [0.2] * 7, [0.3, 0.3, 0.3, NAN, 0.3, 0.3, 0.3], [0, 1, 2, 3, 4, 5, 6], [4.0] * 7))
    grey = (90, 90, 90)

    def px(mode, x, **kw):
        return tuple(model.literal([f], w, h, mode, **kw)["bgr"][0][8, x + 3])
    assert [px(0, x) for x in (5, 13, 21)] == [model.rainbow(0.25), model.rainbow(1.5), model.WHITE]
    assert [px(1, x) for x in (5, 13, 21)] == [model.rainbow(0.25), model.BLACK, model.WHITE]
    for mode in (2, 8, 9):
        r = model.literal([f], w, h, mode)
        assert (r["bgr"] == 90).all() and not r["sources"].any()
    # 3: GOOD, SKIPPED, BADCONDITION only; SKIPPED has a NaN idepth_max: black
    assert [px(3, x) for x in (5, 9, 13, 17, 21, 25, 29)] == [model.rainbow(0.25), grey, grey, model.BLACK, model.rainbow(0.25), grey, grey]
    assert [px(4, x) for x in (5, 9, 13, 17, 21, 25, 29)] == [(0, 255, 0), (255, 0, 0), (0, 0, 255), (255, 255, 0), model.WHITE, model.BLACK, grey]
    # 5: d = quality_scale * (sqrt(4) - 1) = quality_scale
    assert [px(5, x, quality_scale=0.5) for x in (5, 25, 29)] == [(0, 127, 127), grey, (0, 127, 127)]
    assert px(5, 5, quality_scale=2.0) == (0, 255, 0) and px(5, 5, quality_scale=-1.0) == (0, 0, 255)
    assert model.mode5_colour(NAN, 1.0) == (0, 0, 0) and model.mode5_colour(-1.0, 1.0) == (0, 0, 0) and model.mode5_colour(INF, 1.0) == (0, 255, 0)
    # 7: active jet, marginalised black, out not drawn but counted
    r = model.literal([f], w, h, 7)
    assert r["n_values"] == 3 and r["sources"].tolist() == [[0, 1, 1, 0]]
    assert tuple(r["bgr"][0][8, 15]) == model.BLACK and tuple(r["bgr"][0][8, 23]) == grey
    assert model.literal([f], w, h, 4)["sources"].tolist() == [[6, 0, 0, 0]]
    # the mask selects frames in window order; mode 7's range ignores it
    g = dict(I=flat(w, h, 50.0), active=pts([5], [8], [9.0]))
    r = model.literal([f, g], w, h, 7, frame_mask=0b10)
    assert r["frames"] == [1] and r["bgr"].shape[0] == 1 and r["n_values"] == 4 and (r["bgr"][0][0, 0] == 45).all()


def test_ranks_with_negatives_and_signed_zero():
    def sel(v):
        return model.select(np.asarray(v, F), None)
    r = sel([3.0])
    assert (r["min_new"], r["max_new"], r["n_values"]) == (3.0, 3.0, 1)
    r = sel([2.0, -1.0])                                            # n = 1: both ranks 0
    assert (r["min_new"], r["max_new"]) == (-1.0, -1.0)
    v20 = np.arange(20, dtype=F) - 10                               # n = 19: ranks 0 and 18
    assert model.ranks(20) == (0, 18)
    r = sel(v20[::-1])
    assert (r["min_new"], r["max_new"]) == (-10.0, 8.0)
    v21 = np.arange(21, dtype=F) - 10                               # n = 20: ranks 1 and 19
    assert model.ranks(21) == (1, 19)
    r = sel(v21)
    assert (r["min_new"], r["max_new"]) == (-9.0, 9.0)
    assert model.ranks(101) == (5, 95)
    v101 = np.arange(101, dtype=F) - 50
    r = sel(np.random.RandomState(0).permutation(v101))
    assert (r["min_new"], r["max_new"]) == (-45.0, 45.0)
    # -0 orders before +0: of {-0, +0} rank 0 is -0; of {+0 x 19, -0} rank 0 is -0 and rank 18 is +0
    r = sel([0.0, -0.0])
    assert np.signbit(r["min_new"]) and np.signbit(r["max_new"])
    r = sel([0.0] * 19 + [-0.0])
    assert np.signbit(r["min_new"]) and not np.signbit(r["max_new"])
    # NaNs are left out, infinities stay
    r = sel([NAN, 1.0, NAN, -INF, INF])
    assert r["n_values"] == 3 and (r["min_new"], r["max_new"]) == (-INF, 1.0)
    assert sel([NAN, NAN]) is None and sel([]) is None
    for v in ([3.0], [2.0, -1.0], v20, v21, v101, [0.0] * 19 + [-0.0], [NAN, 1.0, -INF, INF]):
        a, b = model.select(np.asarray(v, F), (0.1, 0.2)), model.select_fast(np.asarray(v, F), (0.1, 0.2))
        assert all(np.asarray(a[k], F).tobytes() == np.asarray(b[k], F).tobytes() for k in a)


def test_each_clamp_of_the_smoothing():
    # a stored value < 0: maxChange = 1e5, the new values pass and are stored
    assert [float(x) for x in model.smooth(0.5, 2.0, (-1.0, -1.0))[:2]] == [0.5, 2.0]
    assert model.smooth(0.5, 2.0, (-1.0, -1.0))[2].tolist() == [0.5, 2.0]
    assert float(model.smooth(-3e5, 2.0, (-1.0, 5.0))[0]) == float(F(F(-1.0) - F(1e5)))       # ... but 1e5 still clamps
    # span 1: maxChange = (float)(0.1 * 1.0)
    mc = F(0.1 * float(F(2.0) - F(1.0)))
    assert float(model.smooth(0.5, 2.0, (1.0, 2.0))[0]) == float(F(F(1.0) - mc))              # first if
    assert float(model.smooth(1.5, 2.0, (1.0, 2.0))[0]) == float(F(F(1.0) + mc))              # second if
    assert float(model.smooth(1.0, 1.5, (1.0, 2.0))[1]) == float(F(F(2.0) - mc))              # third if
    assert float(model.smooth(1.0, 2.5, (1.0, 2.0))[1]) == float(F(F(2.0) + mc))              # fourth if
    assert [float(x) for x in model.smooth(1.05, 1.95, (1.0, 2.0))[:2]] == [float(F(1.05)), float(F(1.95))]   # none
    assert model.smooth(0.5, 2.0, None) == (F(0.5), F(2.0), None)
    lo, hi, pair = model.smooth(0.5, 2.5, (1.0, 2.0))
    assert pair.tolist() == [float(lo), float(hi)]


def test_base_image_conversions():
    w, h = 8, 1
    I = np.array([0.0, 100.0, 283.0, 284.0, -1.2, -2.0, np.nan, 3e9], F)
    img = model.literal([dict(I=I)], w, h, 2)["bgr"][0][0, :, 0].tolist()
    assert img == [0, 90, 254, 255, 255, 255, 0, 255]                # -1.2 * 0.9 truncates to -1: wraps to 255; -2 * 0.9 = -1.8 too
    assert model.literal([dict(I=np.array([-3.0] * 8, F))], w, h, 2)["bgr"][0][0, 0, 0] == 254
