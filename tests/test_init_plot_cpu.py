"""The host models of CoarseInitializer::debugPlot (tests/init_plot_model.py) against each other and against hand-worked cases. No GPU.

The device painter (nalo_init_depth_image) is compared with these models in tests/test_init_plot_gpu.py; what no public input reaches on the device (a square
clipped at a border: the initialiser keeps its points three pixels inside) is pinned here."""
import numpy as np

import init_plot_model as ip
from window_plot_model import rainbow

F = np.float32
W, H = 24, 16


def grey(val=7.0, w=W, h=H):
    return np.full(w * h, val, F)


def paint(u, v, iR, good, I=None, w=W, h=H, scale=1.0):
    a = [np.asarray(x, F) for x in (u, v, iR)]
    I = grey(w=w, h=h) if I is None else I
    lit = ip.literal(I, w, h, a[0], a[1], a[2], np.asarray(good, np.uint8), scale)
    fst = ip.fast(I, w, h, a[0], a[1], a[2], np.asarray(good, np.uint8), scale)
    assert np.array_equal(lit["bgr"], fst["bgr"])
    assert lit["n_good"] == fst["n_good"] and ip.same_float(lit["sum_iR"], fst["sum_iR"]) and ip.same_float(lit["fac"], fst["fac"])
    return lit


def block(img, x, y):
    return img[y - 1:y + 2, x - 1:x + 2].reshape(-1, 3)


def test_fast_equals_literal_on_random_inputs():
    rng = np.random.RandomState(0)
    for trial in range(6):
        n = 80
        u = rng.uniform(-3, W + 3, n).astype(F); v = rng.uniform(-3, H + 3, n).astype(F)
        iR = rng.uniform(0.05, 3.0, n).astype(F)
        good = rng.randint(0, 2, n).astype(np.uint8)
        if trial == 1:
            iR[::7] = [0.0, -0.0, -1.0, np.nan, np.inf, 1e30, 1e-42, 3e9][trial % 8]
        if trial == 2:
            iR[:8] = [0.0, -0.0, -1.0, np.nan, np.inf, 1e30, 1e-42, 1e-45]
            good[:8] = 1
        if trial == 3:
            u[:4] = [np.nan, np.inf, -np.inf, 3e9]; v[4:8] = [np.nan, np.inf, -np.inf, -3e9]
        I = rng.uniform(-40, 320, W * H).astype(F)
        I[:4] = [np.nan, np.inf, -np.inf, 1e20]
        paint(u, v, iR, good, I, scale=[1.0, 0.37, 2.5][trial % 3])


def test_base_image_conversion():
    I = grey()
    I[:9] = [0.0, 0.99, 254.7, 255.0, 256.0, 300.0, -1.0, -0.5, np.nan]
    I[9:12] = [np.inf, -np.inf, 1e20]
    out = paint([], [], [], [], I)
    got = out["bgr"].reshape(-1, 3)
    # truncation, wrap at 256, (unsigned char)-1 = 255, -0.5 -> 0, NaN -> 0, INT_MAX & 255 = 255, INT_MIN & 255 = 0
    assert got[:12, 0].tolist() == [0, 0, 254, 255, 0, 44, 255, 0, 0, 255, 0, 255]
    assert np.all(got[:, 0] == got[:, 1]) and np.all(got[:, 0] == got[:, 2]) and np.all(got[12:] == 7)
    assert out["n_points"] == 0 and out["n_good"] == 0 and np.isnan(out["fac"]) and out["sum_iR"] == 0


def test_two_overlapping_squares_both_orders():
    # iR equal -> fac = 1 / iR mean; use two different iR so the colours differ
    u, v, iR = [5.1, 6.1], [5.1, 5.1], [1.0, 0.5]
    a = paint(u, v, iR, [1, 1])
    fac = a["fac"]
    c0, c1 = rainbow(F(F(1.0) * fac)), rainbow(F(F(0.5) * fac))
    assert c0 != c1
    img = a["bgr"]
    assert all(tuple(img[y, 4]) == c0 for y in (4, 5, 6))                    # only the first point covers x = 4
    assert all(tuple(img[y, x]) == c1 for y in (4, 5, 6) for x in (5, 6, 7))  # the second wins the shared columns
    b = paint(u[::-1], v, iR[::-1], [1, 1])["bgr"]
    assert all(tuple(b[y, x]) == c0 for y in (4, 5, 6) for x in (4, 5, 6))    # now the point at x = 5 is last
    assert all(tuple(b[y, 7]) == c1 for y in (4, 5, 6))
    assert tuple(img[3, 5]) == (7, 7, 7) and tuple(img[7, 5]) == (7, 7, 7)


def test_bad_point_over_good_and_reverse():
    good_first = paint([5.1, 5.1], [5.1, 5.1], [1.0, 1.0], [1, 0])
    assert np.all(block(good_first["bgr"], 5, 5) == 0) and good_first["n_good"] == 1
    bad_first = paint([5.1, 5.1], [5.1, 5.1], [1.0, 1.0], [0, 1])
    assert np.all(block(bad_first["bgr"], 5, 5) == np.array(rainbow(F(1.0)), np.uint8))   # fac = 1 / 1


def test_square_clipped_at_each_border():
    # (int)(-0.4f + 0.5f) = 0 and (int)(W - 0.6f + 0.5f) = W - 1: the centre lies on the border column / row and one line of the block is outside
    cases = {(-0.4, 5.1): ((0, 1), (4, 5, 6)), (W - 0.6, 5.1): ((W - 2, W - 1), (4, 5, 6)),
             (5.1, -0.4): ((4, 5, 6), (0, 1)), (5.1, H - 0.6): ((4, 5, 6), (H - 2, H - 1))}
    for (u, v), (xs, ys) in cases.items():
        img = paint([u], [v], [1.0], [0])["bgr"]
        black = {(x, y) for y in range(H) for x in range(W) if tuple(img[y, x]) == (0, 0, 0)}
        assert black == {(x, y) for x in xs for y in ys}, (u, v)
    # a corner keeps four pixels, a centre one pixel outside keeps one line, two pixels outside nothing
    assert int(np.sum(np.all(paint([0.2], [0.2], [1.0], [0])["bgr"] == 0, axis=2))) == 4
    assert int(np.sum(np.all(paint([-1.4], [5.1], [1.0], [0])["bgr"] == 0, axis=2))) == 6      # (int)(-0.9f) = 0: truncation toward zero
    assert int(np.sum(np.all(paint([-2.4], [5.1], [1.0], [0])["bgr"] == 0, axis=2))) == 3      # (int)(-1.9f) = -1
    assert int(np.sum(np.all(paint([-3.4], [5.1], [1.0], [0])["bgr"] == 0, axis=2))) == 0
    assert int(np.sum(np.all(paint([W + 0.6], [5.1], [1.0], [0])["bgr"] == 0, axis=2))) == 0


def test_all_three_rainbow_branches_and_white():
    # one good point: fac = 1 / iR, so iR * fac = 1 (up to rounding); the branch is chosen through rainbow_scale
    for scale, want in ((0.5, (127, 127, 0)), (1.5, (0, 127, 127)), (2.5, (127, 0, 127))):
        out = paint([5.1], [5.1], [1.0], [1], scale=scale)
        assert out["fac"] == 1 and tuple(out["bgr"][5, 5]) == want == rainbow(F(1.0), scale)
    assert tuple(paint([5.1], [5.1], [1.0], [1], scale=-1.0)["bgr"][5, 5]) == (255, 255, 255)     # !(id > 0)
    assert tuple(paint([5.1], [5.1], [1.0], [1], scale=3e9)["bgr"][5, 5]) == (255, 255, 255)      # int cannot hold it
    assert tuple(paint([5.1], [5.1], [np.nan], [1])["bgr"][5, 5]) == (255, 255, 255)


def test_fac_without_good_points_and_with_a_zero_sum():
    none = paint([5.1, 9.1], [5.1, 5.1], [1.0, 2.0], [0, 0])
    assert none["n_good"] == 0 and none["sum_iR"] == 0 and np.isnan(none["fac"])
    assert np.all(block(none["bgr"], 5, 5) == 0) and np.all(block(none["bgr"], 9, 5) == 0)
    zero = paint([5.1, 9.1], [5.1, 5.1], [1.0, -1.0], [1, 1])
    assert zero["n_good"] == 2 and zero["sum_iR"] == 0 and np.isposinf(zero["fac"])
    assert tuple(zero["bgr"][5, 5]) == (255, 255, 255) and tuple(zero["bgr"][5, 9]) == (255, 255, 255)   # +inf: int cannot hold it; -inf: !(id > 0)
    zz = paint([5.1], [5.1], [0.0], [1])
    assert np.isposinf(zz["fac"]) and tuple(zz["bgr"][5, 5]) == (255, 255, 255)                           # 0 * inf = NaN


def test_sequential_float_sum_is_not_the_fp64_sum():
    for n in (300, 5000):
        iR = ip.sum_order_set(n)
        good = np.ones(n, np.uint8)
        n_good, sid, fac = ip.scale(iR, good)
        n2, sid2, fac2 = ip.scale_fast(iR, good)
        assert n_good == n2 == n and ip.same_float(sid, sid2) and ip.same_float(fac, fac2)
        assert sid != F(np.sum(iR.astype(np.float64))), "the set does not tell the chain from an fp64 sum"
        assert sid != np.sum(iR, dtype=F), "the set does not tell the chain from a pairwise sum"
        # bad points are left out of the chain, not added as zeros in another order
        good[1::2] = 0
        n3, sid3, _ = ip.scale(iR, good)
        assert n3 == (n + 1) // 2 and ip.same_float(sid3, ip.scale_fast(iR, good)[1]) and sid3 != sid
