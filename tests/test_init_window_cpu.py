"""tests/init_window_model.py - the literal model of FullSystem::initializeFromInitializer (reference FullSystem.cpp:1589-1648) plus the insertion of the second
frame (:1335-1348) - on hand-built inputs whose results are worked out by hand. tests/test_init_window_gpu.py compares nalo_ba_window_from_initializer with it."""
import numpy as np

import init_window_model as iw
import lifecycle_model as lm

F32 = np.float32


def straddle(keep):
    """the two neighbouring ints around keepPercentage * 2^31 between which the literal rule changes its answer, and floor / ceil of the product itself"""
    x = float(keep) * 2147483648.0
    lo = int(np.floor(x))
    d = lo - 200
    while not iw.skipped(d + 1, keep):
        d += 1
    return d, d + 1, lo, lo + 1


def test_the_sum_is_sequential():
    # 1e-5 + 2^24 rounds to 2^24 (the ulp there is 2); each 1 added after that is half an ulp and is rounded away (ties to even): the sequential float sum of
    # [2^24, 1, 1, 1, 1] is 2^24, where a pairwise sum (2^24 + 1 -> 2^24, 1 + 1 = 2, ...) and an fp64 sum rounded once both give 2^24 + 4
    iR = np.array([2.0 ** 24, 1, 1, 1, 1], np.float32)
    sumID, numID, rescale = iw.scale(iR)
    assert sumID == F32(2.0 ** 24)
    assert iw.pairwise_sum(iR) == F32(2.0 ** 24 + 4) and iw.fp64_sum(iR) == F32(2.0 ** 24 + 4)
    # numID: 1e-5f + 1 = 1.00001001..f (rounded), then four exact steps of 1 up to the rounding of each: worked out in fp32
    want = F32(1e-5)
    for _ in range(5):
        want = F32(want + F32(1))
    assert numID == want and abs(float(numID) - 5.00001) < 1e-6
    assert rescale == F32(F32(1) / F32(F32(2.0 ** 24) / want))
    # the order matters the other way round too: the small values first survive
    s2, _, _ = iw.scale(iR[::-1])
    assert s2 == F32(2.0 ** 24 + 4)
    # an empty level: both sums stay at 1e-5f, the factor is 1
    assert iw.scale(np.zeros(0, np.float32)) == (F32(1e-5), F32(1e-5), F32(1))


def test_the_keep_rule():
    n, density = 10000, 2000.0
    keep = iw.keep_percentage(density, n)
    assert keep == F32(0.2)
    assert not iw.skipped(0, keep)                                           # 0 / 2^31 = 0 is never above a positive percentage
    assert iw.skipped(2 ** 31 - 1, keep)                                     # (float)(2^31 - 1) = 2^31: the ratio is exactly 1
    assert not iw.skipped(2 ** 31 - 1, iw.keep_percentage(1e9, n))           # keepPercentage >= 1 keeps every point
    last_kept, first_skipped, lo, hi = straddle(keep)
    assert first_skipped == last_kept + 1 and not iw.skipped(last_kept, keep) and iw.skipped(first_skipped, keep)
    # F32(0.2) = 13421773 * 2^-26: times 2^31 it is the integer 429496736, whose float is exact (a multiple of 32), so the ratio of that draw EQUALS
    # keepPercentage and is kept; ints are rounded to multiples of 32 there, and 13421773 is odd, so the tie 429496736 + 16 rounds to the even neighbour above:
    # the answer changes between +15 and +16
    assert lo == 429496736 and float(keep) * 2 ** 31 == lo
    assert not iw.skipped(lo, keep) and not iw.skipped(hi, keep)
    assert (last_kept, first_skipped) == (lo + 15, lo + 16)
    # every point consumes exactly one draw, kept or not: the selection of point i depends on draws[i] alone
    draws = np.full(n, 2 ** 31 - 1, np.int64)
    draws[[0, 63, 64, 255, 256, n - 1]] = 0
    assert iw.select(draws, density).tolist() == [0, 63, 64, 255, 256, n - 1]


def test_pixel_rounding_and_the_history_constants():
    assert iw.pixel(F32(3.1), F32(7.1)) == (3, 7) and iw.pixel(F32(3.5), F32(7.49)) == (4, 7)
    u = np.array([3.1, 10.1, 20.1], np.float32)
    v = np.array([4.1, 5.1, 6.1], np.float32)
    iR = np.array([0.5, 2.0, 1.5], np.float32)
    w = iw.window(u, v, iR, np.array([0, 1, 2], np.int32), np.array([100.0, np.nan, 100.0], np.float32), np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1))
    assert w["src"].tolist() == [0, 2] and w["rejected"] == 1                 # a point whose energyTH is not finite is rejected, the others keep their order
    assert w["u"].tolist() == [3.0, 20.0] and w["v"].tolist() == [4.0, 6.0] and w["host"].tolist() == [0, 0] and w["has_prior"].tolist() == [1, 1]
    sumID, numID, rescale = w["scale"]
    assert sumID == F32(F32(F32(F32(1e-5) + F32(0.5)) + F32(2.0)) + F32(1.5))
    assert np.array_equal(w["idepth"], np.array([F32(0.5) * rescale, F32(1.5) * rescale], np.float32))
    assert w["exists"].tolist() == [[0, 1], [0, 1]]                           # one residual, to frame 1
    ng, lt, ls = w["hist"]
    assert ng.tolist() == [0, 0] and lt.tolist() == [[1, -1], [1, -1]]
    assert ls.tolist() == [[lm.IN, lm.IN], [lm.IN, lm.IN]] and lm.IN == 0     # slot 1 is IN - the value-initialised pair, shifted - not the OOB of a fresh activation


def test_pure_translation_in_closed_form():
    t = np.array([0.3, -0.1, 1.7])
    T = np.concatenate([np.eye(3), t[:, None]], axis=1)
    iR = np.array([0.5, 0.25, 0.125], np.float32)
    _, _, rescale = iw.scale(iR)
    got = iw.entering_pose(T, rescale)
    assert np.array_equal(got[:, :3], np.eye(3))
    assert np.array_equal(got[:, 3], t / np.float64(rescale))                # -(-(t / r)) exactly
    w = iw.window(np.zeros(3, np.float32) + F32(5.1), np.zeros(3, np.float32) + F32(5.1), iR, np.zeros(0, np.int32), np.zeros(0, np.float32), T)
    assert np.array_equal(w["poses"][0], np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)) and np.array_equal(w["poses"][1], got)
    # with a rotation the two inversions give R and R^T R t' up to rounding
    a = 0.2
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    got = iw.entering_pose(np.concatenate([R, t[:, None]], axis=1), rescale)
    assert np.array_equal(got[:, :3], R) and np.abs(got[:, 3] - t / np.float64(rescale)).max() <= 16 * 2.0 ** -52 * max(1.0, np.linalg.norm(t / np.float64(rescale)))
