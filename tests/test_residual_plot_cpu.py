"""The host models of FullSystem::debugPlotTracking (tests/residual_plot_model.py) against each other and against hand-worked cases. No GPU.

The device painter (nalo_ba_residual_plot) is compared with these models in tests/test_residual_plot_gpu.py."""
import numpy as np

import residual_plot_model as rp
from window_plot_model import rainbow

F = np.float32
W_, H_ = 32, 24


def scene(n, W=3, seed=0, w=W_, h=H_):
    rng = np.random.RandomState(seed)
    I = [rng.uniform(-30, 330, w * h).astype(F) for _ in range(W)]
    aff = [(float(rng.uniform(0.5, 1.5)), float(rng.uniform(-40, 40))) for _ in range(W)]
    u, v = rng.uniform(-2, w + 2, n).astype(F), rng.uniform(-2, h + 2, n).astype(F)
    ids = rng.uniform(0.05, 3.0, n).astype(F)
    state = rng.randint(-1, 3, (n, W)).astype(np.int8)
    energy = rng.uniform(0, 3000, (n, W)).astype(F)
    proj = np.stack([rng.uniform(-1, w + 1, (n, W, 8)), rng.uniform(-1, h + 1, (n, W, 8))], axis=3).astype(F)
    return I, aff, u, v, ids, state, energy, proj


def both(I, aff, host, u, v, ids, state, energy, proj, w=W_, h=H_, **kw):
    a = rp.literal(I, aff, w, h, host, u, v, ids, state, energy, proj, **kw)
    b = rp.fast(I, aff, w, h, host, u, v, ids, state, energy, proj, **kw)
    assert np.array_equal(a["bgr"], b["bgr"]) and a["frames"] == b["frames"]
    assert (a["n_points"], a["n_residuals"], a["n_pattern_pixels"]) == (b["n_points"], b["n_residuals"], b["n_pattern_pixels"])
    return a


def test_fast_equals_literal_on_random_inputs():
    for seed in range(4):
        I, aff, u, v, ids, state, energy, proj = scene(60, seed=seed)
        if seed == 1:
            energy[::5] = [np.nan, -1.0, np.inf, 0.0][seed % 4]
            I[0][:4] = [np.nan, np.inf, -np.inf, 1e30]
            u[:3] = [np.nan, np.inf, -3e9]
            ids[:4] = [0.0, -1.0, np.nan, np.inf]
        for host in range(3):
            for p5 in (0.0, 1.0):
                both(I, aff, host, u, v, ids, state, energy, proj, param5=p5, rainbow_scale=[1.0, 0.4][host % 2], frame_mask=[0, 0b101, 0b010][host])


def flat(W=2, val=100.0):
    return [np.full(W_ * H_, val, F) for _ in range(W)], [(1.0, 0.0)] * W


def one(Ku, Kv, state=rp.IN, energy=0.0):
    """one point hosted by frame 0 with one residual to frame 1, all eight pattern pixels at (Ku, Kv)"""
    st = np.array([[-1, state]], np.int8)
    en = np.array([[0, energy]], F)
    pr = np.zeros((1, 2, 8, 2), F)
    pr[0, 1, :, 0], pr[0, 1, :, 1] = Ku, Kv
    return st, en, pr


def test_guard_either_side():
    I, aff = flat()
    w, h = W_, H_
    for (Ku, Kv), drawn in {(2.0, 10.0): 0, (np.nextafter(F(2), F(3)), 10.0): 8, (10.0, 2.0): 0, (10.0, np.nextafter(F(2), F(3))): 8,
                            (float(w - 3), 10.0): 0, (np.nextafter(F(w - 3), F(0)), 10.0): 8, (10.0, float(h - 3)): 0, (10.0, np.nextafter(F(h - 3), F(0))): 8,
                            (1.5, 10.0): 0, (np.nan, 10.0): 0}.items():
        st, en, pr = one(Ku, Kv)
        out = both(I, aff, 0, [20.0], [12.0], [1.0], st, en, pr, param5=1.0)
        assert out["n_residuals"] == 1 and out["n_pattern_pixels"] == drawn, (Ku, Kv)
        blue = np.argwhere(np.all(out["bgr"][1] == (255, 0, 0), axis=2))
        assert len(blue) == (1 if drawn else 0)
        if drawn:
            assert tuple(blue[0]) == (int(F(Kv) + F(0.5)), int(F(Ku) + F(0.5)))
    # just under w - 3 rounds UP to column w - 3: the last column the guard lets through
    st, en, pr = one(np.nextafter(F(w - 3), F(0)), 10.0)
    assert tuple(both(I, aff, 0, [20.0], [12.0], [1.0], st, en, pr, param5=1.0)["bgr"][1][10, w - 3]) == (255, 0, 0)


def test_state_colours_and_oob():
    I, aff = flat()
    for state, want in ((rp.IN, (255, 0, 0)), (rp.OUTLIER, (0, 0, 255)), (3, (255, 255, 255))):
        st, en, pr = one(10.0, 10.0, state)
        assert tuple(both(I, aff, 0, [20.0], [12.0], [1.0], st, en, pr, param5=0.5)["bgr"][1][10, 10]) == want
    for state in (rp.OOB, -1):
        st, en, pr = one(10.0, 10.0, state)
        out = both(I, aff, 0, [20.0], [12.0], [1.0], st, en, pr, param5=1.0)
        assert out["n_residuals"] == 0 and np.all(out["bgr"][1] == 100)


def test_energy_colours_with_the_clamps_and_nan():
    I, aff = flat()
    # rT = 20 sqrt(e / 9): e = 0 -> 0; e = 9 -> 20; e = 1463 -> 254.99.. -> byte 254; e = 1464 and above -> clamp 255; negative and NaN energy -> NaN -> (0, 0, 0)
    for e, want in ((0.0, (0, 255, 0)), (9.0, (0, 235, 20)), (1463.0, (0, 0, 254)), (1464.0, (0, 0, 255)), (1e30, (0, 0, 255)), (np.inf, (0, 0, 255)),
                    (-1.0, (0, 0, 0)), (np.nan, (0, 0, 0))):
        st, en, pr = one(10.0, 10.0, rp.OUTLIER, e)
        got = tuple(both(I, aff, 0, [20.0], [12.0], [1.0], st, en, pr, param5=0.0)["bgr"][1][10, 10])
        assert got == want == rp.energy_colour(e), (e, got)
    assert rp.energy_colour(2.25) == (0, 245, 10)                               # 255 - 10 exactly; fractions truncate on both channels:
    assert rp.energy_colour(1.0) == (0, 248, 6)                                 # rT = 6.67 -> 6, 255 - rT = 248.3 -> 248


def test_brightness_transfer_and_its_clamps():
    I = [np.array([0.0, 100.0, 300.0, -50.0, np.nan, np.inf, -np.inf, 50.4] + [10.0] * (W_ * H_ - 8), F) for _ in range(2)]
    aff = [(1.0, 0.0), (2.0, -100.0)]
    st, en, pr = one(10.0, 10.0, -1)
    out = both(I, aff, 0, [], [], [], st[:0], en[:0], pr[:0])
    assert out["bgr"][0].reshape(-1, 3)[:8, 0].tolist() == [0, 100, 255, 0, 0, 255, 0, 50]
    assert out["bgr"][1].reshape(-1, 3)[:8, 0].tolist() == [0, 100, 255, 0, 0, 255, 0, 0]      # 2 I - 100: -100 -> 0, 100, 500 -> 255, .., 0.8 -> 0
    assert np.all(out["bgr"][..., 0] == out["bgr"][..., 1]) and np.all(out["bgr"][..., 0] == out["bgr"][..., 2])
    # the product and the sum are in double: a float product would round 16777217 away
    assert rp.base_byte(F(16777216.0), 1.0 + 2.0 ** -24, -16777216.0) == 1
    a, b = rp.aff_l(0.5, 2.0, 0.1, 3.0, 0.3, 5.0)
    assert abs(a - np.exp(0.2) * 4.0) < 1e-14 * a and abs(b - (5.0 - a * 3.0)) < 1e-13
    assert rp.aff_l(0.0, 2.0, 0.0, 0.0, 0.0, 7.0) == (1.0, 7.0)                 # an exposure of 0: both count as 1


def test_two_points_on_the_same_pixel_last_index_wins():
    I, aff = flat()
    st = np.array([[-1, rp.OUTLIER], [-1, rp.OUTLIER]], np.int8)
    en = np.array([[0, 9.0], [0, 36.0]], F)
    pr = np.zeros((2, 2, 8, 2), F)
    pr[..., 0], pr[..., 1] = 10.0, 10.0
    a = both(I, aff, 0, [20.0, 20.0], [12.0, 12.0], [1.0, 1.7], st, en, pr)
    assert tuple(a["bgr"][1][10, 10]) == rp.energy_colour(36.0) == (0, 215, 40)
    assert tuple(a["bgr"][0][12, 20]) == rainbow(F(1.7))                        # the squares too
    b = both(I, aff, 0, [20.0, 20.0], [12.0, 12.0], [1.7, 1.0], st, en[::-1], pr)
    assert tuple(b["bgr"][1][10, 10]) == rp.energy_colour(9.0) and tuple(b["bgr"][0][12, 20]) == rainbow(F(1.0))
    assert a["n_pattern_pixels"] == 16 and a["n_residuals"] == 2 and a["n_points"] == 2


def test_square_is_on_the_host_image_clipped_and_the_mask_selects_images():
    I, aff = flat(W=3)
    st = np.full((1, 3), -1, np.int8); en = np.zeros((1, 3), F); pr = np.zeros((1, 3, 8, 2), F)
    out = both(I, aff, 1, [0.2], [H_ - 0.7], [1.0], st, en, pr)
    sq = np.argwhere(np.all(out["bgr"][1] == rainbow(F(1.0)), axis=2))
    assert sorted(map(tuple, sq)) == [(H_ - 2, 0), (H_ - 2, 1), (H_ - 1, 0), (H_ - 1, 1)]      # (int)(0.7) = 0, (int)(H - 0.2) = H - 1: the corner keeps four
    assert np.all(out["bgr"][0] == 100) and np.all(out["bgr"][2] == 100)
    m = both(I, aff, 1, [0.2], [H_ - 0.7], [1.0], st, en, pr, frame_mask=0b101)
    assert m["frames"] == [0, 2] and m["bgr"].shape[0] == 2 and np.all(m["bgr"] == 100) and m["n_points"] == 1
