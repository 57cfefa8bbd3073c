"""Planted level-0 inverse-depth maps and the irradiance image for the nalo_trk_depth_image tests: maps the scatter and dilation of nalo_trk_set_ref never
produce, shared by the host-model test (fast == literal) and the device test (device == fast)."""
import numpy as np

F = np.float32
# 283.3 * 0.9f truncates to 254, 283.4 * 0.9f to 255 (the clamp's edge); 1e10 and +inf saturate the conversion; -1 -> 0, -2.5 -> -2 -> byte 254; NaN -> 0
SPECIAL_I = [0.0, 283.3, 283.4, 300.0, 1e10, -1.0, -2.5, np.nan, np.inf]


def image(w, h, seed=11):
    """irradiance with the special values in the top row (which few rings reach), in the middle and in the last row"""
    rng = np.random.RandomState(seed)
    I = rng.uniform(0.0, 300.0, (h, w)).astype(F)
    for y in (0, h // 2, h - 1):
        for k, v in enumerate(SPECIAL_I):
            I[y, 2 + 3 * k] = v
    return I


def _with(w, h, pts):
    m = np.zeros((h, w), F)
    for (x, y), v in pts.items():
        m[y, x] = v
    return m


def n_positive_map(w, h, k, seed):
    rng = np.random.RandomState(seed)
    m = np.zeros(w * h, F)
    m[rng.choice(w * h, k, replace=False)] = rng.uniform(0.05, 4.0, k).astype(F)
    return m.reshape(h, w)


def planted(w, h):
    """[(name, map)] at w x h (w >= 64, h >= 32)"""
    rng = np.random.RandomState(5)
    out = []
    for name, (x, y) in (("single_3_3", (3, 3)), ("single_last", (w - 4, h - 4)), ("single_x2_noplot", (2, 5)), ("single_xw3_noplot", (w - 3, 5))):
        out.append((name, _with(w, h, {(x, y): 0.7})))
    out.append(("corners", _with(w, h, {(3, 3): 0.2, (w - 4, 3): 0.4, (3, h - 4): 0.8, (w - 4, h - 4): 1.6})))
    # a non-positive centre with three / four positive neighbours plots through nid >= 3 (the neighbours plot themselves); 30,20: centre NaN
    out.append(("nid3", _with(w, h, {(11, 10): 0.5, (9, 10): 0.6, (10, 11): 0.9, (10, 10): 0.0,
                                     (21, 12): 0.3, (19, 12): 0.35, (20, 13): 0.4, (20, 11): 0.45, (20, 12): -1.0,
                                     (31, 20): 1.0, (29, 20): 1.1, (30, 19): 1.2, (30, 20): np.nan})))
    out.append(("two_neighbours", _with(w, h, {(11, 10): 0.5, (9, 10): 0.6, (40, 21): 0.7, (40, 19): 0.8})))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checkerboard", np.where((xx + yy) % 2 == 0, 0.1 + 0.01 * ((xx * 7 + yy * 13) % 97), 0.0).astype(F)))
    out.append(("full_distinct", rng.permutation(np.linspace(0.01, 3.0, w * h)).astype(F).reshape(h, w)))
    const = np.full((h, w), 0.5, F)                                      # both quantiles 0.5: 0/0 = NaN (white) where the stencil's mean is 0.5, +inf / -inf elsewhere
    const[8, 8], const[8, 20], const[20, 30], const[12, 50] = 0.25, 2.0, 0.0, 0.125
    out.append(("constant", const))
    sp = rng.uniform(0.1, 2.0, (h, w)).astype(F)
    sp[rng.rand(h, w) < 0.5] = 0.0
    vals = [np.inf, np.nan, -0.0, -1.5, -np.inf, 1e-45, 1e-40, -1e-42, 3.4e38]
    for k in range(90):
        sp[3 + (k * 5) % (h - 6), 3 + (k * 11) % (w - 6)] = vals[k % len(vals)]
    out.append(("specials", sp))
    den = np.zeros((h, w), F)                                            # denormals only: the select's top-level bin 0
    den.reshape(-1)[::3] = (np.arange(len(den.reshape(-1)[::3])) % 200 + 1).astype(np.uint32).view(F)
    out.append(("denormals", den))
    for k in (1, 2, 20, 21, 22, 101):
        out.append(("npos_%d" % k, n_positive_map(w, h, k, 100 + k)))
    low = (np.uint32(0x3F800000) + (rng.permutation(w * h) % 700).astype(np.uint32)).view(F).reshape(h, w)   # 1.0 + j ulp: the select's last level decides
    out.append(("low_bits", low.copy()))
    ties = np.array([0.25, 0.5, 0.5000001, 1.0, 1.5, 2.0, 3.0], F)[rng.randint(0, 7, w * h)].reshape(h, w)   # both ranks fall inside runs of equal values
    out.append(("ties", ties))
    return out
