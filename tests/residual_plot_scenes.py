"""Planted windows for tests/test_residual_plot_gpu.py: small frames of ONE fronto-parallel plane seen by cameras that differ by a sub-two-pixel translation, so
that every residual's fate is decided by where the point was put.

The scene radiance R(x, y) is smooth; frame i shows exposure_i * exp(a_i) * R(x - sx_i, y - sy_i) + b_i, which the reference's brightness transfer between any two
frames maps exactly onto each other (AffLight::fromToVecExposure), so a residual of a point on the plane (idepth ~ 1) is IN. The last frame carries an extra
brightness step on its right half: residuals that land there become OUTLIER. Points two to three pixels from the left / top border have pattern pixels that
project to (1.1, 2] in the frame shifted towards that border - IN, but behind the plot's guard - and points one pixel closer leave it: OOB."""
import numpy as np

from nalo_slam_amd import synth
from nalo_slam_amd.synth import PATTERN

F = np.float32
SHIFT = [(0.0, 0.0), (-1.6, -1.3), (1.2, 0.7), (0.9, -1.1)]                      # pixels at idepth 1, per frame (W <= 4)
EXPOSURE = [1.0, 1.5, 0.8, 1.2]
AFF = [(0.0, 0.0), (0.2, -30.0), (-0.1, 12.0), (0.05, -8.0)]                     # aff_g2l (a, b) per frame
STEP = 60.0                                                                     # the brightness step on the right half of the last frame


def radiance(x, y):
    return 80.0 + 50.0 * np.sin(0.35 * x) + 40.0 * np.cos(0.3 * y) + 20.0 * np.sin(0.2 * (x + y))


def planted(w, h, W, sizes, seed):
    """-> synth.Window (images, poses, points, colours, the full residual graph) and the per-frame (aff, exposure) lists"""
    rng = np.random.RandomState(seed)
    f = 0.5 * w
    K = (f, f, (w - 1) / 2.0, (h - 1) / 2.0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    images = np.zeros((W, h, w), F)
    w2c = np.zeros((W, 3, 4))
    for i in range(W):
        sx, sy = SHIFT[i]
        img = EXPOSURE[i] * np.exp(AFF[i][0]) * radiance(xx - sx, yy - sy) + AFF[i][1]
        if i == W - 1:
            img[:, w // 2:] += STEP
        images[i] = img.astype(F)
        w2c[i, :, :3] = np.eye(3)
        w2c[i, :, 3] = (sx / f, sy / f, 0.0)
    host, u, v = [], [], []
    for i, n in enumerate(sizes):
        # the border cases first (columns / rows 4 and 5, and their mirror images), then random interior positions that overlap freely
        uv = [(4, 9), (5, 9), (5, 12), (9, 4), (9, 5), (12, 5), (w - 5, 9), (w - 6, 9), (9, h - 5), (9, h - 6), (5, 5), (4, 4)]
        uv += list(zip(rng.randint(4, w - 4, max(n, 1)), rng.randint(4, h - 4, max(n, 1))))
        uv = uv[:n] if n > 2 else [(w // 2 - 3, h // 2), (w // 2 + 6, h // 2 + 1)][:n]
        host += [i] * n
        u += [p[0] for p in uv]; v += [p[1] for p in uv]
    order = rng.permutation(len(host))                                           # hosts interleaved in submission order
    host, u, v = np.array(host, np.int32)[order], np.array(u, np.int64)[order], np.array(v, np.int64)[order]
    P = len(host)
    idepth = (1.0 + 0.02 * rng.randn(P)).astype(F)
    color = np.zeros((P, 8), F)
    for k in range(8):
        color[:, k] = images[host, v + PATTERN[k, 1], u + PATTERN[k, 0]]
    # two points at the same (u, v) and inverse depth, the second with colours that are off: the same pixels, another energy
    # (left of the brightness step and clear of the borders, so that both stay IN)
    twins = [p for p in range(P - 1) if host[p] == host[p + 1] and 8 <= u[p] < w // 2 - 8 and 8 <= v[p] < h - 8][:3]
    for p in twins:
        u[p + 1], v[p + 1], idepth[p + 1] = u[p], v[p], idepth[p]
        color[p + 1] = color[p] + F(1.5)
    exists = np.ones((P, W), np.uint8)
    exists[np.arange(P), host] = 0
    win = synth.Window(w, h, 1, K, images, np.ones((W, h, w), F), w2c, W, host, u.astype(F), v.astype(F), idepth, idepth.copy(), color, np.ones((P, 8), F), exists)
    return win, AFF[:W], EXPOSURE[:W]
