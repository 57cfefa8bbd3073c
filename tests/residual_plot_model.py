"""Host models of one outer iteration of FullSystem::debugPlotTracking (FullSystemDebugStuff.cpp:52-107) with PointFrameResidual::debugPlot
(Residuals.cpp:278-302), for nalo_ba_residual_plot.

Inputs, for host frame `host` of a window of W frames: I[f] (w * h irradiance, level 0) and aff[f] = (a, b) of every frame (aff_l() below, in double); the host's
valid points in the library's order (submission order): u, v, idepth_scaled [n]; per point and window row state [n][W] (-1 no residual, 0 IN, 1 OOB, 2 OUTLIER),
state_energy [n][W] and the pattern projections proj [n][W][8][2]. literal(): the reference's loops one to one; np.float32 scalars carry the float arithmetic and
Python floats the double arithmetic. fast(): the same result vectorised (the last writer as the maximum point index per pixel). Both use the conversions the
library DEFINES where the reference is undefined (include/nalo_gpu.h).

Both return a dict: bgr (n_frames, h, w, 3) uint8, frames (window indices of the returned images), n_points, n_residuals, n_pattern_pixels (counted over every
target, whatever the mask)."""
import numpy as np

from init_plot_model import SQUARE
from window_plot_model import F, _byte_vec, _rainbow_vec, color_byte, painted, rainbow

IN, OOB, OUTLIER = 0, 1, 2
STATE_COLOUR = {IN: (255, 0, 0), OUTLIER: (0, 0, 255)}
WHITE = (255, 255, 255)


def aff_l(exp_from, exp_to, a_from, b_from, a_to, b_to):
    """AffLight::fromToVecExposure(exposureF, exposureT, g2F, g2T) in double; a, b are aff_g2l (the scaled state)"""
    exp_from, exp_to = float(F(exp_from)), float(F(exp_to))
    if exp_from == 0 or exp_to == 0:
        exp_from = exp_to = 1.0
    a = float(np.exp(np.float64(a_to) - np.float64(a_from))) * exp_to / exp_from
    return a, float(b_to) - a * float(b_from)


def to_int_d(x):
    """double -> int: truncation toward zero, saturating, NaN -> 0"""
    x = float(x)
    if x != x:
        return 0
    return int(min(max(x, -2147483648.0), 2147483647.0))


def base_byte(I, a, b):
    """:79-81: the product and the sum in double, the clamps in float; NaN -> 0"""
    with np.errstate(all="ignore"):
        colL = F(np.float64(a) * np.float64(F(I)) + np.float64(b))
    if colL < 0:
        colL = F(0)
    if colL > 255:
        colL = F(255)
    return color_byte(colL)


def energy_colour(e):
    """Residuals.cpp:285-287: the quotient in float, sqrt and the product in double"""
    with np.errstate(all="ignore"):
        rT = F(20.0 * np.sqrt(np.float64(F(F(e) / F(9)))))
        if rT < 0:
            rT = F(0)
        if rT > 255:
            rT = F(255)
        return (0, color_byte(F(F(255) - rT)), color_byte(rT))


def state_colour(s):
    return STATE_COLOUR.get(int(s), WHITE)


def guard(Ku, Kv, w, h):
    return bool(F(Ku) > 2 and F(Kv) > 2 and F(Ku) < F(w - 3) and F(Kv) < F(h - 3))


def literal(I, aff, w, h, host, u, v, idepth_scaled, state, energy, proj, param5=0.0, rainbow_scale=1.0, frame_mask=0):
    W = len(I)
    images = []
    for f2 in range(W):
        src = np.ascontiguousarray(I[f2], F).reshape(-1)
        img = np.zeros((h, w, 3), np.uint8)
        for i in range(w * h):
            img[i // w, i % w, :] = base_byte(src[i], aff[f2][0], aff[f2][1])
        images.append(img)
    n_res = n_px = 0
    for k in range(len(u)):
        for t in range(W):
            if t == host or state[k][t] < 0 or state[k][t] == OOB:
                continue
            cT = energy_colour(energy[k][t]) if param5 == 0 else state_colour(state[k][t])
            n_res += 1
            for i in range(8):
                Ku, Kv = F(proj[k][t][i][0]), F(proj[k][t][i][1])
                if guard(Ku, Kv, w, h):
                    n_px += 1
                    images[t][int(F(Kv + F(0.5))), int(F(Ku + F(0.5))), :] = cT          # setPixel1
        cu, cv = to_int_d(float(F(u[k])) + 0.5), to_int_d(float(F(v[k])) + 0.5)
        col = rainbow(idepth_scaled[k], rainbow_scale)
        for dx, dy in SQUARE:
            if 0 <= cu + dx < w and 0 <= cv + dy < h:
                images[host][cv + dy, cu + dx, :] = col
    sel = painted(W, frame_mask)
    return {"bgr": np.stack([images[f] for f in sel]), "frames": sel, "n_points": len(u), "n_residuals": n_res, "n_pattern_pixels": n_px}


def fast(I, aff, w, h, host, u, v, idepth_scaled, state, energy, proj, param5=0.0, rainbow_scale=1.0, frame_mask=0):
    W, n = len(I), len(u)
    state = np.asarray(state).reshape(n, W)
    energy = np.asarray(energy, F).reshape(n, W)
    proj = np.asarray(proj, F).reshape(n, W, 8, 2)
    images = []
    with np.errstate(all="ignore"):
        for f2 in range(W):
            colL = (np.float64(aff[f2][0]) * np.ascontiguousarray(I[f2], F).reshape(h, w).astype(np.float64) + np.float64(aff[f2][1])).astype(F)
            colL = np.where(colL < 0, F(0), colL)
            colL = np.where(colL > 255, F(255), colL)
            images.append(np.repeat(_byte_vec(colL).astype(np.uint8)[:, :, None], 3, axis=2))
        live = (state >= 0) & (state != OOB)
        live[:, host] = False
        rT = (20.0 * np.sqrt((energy / F(9)).astype(F).astype(np.float64))).astype(F)
        rT = np.where(rT < 0, F(0), rT)
        rT = np.where(rT > 255, F(255), rT).astype(F)
        e_col = np.stack([np.zeros_like(rT, np.int64), _byte_vec((F(255) - rT).astype(F)), _byte_vec(rT)], axis=2).astype(np.uint8)
    s_col = np.full((n, W, 3), 255, np.uint8)
    s_col[state == IN] = STATE_COLOUR[IN]
    s_col[state == OUTLIER] = STATE_COLOUR[OUTLIER]
    col = e_col if param5 == 0 else s_col
    Ku, Kv = proj[..., 0], proj[..., 1]
    ok = (Ku > 2) & (Kv > 2) & (Ku < F(w - 3)) & (Kv < F(h - 3)) & live[:, :, None]
    order = np.arange(n, dtype=np.int64)
    for t in range(W):
        if t == host:
            continue
        best = np.full(w * h, -1, np.int64)
        for i in range(8):
            m = ok[:, t, i]
            x, y = (Ku[m, t, i] + F(0.5)).astype(F).astype(np.int64), (Kv[m, t, i] + F(0.5)).astype(F).astype(np.int64)
            np.maximum.at(best, y * w + x, order[m])
        hit = best >= 0
        images[t].reshape(-1, 3)[hit] = col[best[hit], t]
    if n:
        with np.errstate(all="ignore"):
            cu = np.where(np.isnan(np.asarray(u, F)), 0.0, np.clip(np.asarray(u, F).astype(np.float64) + 0.5, -2147483648.0, 2147483647.0)).astype(np.int64)
            cv = np.where(np.isnan(np.asarray(v, F)), 0.0, np.clip(np.asarray(v, F).astype(np.float64) + 0.5, -2147483648.0, 2147483647.0)).astype(np.int64)
        sq = _rainbow_vec(np.asarray(idepth_scaled, F), rainbow_scale)
        best = np.full(w * h, -1, np.int64)
        for dx, dy in SQUARE:
            x, y = cu + dx, cv + dy
            m = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            np.maximum.at(best, y[m] * w + x[m], order[m])
        hit = best >= 0
        images[host].reshape(-1, 3)[hit] = sq[best[hit]]
    sel = painted(W, frame_mask)
    return {"bgr": np.stack([images[f] for f in sel]), "frames": sel, "n_points": n, "n_residuals": int(live.sum()), "n_pattern_pixels": int(ok.sum())}
