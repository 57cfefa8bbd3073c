"""Host models of CoarseTracker::debugPlotIDepthMap (CoarseTracker.cpp:1263-1359) with setPixelCirc (MinimalImage.h:112-126) and makeJet3B
(globalFuncs.h:350-367), for nalo_trk_depth_image.

literal(): the reference's loops one to one, the sequential setPixelCirc scatter in raster order included; np.float32 scalars carry the float arithmetic and
Python floats the double products. fast(): the same result vectorised (quantiles from np.sort, the last writer as the maximum raster index over the 40 ring
offsets), for full-size frames. Both use the three conversions the library DEFINES where the reference is undefined (include/nalo_gpu.h): float -> int of the
grey value saturates with NaN -> 0, a negative grey value wraps as int -> unsigned char does, a NaN id paints white.

Both return None when the map holds no positive value (the reference indexes an empty vector), else a dict with the keys of Context.trk_depth_image."""
import numpy as np

F = np.float32
# the 40 offsets setPixelCirc writes: Chebyshev distance 2 or 3
RING = [(dx, dy) for dy in range(-3, 4) for dx in range(-3, 4) if max(abs(dx), abs(dy)) >= 2]
assert len(RING) == 40


def ranks(size):
    """the two indices into the sorted allID: `int n = allID.size()-1; (int)(n*0.05), (int)(n*0.95)`"""
    n = size - 1
    return int(n * 0.05), int(n * 0.95)


def smooth(min_new, max_new, minmax):
    """:1283-1313. minmax None = NULL pointers. Returns (minID, maxID, rewritten pair or None)"""
    minID, maxID = F(min_new), F(max_new)
    if minmax is None:
        return minID, maxID, None
    mn, mx = F(minmax[0]), F(minmax[1])
    with np.errstate(all="ignore"):
        if mn < 0 or mx < 0:
            mx, mn = maxID, minID
        else:
            maxChange = F(0.3 * float(F(mx - mn)))
            if minID < F(mn - maxChange):
                minID = F(mn - maxChange)
            if minID > F(mn + maxChange):
                minID = F(mn + maxChange)
            if maxID < F(mx - maxChange):
                maxID = F(mx - maxChange)
            if maxID > F(mx + maxChange):
                maxID = F(mx + maxChange)
            mx, mn = maxID, minID
    return minID, maxID, np.array([mn, mx], F)


def grey_byte(v):
    """`int c = I*0.9f; if(c>255) c=255; (unsigned char)c` with the saturating, NaN -> 0 conversion"""
    with np.errstate(all="ignore"):
        p = F(v) * F(0.9)
    if np.isnan(p):
        c = 0
    elif p >= F(2147483648.0):
        c = 2147483647
    elif p <= F(-2147483648.0):
        c = -2147483648
    else:
        c = int(p)
    if c > 255:
        c = 255
    return c & 0xFF


def jet(id_):
    """makeJet3B as written; NaN -> white"""
    id_ = F(id_)
    if id_ <= 0:
        return (128, 0, 0)
    if id_ >= 1:
        return (0, 0, 128)
    if np.isnan(id_):
        return (255, 255, 255)
    id8 = F(id_ * F(8))
    icP = int(id8)
    ifP = float(F(id8 - F(icP)))
    if icP == 0:
        return (int(255 * (0.5 + 0.5 * ifP)), 0, 0)
    if icP == 1:
        return (255, int(255 * (0.5 * ifP)), 0)
    if icP == 2:
        return (255, int(255 * (0.5 + 0.5 * ifP)), 0)
    if icP == 3:
        return (int(255 * (1 - 0.5 * ifP)), 255, int(255 * (0.5 * ifP)))
    if icP == 4:
        return (int(255 * (0.5 - 0.5 * ifP)), 255, int(255 * (0.5 + 0.5 * ifP)))
    if icP == 5:
        return (0, int(255 * (1 - 0.5 * ifP)), 255)
    if icP == 6:
        return (0, int(255 * (0.5 - 0.5 * ifP)), 255)
    if icP == 7:
        return (0, 0, int(255 * (1 - 0.5 * ifP)))
    return (255, 255, 255)


def _select(idepth, minmax):
    idepth = np.ascontiguousarray(idepth, F).reshape(-1)
    allID = np.sort(idepth[idepth > 0])
    if allID.size == 0:
        return None
    r0, r1 = ranks(allID.size)
    min_new, max_new = allID[r0], allID[r1]
    minID, maxID, pair = smooth(min_new, max_new, minmax)
    return {"n_positive": int(allID.size), "min_new": F(min_new), "max_new": F(max_new), "min_used": minID, "max_used": maxID, "minmax": pair}


def literal(idepth, I, w, h, minmax=None):
    out = _select(idepth, minmax)
    if out is None:
        return None
    idepth = np.ascontiguousarray(idepth, F).reshape(-1)
    I = np.ascontiguousarray(I, F).reshape(-1)
    minID, maxID = out["min_used"], out["max_used"]
    mf = np.zeros((h, w, 3), np.uint8)
    for i in range(w * h):
        mf[i // w, i % w, :] = grey_byte(I[i])
    with np.errstate(all="ignore"):
        for y in range(3, h - 3):
            for x in range(3, w - 3):
                idx = x + y * w
                sid, nid = F(0), F(0)
                for o in (0, 1, -1, w, -w):
                    if idepth[idx + o] > 0:
                        sid = F(sid + idepth[idx + o])
                        nid = F(nid + F(1))
                if idepth[idx] > 0 or nid >= 3:
                    col = jet(F(F(F(sid / nid) - minID) / F(maxID - minID)))
                    for i in range(-3, 4):                                    # setPixelCirc, in its own order
                        for (u, v) in ((x + 3, y + i), (x - 3, y + i), (x + 2, y + i), (x - 2, y + i), (x + i, y - 3), (x + i, y + 3), (x + i, y - 2), (x + i, y + 2)):
                            mf[v, u, :] = col
    out["bgr"] = mf
    return out


def _jet_vec(id_):
    id_ = np.asarray(id_, F)
    out = np.full((id_.size, 3), 255, np.int64)
    with np.errstate(all="ignore"):
        id8 = (id_ * F(8)).astype(F)
        mid = (id_ > 0) & (id_ < 1)
        icP = np.where(mid, id8, 0).astype(np.int64)
        ifP = (id8 - icP.astype(F)).astype(F).astype(np.float64)
    z, f = np.zeros(id_.size, np.int64), np.full(id_.size, 255, np.int64)

    def t(v):
        return np.where(mid, v, 0).astype(np.int64)
    table = {0: (t(255 * (0.5 + 0.5 * ifP)), z, z), 1: (f, t(255 * (0.5 * ifP)), z), 2: (f, t(255 * (0.5 + 0.5 * ifP)), z),
             3: (t(255 * (1 - 0.5 * ifP)), f, t(255 * (0.5 * ifP))), 4: (t(255 * (0.5 - 0.5 * ifP)), f, t(255 * (0.5 + 0.5 * ifP))),
             5: (z, t(255 * (1 - 0.5 * ifP)), f), 6: (z, t(255 * (0.5 - 0.5 * ifP)), f), 7: (z, z, t(255 * (1 - 0.5 * ifP)))}
    for k, cols in table.items():
        m = mid & (icP == k)
        for ch in range(3):
            out[m, ch] = cols[ch][m]
    out[id_ <= 0] = (128, 0, 0)
    out[id_ >= 1] = (0, 0, 128)
    return out.astype(np.uint8)


def fast(idepth, I, w, h, minmax=None):
    out = _select(idepth, minmax)
    if out is None:
        return None
    d = np.ascontiguousarray(idepth, F).reshape(h, w)
    I = np.ascontiguousarray(I, F).reshape(h, w)
    minID, maxID = out["min_used"], out["max_used"]
    with np.errstate(all="ignore"):
        p = (I * F(0.9)).astype(F)
        c = np.where(np.isnan(p), 0.0, np.clip(p.astype(np.float64), -2147483648.0, 2147483647.0)).astype(np.int64)   # trunc toward zero, saturating
        c = np.minimum(c, 255)
        grey = (c & 0xFF).astype(np.uint8)
        # the five taps of the sources in [3, w-3) x [3, h-3), added in the reference's order
        ys, xs = slice(3, h - 3), slice(3, w - 3)
        taps = [d[ys, xs], d[ys, 4:w - 2], d[ys, 2:w - 4], d[4:h - 2, xs], d[2:h - 4, xs]]
        sid = np.zeros(taps[0].shape, F)
        nid = np.zeros(taps[0].shape, F)
        for tp in taps:
            pos = tp > 0
            sid = np.where(pos, (sid + tp).astype(F), sid)
            nid = np.where(pos, nid + F(1), nid)
        plot = (taps[0] > 0) | (nid >= 3)
        idn = (((sid / nid).astype(F) - minID).astype(F) / F(maxID - minID)).astype(F)
    ridx = np.full((h + 6, w + 6), -1, np.int64)                                 # raster index of each plotting source, padded by the ring's reach
    yy, xx = np.nonzero(plot)
    ridx[yy + 6, xx + 6] = (yy + 3) * w + (xx + 3)
    colour = np.zeros((w * h, 3), np.uint8)
    colour[(yy + 3) * w + (xx + 3)] = _jet_vec(idn[yy, xx])
    best = np.full((h, w), -1, np.int64)
    for dx, dy in RING:                                                          # output q is written by the sources q - d
        np.maximum(best, ridx[3 - dy:3 - dy + h, 3 - dx:3 - dx + w], out=best)
    mf = np.repeat(grey[:, :, None], 3, axis=2)
    hit = best >= 0
    mf[hit] = colour[best[hit]]
    out["bgr"] = mf
    return out
