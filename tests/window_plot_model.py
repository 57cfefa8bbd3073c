"""Host models of FullSystem::debugPlot (FullSystemDebugStuff.cpp:109-358) with setPixelCirc (MinimalImage.h:112-126), makeRainbow3B and makeJet3B
(globalFuncs.h:334-367), for nalo_map_window_plot.

A window is a list of frames, each a dict: I (w * h irradiance, level 0), active / marg / out (dicts of u, v, idepth) and imm (dict of u, v, idmin, idmax, status,
quality), every list in the library's order (submission / archive / storage). literal(): the reference's loops one to one - one `for` per list, a setPixelCirc
that clips, the sort for mode 7 -; np.float32 scalars carry the float arithmetic and Python floats the double products. fast(): the same result vectorised (the
last writer as the maximum painting position over the 40 ring offsets), for full-size frames. Both use the conversions the library DEFINES where the reference is
undefined (include/nalo_gpu.h): ring pixels outside the image are skipped, (int)(u + 0.5f) saturates with NaN -> 0, an id int cannot hold paints white, the bytes of
mode 5 saturate with NaN -> 0, NaNs are left out of allID and -0 orders before +0.

Both return None when mode 7 finds an empty allID (the reference indexes an empty vector), else a dict with the keys of Context.map_window_plot plus `frames`, the
window indices of the painted frames. Mode 6 is not modelled (the library refuses it)."""
import numpy as np

from depth_image_model import _jet_vec, grey_byte, jet, ranks

F = np.float32
GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)               # ImmaturePointStatus (ImmaturePoint.h:47-53)
WHITE, BLACK = (255, 255, 255), (0, 0, 0)
STATUS_COLOUR = {GOOD: (0, 255, 0), OOB: (255, 0, 0), OUTLIER: (0, 0, 255), SKIPPED: (255, 255, 0), BADCONDITION: WHITE, UNINITIALIZED: BLACK}   # :245-256
# the 40 offsets setPixelCirc writes: Chebyshev distance 2 or 3
RING = [(dx, dy) for dy in range(-3, 4) for dx in range(-3, 4) if max(abs(dx), abs(dy)) >= 2]
assert len(RING) == 40
EMPTY = dict(u=np.zeros(0, F), v=np.zeros(0, F), idepth=np.zeros(0, F))
NO_IMM = dict(u=np.zeros(0, F), v=np.zeros(0, F), idmin=np.zeros(0, F), idmax=np.zeros(0, F), status=np.zeros(0, np.int32), quality=np.zeros(0, F))


def to_int(x):
    """float -> int: truncation toward zero, saturating, NaN -> 0"""
    x = F(x)
    if np.isnan(x):
        return 0
    if x >= F(2147483648.0):
        return 2147483647
    if x <= F(-2147483648.0):
        return -2147483648
    return int(x)


def centre(u):
    """the `const int&` argument of setPixelCirc(ph->u+0.5f, ...)"""
    with np.errstate(all="ignore"):
        return to_int(F(u) + F(0.5))


def color_byte(x):
    """float -> byte of a colour: truncation toward zero, saturated to 0..255, NaN -> 0"""
    x = F(x)
    if not x > 0:
        return 0
    return 255 if x >= 255 else int(x)


def rainbow(id_, scale=1.0):
    """makeRainbow3B as written, freeDebugParam3 = scale; an id int cannot hold -> white"""
    with np.errstate(all="ignore"):
        id_ = F(F(id_) * F(scale))
    if not id_ > 0:
        return WHITE
    if id_ >= F(2147483648.0):
        return WHITE
    icP = int(id_)
    ifP = F(id_ - F(icP))
    icP %= 3
    a, b = int(F(255) * F(F(1) - ifP)), int(F(255) * ifP)
    if icP == 0:
        return (a, b, 0)
    if icP == 1:
        return (0, a, b)
    return (b, 0, a)


def order_key(x):
    """the float's bits as an unsigned that orders like the float, -0 before +0"""
    u = int(np.asarray(x, F).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def smooth(min_new, max_new, minmax):
    """:139-156. minmax None = no smoothing. Returns (minID, maxID, rewritten pair or None)"""
    minID, maxID = F(min_new), F(max_new)
    if minmax is None:
        return minID, maxID, None
    mn, mx = F(minmax[0]), F(minmax[1])
    with np.errstate(all="ignore"):
        maxChange = F(0.1 * float(F(mx - mn)))
        if mx < 0 or mn < 0:
            maxChange = F(1e5)
        if minID < F(mn - maxChange):
            minID = F(mn - maxChange)
        if minID > F(mn + maxChange):
            minID = F(mn + maxChange)
        if maxID < F(mx - maxChange):
            maxID = F(mx - maxChange)
        if maxID > F(mx + maxChange):
            maxID = F(mx + maxChange)
    return minID, maxID, np.array([minID, maxID], F)


def select(values, minmax):
    """:121-136 on allID = values (NaNs left out). None when it is empty"""
    allID = [F(x) for x in np.asarray(values, F).reshape(-1) if not np.isnan(x)]
    if not allID:
        return None
    allID.sort(key=order_key)
    r0, r1 = ranks(len(allID))
    minID, maxID, pair = smooth(allID[r0], allID[r1], minmax)
    return {"n_values": len(allID), "min_new": F(allID[r0]), "max_new": F(allID[r1]), "min_used": minID, "max_used": maxID, "minmax": pair}


def select_fast(values, minmax):
    v = np.asarray(values, F).reshape(-1)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return None
    u = v.view(np.uint32)
    v = v[np.argsort(np.where(u & 0x80000000, ~u, u | 0x80000000), kind="stable")]
    r0, r1 = ranks(v.size)
    minID, maxID, pair = smooth(v[r0], v[r1], minmax)
    return {"n_values": int(v.size), "min_new": F(v[r0]), "max_new": F(v[r1]), "min_used": minID, "max_used": maxID, "minmax": pair}


def all_id(frames):
    parts = [np.asarray(f.get(k, EMPTY)["idepth"], F) for f in frames for k in ("active", "marg", "out")]
    return np.concatenate(parts) if parts else np.zeros(0, F)


def set_pixel_circ(img, u, v, val):
    """MinimalImage::setPixelCirc; at() clips here"""
    h, w = img.shape[:2]

    def at(x, y):
        if 0 <= x < w and 0 <= y < h:
            img[y, x, :] = val
    for i in range(-3, 4):
        at(u + 3, v + i); at(u - 3, v + i); at(u + 2, v + i); at(u - 2, v + i)
        at(u + i, v - 3); at(u + i, v + 3); at(u + i, v - 2); at(u + i, v + 2)


def mode5_colour(quality, scale):
    with np.errstate(all="ignore"):
        d = F(F(scale) * F(np.sqrt(F(quality)) - F(1)))
        if d < 0:
            d = F(0)
        if d > 1:
            d = F(1)
        return (0, color_byte(F(d * F(255))), color_byte(F(F(F(1) - d) * F(255))))


def painted(n_frames, frame_mask):
    return [i for i in range(n_frames) if not frame_mask or (frame_mask >> i) & 1]


def literal(frames, w, h, mode, frame_mask=0, minmax=None, rainbow_scale=1.0, quality_scale=1.0):
    out = {"n_values": 0, "min_new": F(0), "max_new": F(0), "min_used": F(0), "max_used": F(0), "minmax": None if minmax is None else np.array(minmax, F)}
    minID = maxID = F(0)
    if mode == 7:
        out = select(all_id(frames), minmax)
        if out is None:
            return None
        minID, maxID = out["min_used"], out["max_used"]
    sel = painted(len(frames), frame_mask)
    images, sources = [], []
    for fi in sel:
        f = frames[fi]
        I = np.ascontiguousarray(f["I"], F).reshape(-1)
        img = np.zeros((h, w, 3), np.uint8)
        for i in range(w * h):
            img[i // w, i % w, :] = grey_byte(I[i])
        act, marg, outp, imm = f.get("active", EMPTY), f.get("marg", EMPTY), f.get("out", EMPTY), f.get("imm", NO_IMM)
        n = [0, 0, 0, 0]

        def ring(ph, k, col, cls):
            set_pixel_circ(img, centre(ph["u"][k]), centre(ph["v"][k]), col)
            n[cls] += 1
        if mode == 0:
            for k in range(len(act["u"])):
                ring(act, k, rainbow(act["idepth"][k], rainbow_scale), 1)
            for k in range(len(marg["u"])):
                ring(marg, k, rainbow(marg["idepth"][k], rainbow_scale), 2)
            for k in range(len(outp["u"])):
                ring(outp, k, WHITE, 3)
        elif mode == 1:
            for k in range(len(act["u"])):
                ring(act, k, rainbow(act["idepth"][k], rainbow_scale), 1)
            for k in range(len(marg["u"])):
                ring(marg, k, BLACK, 2)
            for k in range(len(outp["u"])):
                ring(outp, k, WHITE, 3)
        elif mode == 3:
            for k in range(len(imm["u"])):
                if imm["status"][k] in (GOOD, SKIPPED, BADCONDITION):
                    if not np.isfinite(imm["idmax"][k]):
                        ring(imm, k, BLACK, 0)
                    else:
                        with np.errstate(all="ignore"):
                            ring(imm, k, rainbow(F(F(imm["idmin"][k] + imm["idmax"][k]) * F(0.5)), rainbow_scale), 0)
        elif mode == 4:
            for k in range(len(imm["u"])):
                if int(imm["status"][k]) in STATUS_COLOUR:
                    ring(imm, k, STATUS_COLOUR[int(imm["status"][k])], 0)
        elif mode == 5:
            for k in range(len(imm["u"])):
                if imm["status"][k] == UNINITIALIZED:
                    continue
                ring(imm, k, mode5_colour(imm["quality"][k], quality_scale), 0)
        if mode == 7:
            with np.errstate(all="ignore"):
                for k in range(len(act["u"])):
                    ring(act, k, jet(F(F(act["idepth"][k] - minID) / F(maxID - minID))), 1)
            for k in range(len(marg["u"])):
                ring(marg, k, BLACK, 2)
        images.append(img)
        sources.append(n)
    out["bgr"] = np.stack(images) if images else np.zeros((0, h, w, 3), np.uint8)
    out["sources"] = np.array(sources, np.int32).reshape(len(sel), 4)
    out["frames"] = sel
    return out


# ------------------------------------------------------------------------------------------------ the vectorised form
def _to_int_vec(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x), 0.0, np.clip(x.astype(np.float64), -2147483648.0, 2147483647.0)).astype(np.int64)


def _byte_vec(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return np.where(x > 0, np.minimum(np.where(np.isnan(x), 0, x), 255), 0).astype(np.int64)


def _rainbow_vec(id_, scale):
    with np.errstate(all="ignore"):
        id_ = (np.asarray(id_, F) * F(scale)).astype(F)
        ok = (id_ > 0) & (id_ < F(2147483648.0))
        icP = np.where(ok, id_, 0).astype(np.int64)
        ifP = (np.where(ok, id_, 0).astype(F) - icP.astype(F)).astype(F)
        a = (F(255) * (F(1) - ifP).astype(F)).astype(F).astype(np.int64)
        b = (F(255) * ifP).astype(F).astype(np.int64)
    z = np.zeros_like(a)
    br = icP % 3
    out = np.where((br == 0)[:, None], np.stack([a, b, z], 1), np.where((br == 1)[:, None], np.stack([z, a, b], 1), np.stack([b, z, a], 1)))
    out[~ok] = 255
    return out.astype(np.uint8)


def _const(n, col):
    return np.tile(np.array(col, np.uint8), (n, 1))


def _frame_sources(f, mode, minID, maxID, rainbow_scale, quality_scale):
    """(u, v, colour [n][3], class) of the frame's drawn sources in painting order"""
    act, marg, outp, imm = f.get("active", EMPTY), f.get("marg", EMPTY), f.get("out", EMPTY), f.get("imm", NO_IMM)
    parts = []
    if mode in (0, 1):
        parts.append((act["u"], act["v"], _rainbow_vec(act["idepth"], rainbow_scale), 1))
        parts.append((marg["u"], marg["v"], _rainbow_vec(marg["idepth"], rainbow_scale) if mode == 0 else _const(len(marg["u"]), BLACK), 2))
        parts.append((outp["u"], outp["v"], _const(len(outp["u"]), WHITE), 3))
    elif mode == 7:
        with np.errstate(all="ignore"):
            idn = ((np.asarray(act["idepth"], F) - minID).astype(F) / F(maxID - minID)).astype(F)
        parts.append((act["u"], act["v"], _jet_vec(idn).reshape(-1, 3), 1))
        parts.append((marg["u"], marg["v"], _const(len(marg["u"]), BLACK), 2))
    elif mode in (3, 4, 5):
        st = np.asarray(imm["status"])
        u, v = np.asarray(imm["u"], F), np.asarray(imm["v"], F)
        if mode == 3:
            keep = np.isin(st, (GOOD, SKIPPED, BADCONDITION))
            with np.errstate(all="ignore"):
                col = _rainbow_vec(((np.asarray(imm["idmin"], F) + np.asarray(imm["idmax"], F)).astype(F) * F(0.5)).astype(F), rainbow_scale)
            col[~np.isfinite(np.asarray(imm["idmax"], F))] = 0
        elif mode == 4:
            keep = np.isin(st, list(STATUS_COLOUR))
            col = np.zeros((len(st), 3), np.uint8)
            for s, c in STATUS_COLOUR.items():
                col[st == s] = c
        else:
            keep = st != UNINITIALIZED
            with np.errstate(all="ignore"):
                d = (F(quality_scale) * (np.sqrt(np.asarray(imm["quality"], F)) - F(1)).astype(F)).astype(F)
                d = np.where(d < 0, F(0), d)
                d = np.where(d > 1, F(1), d).astype(F)
                col = np.stack([np.zeros(len(st), np.int64), _byte_vec((d * F(255)).astype(F)), _byte_vec(((F(1) - d).astype(F) * F(255)).astype(F))], 1).astype(np.uint8)
        parts.append((u[keep], v[keep], col[keep], 0))
    return parts


def fast(frames, w, h, mode, frame_mask=0, minmax=None, rainbow_scale=1.0, quality_scale=1.0):
    out = {"n_values": 0, "min_new": F(0), "max_new": F(0), "min_used": F(0), "max_used": F(0), "minmax": None if minmax is None else np.array(minmax, F)}
    minID = maxID = F(0)
    if mode == 7:
        out = select_fast(all_id(frames), minmax)
        if out is None:
            return None
        minID, maxID = out["min_used"], out["max_used"]
    sel = painted(len(frames), frame_mask)
    images, sources = [], []
    for fi in sel:
        f = frames[fi]
        I = np.ascontiguousarray(f["I"], F).reshape(h, w)
        with np.errstate(all="ignore"):
            c = np.minimum(_to_int_vec((I * F(0.9)).astype(F)), 255)
        img = np.repeat((c & 0xFF).astype(np.uint8)[:, :, None], 3, axis=2)
        parts = _frame_sources(f, mode, minID, maxID, rainbow_scale, quality_scale)
        n = [0, 0, 0, 0]
        for p in parts:
            n[p[3]] += len(p[0])
        if parts and sum(len(p[0]) for p in parts):
            with np.errstate(all="ignore"):
                cu = np.concatenate([_to_int_vec(np.asarray(p[0], F) + F(0.5)) for p in parts])
                cv = np.concatenate([_to_int_vec(np.asarray(p[1], F) + F(0.5)) for p in parts])
            col = np.concatenate([p[2].reshape(-1, 3) for p in parts])
            order = np.arange(len(cu), dtype=np.int64)
            best = np.full(w * h, -1, np.int64)
            for dx, dy in RING:
                x, y = cu + dx, cv + dy
                ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
                np.maximum.at(best, (y[ok] * w + x[ok]), order[ok])
            hit = best >= 0
            img.reshape(-1, 3)[hit] = col[best[hit]]
        images.append(img)
        sources.append(n)
    out["bgr"] = np.stack(images) if images else np.zeros((0, h, w, 3), np.uint8)
    out["sources"] = np.array(sources, np.int32).reshape(len(sel), 4)
    out["frames"] = sel
    return out
