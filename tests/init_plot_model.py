"""Host models of CoarseInitializer::debugPlot (CoarseInitializer.cpp:287-335) with setPixel9 (MinimalImage.h), for nalo_init_depth_image.

Inputs: I (w * h irradiance of the first frame at the level) and the level's u, v, iR, isGood. literal(): the reference's three loops one to one - the base image,
the scale, the squares in ascending index with a setPixel9 that clips -; np.float32 scalars carry the float arithmetic. fast(): the same result vectorised (the
last writer as the maximum index over the nine offsets), for full-size levels. Both use the conversions the library DEFINES where the reference is undefined
(include/nalo_gpu.h): float -> unsigned char of the base is (unsigned char)(saturating int, NaN -> 0), pixels of a block outside the image are skipped,
(int)(u + 0.5f) saturates with NaN -> 0, an id int cannot hold paints white.

Both return a dict with the keys of Context.init_depth_image: bgr (h, w, 3) uint8, n_points, n_good, sum_iR, fac (float32)."""
import numpy as np

from window_plot_model import BLACK, F, _rainbow_vec, _to_int_vec, centre, rainbow, to_int

SQUARE = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def base_byte(I):
    """`Vec3b(I, I, I)` from a float: (unsigned char)(int)I"""
    return to_int(I) & 0xFF


def scale(iR, isGood):
    """:306-316: (n_good, sid, fac) - the chain of dependent float adds in index order"""
    nid, sid = F(0), F(0)
    with np.errstate(all="ignore"):
        for i in range(len(iR)):
            if isGood[i]:
                nid = F(nid + F(1))
                sid = F(sid + F(iR[i]))
        fac = F(nid / sid)
    return int(nid), sid, fac


def scale_fast(iR, isGood):
    g = np.asarray(iR, F)[np.asarray(isGood) != 0]
    with np.errstate(all="ignore"):
        sid = np.cumsum(g, dtype=F)[-1] if g.size else F(0)                   # cumsum is the sequential chain
        fac = F(F(g.size) / sid)
    return int(g.size), F(sid), fac


def set_pixel9(img, u, v, val):
    """MinimalImage::setPixel9; at() clips here"""
    h, w = img.shape[:2]
    for dx, dy in SQUARE:
        if 0 <= u + dx < w and 0 <= v + dy < h:
            img[v + dy, u + dx, :] = val


def literal(I, w, h, u, v, iR, isGood, rainbow_scale=1.0):
    I = np.ascontiguousarray(I, F).reshape(-1)
    img = np.zeros((h, w, 3), np.uint8)
    for i in range(w * h):
        img[i // w, i % w, :] = base_byte(I[i])
    n_good, sid, fac = scale(iR, isGood)
    with np.errstate(all="ignore"):
        for i in range(len(u)):
            if not isGood[i]:
                set_pixel9(img, centre(u[i]), centre(v[i]), BLACK)
            else:
                set_pixel9(img, centre(u[i]), centre(v[i]), rainbow(F(F(iR[i]) * fac), rainbow_scale))
    return {"bgr": img, "n_points": len(u), "n_good": n_good, "sum_iR": sid, "fac": fac}


def fast(I, w, h, u, v, iR, isGood, rainbow_scale=1.0):
    I = np.ascontiguousarray(I, F).reshape(h, w)
    img = np.repeat((_to_int_vec(I) & 0xFF).astype(np.uint8)[:, :, None], 3, axis=2)
    n_good, sid, fac = scale_fast(iR, isGood)
    n = len(u)
    if n:
        good = np.asarray(isGood) != 0
        with np.errstate(all="ignore"):
            col = _rainbow_vec((np.asarray(iR, F) * fac).astype(F), rainbow_scale)
            cu, cv = _to_int_vec(np.asarray(u, F) + F(0.5)), _to_int_vec(np.asarray(v, F) + F(0.5))
        col[~good] = 0
        order = np.arange(n, dtype=np.int64)
        best = np.full(w * h, -1, np.int64)
        for dx, dy in SQUARE:
            x, y = cu + dx, cv + dy
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            np.maximum.at(best, (y[ok] * w + x[ok]), order[ok])
        hit = best >= 0
        img.reshape(-1, 3)[hit] = col[best[hit]]
    return {"bgr": img, "n_points": n, "n_good": n_good, "sum_iR": sid, "fac": fac}


def sum_order_set(n, seed=5):
    """n values of iR whose sequential float sum is neither the fp64 sum rounded to float nor numpy's pairwise float sum: one term of 2^22 (ulp 0.5) first,
    then values in [0.5, 1.5), every add of which rounds"""
    iR = np.random.RandomState(seed).uniform(0.5, 1.5, n).astype(F)
    iR[0] = F(4194304.0)
    return iR


def same_float(a, b):
    """bit-equal, or both NaN (a NaN's sign and payload are not defined)"""
    a, b = F(a), F(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32))
