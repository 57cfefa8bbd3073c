"""The list nalo_trk_set_ref_from_depth is DEFINED on (include/nalo_gpu.h): the passing pixels of a depth plane in raster order as the four arrays
nalo_trk_set_ref takes. inputs_literal is the header's predicate written out pixel by pixel, inputs the same in numpy; step1 restates step 1 of
makeCoarseDepthL0 (CoarseTracker.cpp:388-405) for such a list, in which no pixel is hit twice."""
import numpy as np

F = np.float32


def bits(a):
    """the words of a float32 array: equality of bits is equality bit for bit, NaN payloads and signed zeros included"""
    return np.ascontiguousarray(a, F).view(np.uint32).tobytes()


def weight_of(hdi):
    """sqrtf((float)(1e-3 / ((double)hdi + 1e-12)))"""
    return np.sqrt(F(1e-3 / (float(F(hdi)) + 1e-12)))


def inputs_literal(depth, absg, min_depth, max_depth, hdi, step=1, min_grad=0.0):
    """(Ku, Kv, new_idepth, HdiF): the double loop, v outer and u inner; depth and absg are [h][w] float32 (absg is not read with min_grad == 0)"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    mn, mx, mg = F(min_depth), F(max_depth), F(min_grad)
    Ku, Kv, nid, hd = [], [], [], []
    with np.errstate(all="ignore"):
        for v in range(h):
            for u in range(w):
                if u % step != 0 or v % step != 0:
                    continue
                D = depth[v, u]
                if not (D >= mn and D <= mx):                          # float comparisons on the values as they stand: a NaN fails both
                    continue
                if mg != F(0.0) and not (F(absg[v][u]) >= mg):
                    continue
                Ku.append(F(u)); Kv.append(F(v)); nid.append(F(1.0) / D); hd.append(F(hdi))
    return tuple(np.array(a, F) for a in (Ku, Kv, nid, hd))


def passing(depth, absg, min_depth, max_depth, step=1, min_grad=0.0):
    """the predicate as a [h][w] bool array"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    with np.errstate(invalid="ignore"):
        ok = (depth >= F(min_depth)) & (depth <= F(max_depth))
        if F(min_grad) != F(0.0):
            ok &= np.asarray(absg, F).reshape(h, w) >= F(min_grad)
    ok &= (np.arange(w) % step == 0)[None, :] & (np.arange(h) % step == 0)[:, None]
    return ok


def inputs(depth, absg, min_depth, max_depth, hdi, step=1, min_grad=0.0):
    """inputs_literal, vectorised"""
    depth = np.asarray(depth, F)
    v, u = np.nonzero(passing(depth, absg, min_depth, max_depth, step, min_grad))          # row-major: v outer, u inner
    with np.errstate(all="ignore"):
        nid = F(1.0) / depth[v, u]
    return u.astype(F), v.astype(F), nid.astype(F), np.full(len(u), F(hdi), F)


def step1(depth, absg, min_depth, max_depth, hdi, step=1, min_grad=0.0):
    """idepth[0] and weightSums[0] ([h][w]) after step 1 on the list: (1 / D) * weight and weight where the pixel passed, zeros elsewhere"""
    depth = np.asarray(depth, F)
    ok = passing(depth, absg, min_depth, max_depth, step, min_grad)
    wgt = weight_of(hdi)
    with np.errstate(all="ignore"):
        idp = np.where(ok, (F(1.0) / depth) * wgt, F(0.0)).astype(F)
    return idp, np.where(ok, wgt, F(0.0)).astype(F)
