"""Literal model of nalo_dense_update_map and of the two consumers of the dense archive (include/nalo_gpu.h).

update_map() is the loop of DenseMapping::updateMap (reference src/FullSystem/MapPoint.cpp:271-331) over tests/plane_model.py's clusters: per cluster the
oracle's orc_dense_bbox (the mask scan of :300-310) and orc_dense_make_map (makeMap, :334-407), the kept points appended under the accept bit.
refresh_pc() is KeyFrameDisplay::refreshPC() (IOWrapper/Pangolin/KeyFrameDisplay.cpp:212-271) and world_points() the tsdf=1 loop of SampleOutputWrapper
(IOWrapper/OutputWrapper/SampleOutputWrapper.h:152-176) as plain Python loops with numpy.float32 scalars; refresh_pc_fast() is the vectorised form the GPU
tests use on large frames, held equal to the literal one in test_dense_map_cpu.py."""
import numpy as np

import orc
import plane_model as pm

F = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
RAND_MAX = 2147483647


def make_map(mask, img, bgr, w, h, K, plane, value, rect, c2w):
    """orc_dense_make_map for one cluster -> dict(n, accept, u, v, idepth, color, bgr)"""
    O = orc.lib()
    cap = max((w - 4) * (h - 4), 1)
    dI, _ = orc.make_images(np.ascontiguousarray(img, F), 1)
    pu, pv = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    pid, pc, pb = np.zeros(cap, F), np.zeros(cap, F), np.zeros((cap, 3), np.uint8)
    acc = np.zeros(1, np.int32)
    rect = np.ascontiguousarray(rect, np.int32)
    n = 0
    if rect[0] < 2 ** 30:                         # an empty scan leaves INT_MAX / INT_MIN: the loops run over nothing
        n = O.orc_dense_make_map(orc.fp(np.ascontiguousarray(mask, F)), orc.fp(dI), orc.u8p(np.ascontiguousarray(bgr, np.uint8)), w, h,
                                 orc.fp(np.ascontiguousarray(plane, F)), float(value), orc.ip(rect), float(F(1) / F(K[0])), float(F(1) / F(K[1])), float(F(K[2])), float(F(K[3])),
                                 orc.dp(np.ascontiguousarray(c2w, np.float64).reshape(-1)), orc.ip(pu), orc.ip(pv), orc.fp(pid), orc.fp(pc), orc.u8p(pb), orc.ip(acc))
    return dict(n=int(n), accept=int(acc[0]) if n else 0, u=pu[:n].copy(), v=pv[:n].copy(), idepth=pid[:n].copy(), color=pc[:n].copy(), bgr=pb[:n].copy())


def bbox(mask, w, h, value):
    r = np.zeros(4, np.int32)
    orc.lib().orc_dense_bbox(orc.fp(np.ascontiguousarray(mask, F)), w, h, float(value), orc.ip(r))
    return [int(x) for x in r]


def update_map(u, v, idp, mask, img, bgr, w, h, K, draws, c2w, threshold=0.01, min_points=10, planes=None, fast=False):
    """-> dict(clusters: plane_model.fit_planes' list, runs: per cluster dict(rect, n, accept, first, u, v, idepth, color, bgr), points: what was appended, in
    order, as dict of arrays). planes: [C][4] to run makeMap with instead of the model's own fits (the fit has its own tests and its own bound)."""
    clusters = pm.fit_planes(u, v, idp, mask, w, h, K, draws, threshold=threshold, min_points=min_points, fast=fast)
    runs, app = [], []
    total = 0
    for k, c in enumerate(clusters):
        r = dict(rect=[0, 0, 0, 0], n=0, accept=0, first=-1)
        runs.append(r)
        if not c["fitted"]:                       # `continue` (:280-281)
            continue
        r["rect"] = bbox(mask, w, h, c["mask_value"])
        if c["mask_value"] == 0:                  # `if(pcolor==0) return;` (:355-357)
            continue
        plane = c["plane"] if planes is None else planes[k]
        m = make_map(mask, img, bgr, w, h, K, plane, c["mask_value"], r["rect"], c2w)
        r.update(n=m["n"], accept=m["accept"], pts=m)
        if m["accept"] and m["n"] > 0:            # fh->mapPoints.insert(...)
            r["first"] = total
            total += m["n"]
            app.append(m)
    cat = lambda key, dt, tail=(): np.concatenate([a[key] for a in app]) if app else np.zeros((0,) + tail, dt)
    points = dict(u=cat("u", np.int32), v=cat("v", np.int32), idepth=cat("idepth", F), color=cat("color", F), bgr=cat("bgr", np.uint8, (3,)))
    return dict(clusters=clusters, runs=runs, points=points)


def refresh_pc(u, v, idepth, bgr, ci, draws=None):
    """refreshPC(): -> (xyz float32 [n][3], rgb uint8 [n][3]). ci = (fxi, fyi, cxi, cyi); draws: the rand() stream, one value per SURVIVOR (None: z = depth)."""
    fxi, fyi, cxi, cyi = [F(x) for x in ci]
    xyz, rgb = [], []
    j = 0
    with np.errstate(all="ignore"):
        for i in range(len(u)):
            idp = F(idepth[i])
            if idp < 0:                           # a NaN compares false: the point stays
                continue
            depth = F(1.0) / idp
            x = (F(u[i]) * fxi + cxi) * depth
            y = (F(v[i]) * fyi + cyi) * depth
            if draws is None:
                z = depth
            else:
                r = F(F(int(draws[j])) / F(RAND_MAX)) - F(0.5)
                z = depth * (F(1) + F(2) * fxi * r)
            xyz.append([x, y, z])
            rgb.append([bgr[i][2], bgr[i][1], bgr[i][0]])
            j += 1
    return np.array(xyz, F).reshape(-1, 3), np.array(rgb, np.uint8).reshape(-1, 3)


def refresh_pc_fast(u, v, idepth, bgr, ci, draws=None):
    fxi, fyi, cxi, cyi = [F(x) for x in ci]
    idepth = np.asarray(idepth, F)
    with np.errstate(all="ignore"):
        keep = ~(idepth < 0)
        depth = (F(1.0) / idepth[keep]).astype(F)
        x = ((np.asarray(u)[keep].astype(F) * fxi + cxi) * depth).astype(F)
        y = ((np.asarray(v)[keep].astype(F) * fyi + cyi) * depth).astype(F)
        if draws is None:
            z = depth
        else:
            r = (np.asarray(draws[:len(depth)], np.int32).astype(F) / F(RAND_MAX)).astype(F) - F(0.5)
            z = (depth * (F(1) + (F(2) * fxi) * r)).astype(F)
    return np.stack([x, y, z], 1).astype(F).reshape(-1, 3), np.asarray(bgr, np.uint8).reshape(-1, 3)[keep][:, ::-1].copy()


def world_points(u, v, idepth, ci, m):
    """SampleOutputWrapper.h:152-176: float camera point, double world point. m: camToWorld 3x4."""
    fxi, fyi, cxi, cyi = [F(x) for x in ci]
    m = np.asarray(m, np.float64).reshape(3, 4)
    out = np.zeros((len(u), 3))
    with np.errstate(all="ignore"):
        for i in range(len(u)):
            depth = F(1.0) / F(idepth[i])
            x = (F(u[i]) * fxi + cxi) * depth
            y = (F(v[i]) * fyi + cyi) * depth
            z = depth * (F(1) + F(2) * fxi)
            c = [np.float64(x), np.float64(y), np.float64(z), 1.0]
            for r in range(3):
                out[i, r] = ((m[r, 0] * c[0] + m[r, 1] * c[1]) + m[r, 2] * c[2]) + m[r, 3] * c[3]
    return out
