"""The literal model of activatePointsMT's selection loop (reference FullSystem.cpp:805-876) that tests/test_imm_activate_gpu.py compares the device against.

It is the loop as written: the hosts in window order with the newest frame skipped, every point against the CURRENT distance map, and after every accepted
point addIntoDistFinal = the pixel set to 0 and one growDistBFS(1) on that map (CoarseTracker.cpp:1458-1561: 39 levels, odd levels over 8 neighbours, even
levels over 4, border pixels never expand, a neighbour is taken when its value is above the level). Arithmetic is np.float32, one rounding per operation, in
the order the reference writes it. Nothing here knows that the map is a minimum over seeds or that a decision is local: that is what the kernels rest on and
what this model is there to check. The map lives in a flat Python list (item access on a numpy array costs several times more)."""
import numpy as np

GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
MIN_TRACE_QUALITY = np.float32(3)                                              # setting_minTraceQuality (settings.cpp:166)
N4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
N8 = N4 + ((1, 1), (-1, 1), (-1, -1), (1, -1))
f32 = np.float32


def add_into_dist_final(D, w1, h1, u, v):
    """CoarseDistanceMap::addIntoDistFinal on the flat list D"""
    D[u + w1 * v] = 0
    cur = [(u, v)]
    for k in range(1, 40):
        nxt = []
        for x, y in cur:
            if x == 0 or y == 0 or x == w1 - 1 or y == h1 - 1:
                continue
            for dx, dy in (N4 if k % 2 == 0 else N8):
                j = (x + dx) + (y + dy) * w1
                if D[j] > k:
                    D[j] = k
                    nxt.append((x + dx, y + dy))
        cur = nxt
        if not cur:
            break                                                              # the reference goes on with empty lists: nothing more happens


def project(KRKi, Kt, host, u, v, idmin, idmax):
    """:855-857 -> ptp0, U, V, inside-the-int-range flag (a quotient that is NaN or outside int is outside the image)"""
    M, T = KRKi.astype(f32).reshape(-1, 3, 3)[host], Kt.astype(f32).reshape(-1, 3)[host]
    u, v = u.astype(f32), v.astype(f32)
    with np.errstate(all="ignore"):
        z = f32(0.5) * (idmax.astype(f32) + idmin.astype(f32))
        ptp = [((M[:, k, 0] * u + M[:, k, 1] * v) + M[:, k, 2] * f32(1)) + T[:, k] * z for k in range(3)]
        qu, qv = ptp[0] / ptp[2] + f32(0.5), ptp[1] / ptp[2] + f32(0.5)
        ok = np.isfinite(qu) & np.isfinite(qv) & (np.abs(qu) < 2.0 ** 31) & (np.abs(qv) < 2.0 ** 31)
        U = np.where(ok, np.trunc(np.where(ok, qu, 0)), -1).astype(np.int64)
        V = np.where(ok, np.trunc(np.where(ok, qv, 0)), -1).astype(np.int64)
        frac = ptp[0] - np.floor(ptp[0])
    return frac.astype(f32), U, V


def select(D0, frame, host, u, v, idmin, idmax, status, quality, interval, my_type, KRKi, Kt, flagged, min_act_dist):
    """-> fate [n] (the codes of nalo_imm_resident_activate), sel (toOptimize's order), info dict (survivors of the test on D0, rejected although they
    passed it, the largest number of survivors on one pixel)"""
    h1, w1 = D0.shape
    n = len(host)
    D = [float(x) for x in D0.reshape(-1)]
    D0f = D0.reshape(-1)
    frac, U, V = project(KRKi, Kt, host, u, v, idmin, idmax)
    with np.errstate(all="ignore"):
        th = f32(min_act_dist) * my_type.astype(f32)
        ssum = idmax.astype(f32) + idmin.astype(f32)
    fate = np.zeros(n, np.int32)
    sel = []
    survivors = late = 0
    per_pixel = {}
    for h in range(len(flagged)):
        if h == frame:
            fate[host == h] = 3
            continue
        for i in np.nonzero(host == h)[0]:
            if not np.isfinite(idmax[i]) or status[i] == OUTLIER:
                fate[i] = -1
                continue
            can = status[i] in (GOOD, SKIPPED, BADCONDITION, OOB) and interval[i] < 8 and quality[i] > MIN_TRACE_QUALITY and ssum[i] > 0
            if not can:
                fate[i] = -2 if (flagged[h] or status[i] == OOB) else 0
                continue
            x, y = int(U[i]), int(V[i])
            if not (x > 0 and y > 0 and x < w1 and y < h1):
                fate[i] = -3
                continue
            p = x + w1 * y
            if f32(D0f[p]) + frac[i] >= th[i]:
                survivors += 1
                per_pixel[p] = per_pixel.get(p, 0) + 1
                if not (f32(D[p]) + frac[i] >= th[i]):
                    late += 1
            if f32(D[p]) + frac[i] >= th[i]:
                add_into_dist_final(D, w1, h1, x, y)
                sel.append(i)
                fate[i] = 1
            else:
                fate[i] = 2
    return fate, np.asarray(sel, np.int32), dict(survivors=survivors, late=late, max_per_pixel=max(per_pixel.values()) if per_pixel else 0,
                                                 D=np.asarray(D, np.float32).reshape(h1, w1))
