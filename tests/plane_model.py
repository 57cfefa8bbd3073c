"""NumPy restatement of nalo_trk_fit_planes / nalo_dense_fit_planes (include/nalo_gpu.h): the clustering follows the reference's loops line by line
(DenseMapping::makeMaskDistMap, FullSystem/MapPoint.cpp:445-513), the fit is the defined algorithm of the header - float32 with the stated operation order for
the back-projection, the sample models and the scores, then `dtype` (float64, or np.longdouble to measure the float64 floor) for the refinement."""
import numpy as np

F = np.float32


def _c_int(x):
    """(int)x of a float: truncation towards zero; a value outside int's range (undefined in C) saturates as the device's conversion does, NaN gives 0."""
    x = float(x)
    if x != x:
        return 0
    return int(max(min(x, 2147483647.0), -2147483648.0))


def cluster(u, v, idepth, mask, w, h):
    """-> list of clusters, each {"mask_value", "members" (input indices, in the reference's vector order), "xx", "yy"}, in the returned order (size descending,
    ties in discovery order)."""
    mask = np.asarray(mask, F).reshape(-1)
    wait = []
    for i in range(len(u)):
        ix, iy = _c_int(u[i]), _c_int(v[i])
        # `if(dx<0.5) xx = ix; else xx = ix++;` (MapPoint.cpp:469-472): the post-increment hands back the old value, xx never rounds up
        xx, yy = ix, iy
        if xx > 2 and xx < w - 2 and yy > 2 and yy < h - 2:
            mv = mask[xx + yy * w]
            if mv != mv:           # a NaN mask value: dropped (documented difference: the reference makes it a cluster of its own)
                continue
            wait.append((i, xx, yy, mv))
    clusters = []
    while wait:
        ready, _wait = [], []
        ready.append(wait.pop())
        for idx in range(len(wait) - 1, -1, -1):
            if ready[-1][3] == wait[idx][3]:       # float equality: -0 == +0
                ready.append(wait[idx])
            else:
                _wait.append(wait[idx])
            wait.pop()
        wait = _wait
        clusters.append(ready)
    clusters.sort(key=lambda c: -len(c))           # Python's sort is stable: ties keep discovery order (the header's definition)
    return [{"mask_value": F(c[0][3]), "members": np.array([p[0] for p in c], np.int64), "xx": np.array([p[1] for p in c], np.int64),
             "yy": np.array([p[2] for p in c], np.int64)} for c in clusters]


def cluster_fast(u, v, idepth, mask, w, h):
    """cluster() for large inputs: the same result from the per-value (first index, last index, count) - an even sweep (0, 2, ...) takes the value under the last
    remaining member and lists its members in descending index, an odd one the value under the first, ascending. Held equal to cluster() in the CPU tests."""
    mask = np.asarray(mask, F).reshape(-1)
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        inside = (u >= 3) & (u < w - 2) & (v >= 3) & (v < h - 2)
    idx = np.nonzero(inside)[0]
    xx, yy = u[idx].astype(np.int64), v[idx].astype(np.int64)
    mv = mask[xx + yy * w]
    keep = mv == mv
    idx, xx, yy, mv = idx[keep], xx[keep], yy[keep], mv[keep] + F(0)          # -0 + 0 = +0
    vals, inv = np.unique(mv, return_inverse=True)
    groups = [np.nonzero(inv == k)[0] for k in range(len(vals))]               # positions in idx, ascending
    left = set(range(len(vals)))
    disc = []
    while left:
        if len(disc) % 2 == 0:
            k = max(left, key=lambda t: groups[t][-1])
        else:
            k = min(left, key=lambda t: groups[t][0])
        left.remove(k)
        g = groups[k][::-1] if len(disc) % 2 == 0 else groups[k]
        disc.append(g)
    disc.sort(key=lambda g: -len(g))
    return [{"mask_value": F(mv[g[0]]), "members": idx[g].astype(np.int64), "xx": xx[g], "yy": yy[g]} for g in disc]


def ki(K):
    """fxi, cxi, fyi, cyi as the library's level-0 Ki holds them in float: 1 / fx, -cx / fx, 1 / fy, -cy / fy."""
    fx, fy, cx, cy = [F(x) for x in K]
    return F(1) / fx, -cx / fx, F(1) / fy, -cy / fy


def back_project(xx, yy, idepth, K):
    fxi, cxi, fyi, cyi = ki(K)
    xx, yy, idp = np.asarray(xx).astype(F), np.asarray(yy).astype(F), np.asarray(idepth, F)
    with np.errstate(all="ignore"):
        X = (fxi * xx + cxi) / idp
        Y = (fyi * yy + cyi) / idp
        Z = F(1) / idp
    return X.astype(F), Y.astype(F), Z.astype(F)


def triplet(d, m):
    d0, d1, d2 = int(d[0]), int(d[1]), int(d[2])
    i0 = d0 % m
    i1 = d1 % (m - 1)
    if i1 >= i0:
        i1 += 1
    i2 = d2 % (m - 2)
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


def sample_model(p0, p1, p2):
    """-> (a, b, c, d) float32, or None when the triplet is degenerate (zero or non-finite length of the cross product)."""
    with np.errstate(all="ignore"):
        e1 = [F(p1[k] - p0[k]) for k in range(3)]
        e2 = [F(p2[k] - p0[k]) for k in range(3)]
        nx = F(F(e1[1] * e2[2]) - F(e1[2] * e2[1]))
        ny = F(F(e1[2] * e2[0]) - F(e1[0] * e2[2]))
        nz = F(F(e1[0] * e2[1]) - F(e1[1] * e2[0]))
        ln = np.sqrt(F(F(F(nx * nx) + F(ny * ny)) + F(nz * nz)))
        if not np.isfinite(ln) or ln == 0:
            return None
        a, b, c = F(nx / ln), F(ny / ln), F(nz / ln)
        d = F(-F(F(F(a * p0[0]) + F(b * p0[1])) + F(c * p0[2])))
    return a, b, c, d


def inlier_mask(model, X, Y, Z, threshold):
    a, b, c, d = model
    with np.errstate(all="ignore"):
        dist = np.abs(((a * X + b * Y) + c * Z) + d)
    return dist < F(threshold)          # a NaN distance compares false


def _jacobi3(A, dtype):
    """Cyclic Jacobi on a symmetric 3x3 in `dtype`: 12 sweeps over (0,1), (0,2), (1,2). -> (diagonal, V with the eigenvectors in its columns)."""
    A = [[dtype(A[i][j]) for j in range(3)] for i in range(3)]
    V = [[dtype(1 if i == j else 0) for j in range(3)] for i in range(3)]
    one, two = dtype(1), dtype(2)
    with np.errstate(all="ignore"):
        for _ in range(12):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = A[p][q]
                if apq == 0:
                    continue
                theta = (A[q][q] - A[p][p]) / (two * apq)
                t = one / (abs(theta) + np.sqrt(theta * theta + one))
                if theta < 0:
                    t = -t
                c = one / np.sqrt(t * t + one)
                s = t * c
                for k in range(3):                 # A <- A J (columns p, q)
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(3):                 # A <- J^T A (rows p, q)
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return [A[0][0], A[1][1], A[2][2]], V


def refine(model, X, Y, Z, inl, dtype=np.float64):
    """The plane through the inliers' centroid with the normal of the smallest eigenvalue of their covariance, in `dtype`, sums in index order. -> 4 values of dtype."""
    idx = np.nonzero(inl)[0]
    k = dtype(len(idx))
    P = [np.asarray(X)[idx].astype(dtype), np.asarray(Y)[idx].astype(dtype), np.asarray(Z)[idx].astype(dtype)]
    seq = lambda a: np.cumsum(a)[-1]               # cumsum adds in index order, one rounding per term: the sequential sum
    cen = [seq(P[0]) / k, seq(P[1]) / k, seq(P[2]) / k]
    dv = [P[0] - cen[0], P[1] - cen[1], P[2] - cen[2]]
    C = [[dtype(0)] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(r, 3):
            C[r][c] = C[c][r] = seq(dv[r] * dv[c])
    ev, V = _jacobi3(C, dtype)
    j = 0
    for t in (1, 2):
        if ev[t] < ev[j]:
            j = t
    n = [V[0][j], V[1][j], V[2][j]]
    ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    n = [n[0] / ln, n[1] / ln, n[2] / ln]
    if (n[0] * dtype(model[0]) + n[1] * dtype(model[1])) + n[2] * dtype(model[2]) < 0:
        n = [-n[0], -n[1], -n[2]]
    d = -((n[0] * cen[0] + n[1] * cen[1]) + n[2] * cen[2])
    return np.array([n[0], n[1], n[2], d], dtype)


def fit(xx, yy, idepth, K, draws, threshold=0.01, min_points=10, dtype=np.float64):
    """One cluster. -> dict(n_cloud, fitted, best_sample, inliers, inlier_idx (cloud indices), refined, plane (float32[4]), plane_wide (dtype[4]; the sample
    model's values when not refined), sample (float32[4]))."""
    X, Y, Z = back_project(xx, yy, idepth, K)
    ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
    X, Y, Z = X[ok], Y[ok], Z[ok]
    m = len(X)
    out = {"n_cloud": m, "fitted": 0, "best_sample": -1, "inliers": 0, "inlier_idx": np.zeros(0, np.int64), "refined": False, "plane": np.zeros(4, F),
           "plane_wide": np.zeros(4, dtype), "sample": np.zeros(4, F), "cloud": (X, Y, Z)}
    draws = np.asarray(draws, np.uint32)
    if m < max(int(min_points), 3):
        return out
    best, best_cnt, best_model, best_inl = -1, -1, None, None
    for i in range(len(draws) // 3):
        i0, i1, i2 = triplet(draws[3 * i:3 * i + 3], m)
        mod = sample_model((X[i0], Y[i0], Z[i0]), (X[i1], Y[i1], Z[i1]), (X[i2], Y[i2], Z[i2]))
        if mod is None:
            continue                               # a degenerate sample scores no inliers and never wins
        inl = inlier_mask(mod, X, Y, Z, threshold)
        cnt = int(inl.sum())
        if cnt > best_cnt:                         # the first with the largest count
            best, best_cnt, best_model, best_inl = i, cnt, mod, inl
    if best < 0:
        return out
    out.update(fitted=1, best_sample=best, inliers=best_cnt, inlier_idx=np.nonzero(best_inl)[0], sample=np.array(best_model, F))
    if best_cnt > 3:
        pw = refine(best_model, X, Y, Z, best_inl, dtype)
        out.update(refined=True, plane_wide=pw, plane=pw.astype(F))
    else:
        out.update(plane=np.array(best_model, F), plane_wide=np.array(best_model, F).astype(dtype))
    return out


def fit_planes(u, v, idepth, mask, w, h, K, draws, threshold=0.01, min_points=10, dtype=np.float64, fast=False):
    """The whole call without the append: the clusters of cluster() with rect, n and the fit of every cluster."""
    idepth = np.asarray(idepth, F)
    cl = (cluster_fast if fast else cluster)(u, v, idepth, mask, w, h)
    for c in cl:
        c["n"] = len(c["members"])
        c["rect"] = [int(c["xx"].min()), int(c["xx"].max()), int(c["yy"].min()), int(c["yy"].max())]
        c.update(fit(c["xx"], c["yy"], idepth[c["members"]], K, draws, threshold, min_points, dtype))
    return cl


def append_skipped(c, w, h):
    """CoarseTracker.cpp:591,627,635: the clusters the append loop passes over."""
    minx, maxx, miny, maxy = c["rect"]
    return (not c["fitted"]) or maxx > w - 1 or minx < 1 or maxy > h - 1 or miny < 1 or _c_int(c["mask_value"]) == 0


def planted_plane(seed, n, outlier_share, w=1224, h=368, K=(718.856, 718.856, 607.19, 185.2), height=1.6):
    """n pixels of the lower third of the image on the plane y = height (camera frame, y down), displaced by uniform +-2 mm along the normal, the first
    round(outlier_share * n) of them pulled to 0.5-0.9 of their depth. -> u, v, idepth (float32), planted inlier flags. Pixels are distinct."""
    rng = np.random.RandomState(seed)
    y_lo = (2 * h) // 3
    pix = rng.choice((w - 6) * (h - 3 - y_lo), n, replace=False)
    x = 3 + pix % (w - 6)
    y = y_lo + pix // (w - 6)
    fxi, cxi, fyi, cyi = [float(t) for t in ki(K)]
    ry = fyi * y + cyi
    Z = (height + rng.uniform(-0.002, 0.002, n)) / ry
    n_out = int(round(outlier_share * n))
    planted = np.ones(n, bool)
    planted[:n_out] = False
    Z[:n_out] *= rng.uniform(0.5, 0.9, n_out)
    u = (x + rng.uniform(0.0, 0.99, n)).astype(F)
    v = (y + rng.uniform(0.0, 0.99, n)).astype(F)
    return u, v, (1.0 / Z).astype(F), planted


def make_draws(seed, n_samples=50):
    return np.random.RandomState(1000 + seed).randint(0, 2 ** 32, 3 * n_samples, dtype=np.uint64).astype(np.uint32)
