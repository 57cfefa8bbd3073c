"""The literal model of the TSDF section of include/nalo_gpu.h: a per-voxel loop that follows the header's definition operation by operation in float32, a
vectorised numpy form of the same operations, the culling box in float64, the surface points and the plane nalo_tsdf_integrate_frame makes of a dense list.
Neither integration culls: that the device, which visits only the box, equals them is what shows the box to be conservative. No device."""
import numpy as np

F = np.float32
# why a voxel was left alone (integrate's `code`); 0 = updated
UPDATED, BEHIND, OUTSIDE, NO_DEPTH, OCCLUDED = 0, 1, 2, 3, 4


def volume(origin, voxel_size, dims, trunc, max_weight):
    nx, ny, nz = (int(v) for v in dims)
    return dict(origin=np.asarray(origin, F), vs=F(voxel_size), dims=(nx, ny, nz), trunc=F(trunc), max_weight=F(max_weight),
                tsdf=np.ones((nz, ny, nx), F), weight=np.zeros((nz, ny, nx), F))


def world_to_cam(cam_to_world):
    """R^T and -(R^T t), each row summed left to right in float64, every entry then rounded to float32: [3][4]"""
    c = np.asarray(cam_to_world, np.float64).reshape(3, 4)
    M = np.zeros((3, 4), F)
    for r in range(3):
        a, b, e = c[0, r], c[1, r], c[2, r]
        M[r, 0], M[r, 1], M[r, 2] = F(a), F(b), F(e)
        M[r, 3] = F(-((a * c[0, 3] + b * c[1, 3]) + e * c[2, 3]))
    return M


def frustum_box(vol, w, h, K, cam_to_world, max_depth):
    """nalo_tsdf_frustum_box in float64: (lo, hi), hi exclusive, zeros when empty"""
    c = np.asarray(cam_to_world, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(F(k)) for k in K)
    z = np.float64(F(max_depth)) + np.float64(vol["trunc"])
    pts = [c[:, 3].copy()]
    with np.errstate(all="ignore"):
        for vf in (0.0, float(h)):
            for uf in (0.0, float(w)):
                X, Y = (((uf - 0.5) - cx) / fx) * z, (((vf - 0.5) - cy) / fy) * z
                pts.append(np.array([((c[a, 0] * X + c[a, 1] * Y) + c[a, 2] * z) + c[a, 3] for a in range(3)]))
        pts = np.array(pts)
        lo, hi = [0] * 3, [0] * 3
        for a in range(3):
            n, o, vs = vol["dims"][a], np.float64(vol["origin"][a]), np.float64(vol["vs"])
            if np.isnan(pts[:, a]).any():
                lo[a], hi[a] = 0, n
                continue
            l = np.floor((pts[:, a].min() - o) / vs - 0.5) - 1.0
            u = np.ceil((pts[:, a].max() - o) / vs - 0.5) + 2.0
            lo[a] = 0 if not l > 0 else n if l > n else int(l)
            hi[a] = n if not u < n else 0 if u < 0 else int(u)
    if any(lo[a] >= hi[a] for a in range(3)):
        return (0, 0, 0), (0, 0, 0)
    return tuple(lo), tuple(hi)


def integrate_literal(vol, depth, K, cam_to_world, min_depth, max_depth):
    """the definition, one voxel at a time, over EVERY voxel; returns (updated count, code per voxel)"""
    M = world_to_cam(cam_to_world)
    fx, fy, cx, cy = (F(k) for k in K)
    h, w = depth.shape
    o, vs, trunc, mw = vol["origin"], vol["vs"], vol["trunc"], vol["max_weight"]
    nx, ny, nz = vol["dims"]
    mn, mx = F(min_depth), F(max_depth)
    code = np.zeros((nz, ny, nx), np.int8)
    n = 0
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    px, py, pz = o[0] + (F(i) + F(0.5)) * vs, o[1] + (F(j) + F(0.5)) * vs, o[2] + (F(k) + F(0.5)) * vs
                    xc = ((M[0, 0] * px + M[0, 1] * py) + M[0, 2] * pz) + M[0, 3]
                    yc = ((M[1, 0] * px + M[1, 1] * py) + M[1, 2] * pz) + M[1, 3]
                    zc = ((M[2, 0] * px + M[2, 1] * py) + M[2, 2] * pz) + M[2, 3]
                    uf = ((fx * (xc / zc)) + cx) + F(0.5)
                    vf = ((fy * (yc / zc)) + cy) + F(0.5)
                    if not zc > 0:
                        code[k, j, i] = BEHIND
                        continue
                    if not (uf >= 0 and uf < F(w) and vf >= 0 and vf < F(h)):
                        code[k, j, i] = OUTSIDE
                        continue
                    D = depth[int(vf), int(uf)]
                    if not (D >= mn and D <= mx):
                        code[k, j, i] = NO_DEPTH
                        continue
                    sdf = D - zc
                    if sdf < -trunc:
                        code[k, j, i] = OCCLUDED
                        continue
                    d = min(F(1.0), sdf / trunc)
                    t0, w0 = vol["tsdf"][k, j, i], vol["weight"][k, j, i]
                    vol["tsdf"][k, j, i] = (t0 * w0 + d) / (w0 + F(1.0))
                    vol["weight"][k, j, i] = min(w0 + F(1.0), mw)
                    n += 1
    return n, code


def integrate(vol, depth, K, cam_to_world, min_depth, max_depth):
    """the same operations on whole arrays; returns dict(updated, code, uf, vf, zc, sdf, xq) (sdf is NaN where no usable depth was read; xq = xc / zc)"""
    depth = np.asarray(depth, F)
    M = world_to_cam(cam_to_world)
    fx, fy, cx, cy = (F(k) for k in K)
    h, w = depth.shape
    o, vs, trunc, mw = vol["origin"], vol["vs"], vol["trunc"], vol["max_weight"]
    nx, ny, nz = vol["dims"]
    px = (o[0] + (np.arange(nx, dtype=F) + F(0.5)) * vs)[None, None, :]
    py = (o[1] + (np.arange(ny, dtype=F) + F(0.5)) * vs)[None, :, None]
    pz = (o[2] + (np.arange(nz, dtype=F) + F(0.5)) * vs)[:, None, None]
    with np.errstate(all="ignore"):
        xc = ((M[0, 0] * px + M[0, 1] * py) + M[0, 2] * pz) + M[0, 3]
        yc = ((M[1, 0] * px + M[1, 1] * py) + M[1, 2] * pz) + M[1, 3]
        zc = ((M[2, 0] * px + M[2, 1] * py) + M[2, 2] * pz) + M[2, 3]
        xq = xc / zc
        uf = ((fx * xq) + cx) + F(0.5)
        vf = ((fy * (yc / zc)) + cy) + F(0.5)
        assert xc.dtype == F and uf.dtype == F and vf.dtype == F
        code = np.zeros((nz, ny, nx), np.int8)
        front = zc > 0
        inside = (uf >= 0) & (uf < F(w)) & (vf >= 0) & (vf < F(h))
        code[~front] = BEHIND
        code[front & ~inside] = OUTSIDE
        vis = front & inside
        pu, pv = uf[vis].astype(np.int32), vf[vis].astype(np.int32)
        D = depth[pv, pu]
        sdf = np.full((nz, ny, nx), np.nan, F)
        usable = (D >= F(min_depth)) & (D <= F(max_depth))
        s = D - zc[vis]
        sdf[vis] = np.where(usable, s, F(np.nan))
        c = np.where(~usable, NO_DEPTH, np.where(s < -trunc, OCCLUDED, UPDATED)).astype(np.int8)
        code[vis] = c
        up = code == UPDATED
        d = np.minimum(F(1.0), sdf[up] / trunc)
        t0, w0 = vol["tsdf"][up], vol["weight"][up]
        vol["tsdf"][up] = (t0 * w0 + d) / (w0 + F(1.0))
        vol["weight"][up] = np.minimum(w0 + F(1.0), mw)
    assert vol["tsdf"].dtype == F and vol["weight"].dtype == F
    return dict(updated=int(up.sum()), code=code, uf=uf + np.zeros((nz, ny, nx), F), vf=vf + np.zeros((nz, ny, nx), F), zc=zc + np.zeros((nz, ny, nx), F), sdf=sdf,
                xq=xq + np.zeros((nz, ny, nx), F))


def updated_box(code):
    """(lo, hi) of the voxels an integration updated, hi exclusive; None when there is none"""
    k, j, i = np.nonzero(code == UPDATED)
    if len(i) == 0:
        return None
    return (int(i.min()), int(j.min()), int(k.min())), (int(i.max()) + 1, int(j.max()) + 1, int(k.max()) + 1)


def centres(vol):
    o, vs = vol["origin"], vol["vs"]
    nx, ny, nz = vol["dims"]
    return [o[a] + (np.arange(n, dtype=F) + F(0.5)) * vs for a, n in enumerate((nx, ny, nz))]


def _crossing(t0, w0, t1, w1, min_weight):
    return bool(w0 >= min_weight and w1 >= min_weight and ((t0 < 0 and t1 >= 0) or (t0 >= 0 and t1 < 0)))


def surface_points_literal(vol, min_weight, lo=None, size=None):
    nx, ny, nz = vol["dims"]
    lo = (0, 0, 0) if lo is None else tuple(lo)
    size = (nx, ny, nz) if size is None else tuple(size)
    cs, T, W, mw = centres(vol), vol["tsdf"], vol["weight"], F(min_weight)
    out = []
    with np.errstate(all="ignore"):
        for k in range(lo[2], lo[2] + size[2]):
            for j in range(lo[1], lo[1] + size[1]):
                for i in range(lo[0], lo[0] + size[0]):
                    v = (i, j, k)
                    for a in range(3):
                        n = list(v)
                        n[a] += 1
                        if n[a] >= lo[a] + size[a]:
                            continue
                        t0, t1 = T[k, j, i], T[n[2], n[1], n[0]]
                        if not _crossing(t0, W[k, j, i], t1, W[n[2], n[1], n[0]], mw):
                            continue
                        p = [cs[0][i], cs[1][j], cs[2][k]]
                        p[a] = p[a] + vol["vs"] * (t0 / (t0 - t1))
                        out.append(p)
    return np.array(out, F).reshape(-1, 3)


def surface_points(vol, min_weight, lo=None, size=None):
    nx, ny, nz = vol["dims"]
    lo = (0, 0, 0) if lo is None else tuple(lo)
    size = (nx, ny, nz) if size is None else tuple(size)
    sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
    T, W, mw = vol["tsdf"][sl], vol["weight"][sl], F(min_weight)
    cs = centres(vol)
    sz, sy, sx = T.shape
    C = np.zeros((sz, sy, sx, 3), F)
    C[..., 0] = cs[0][lo[0]:lo[0] + sx][None, None, :]
    C[..., 1] = cs[1][lo[1]:lo[1] + sy][None, :, None]
    C[..., 2] = cs[2][lo[2]:lo[2] + sz][:, None, None]
    cross = np.zeros((sz, sy, sx, 3), bool)
    pts = np.repeat(C[:, :, :, None, :], 3, axis=3)                            # [.., axis, xyz]
    with np.errstate(all="ignore"):
        for a, ax in enumerate((2, 1, 0)):                                     # axis a = x, y, z lives on array axis 2, 1, 0
            n = T.shape[ax]
            if n < 2:
                continue
            s0 = [slice(None)] * 3
            s1 = [slice(None)] * 3
            s0[ax], s1[ax] = slice(0, n - 1), slice(1, n)
            s0, s1 = tuple(s0), tuple(s1)
            t0, t1 = T[s0], T[s1]
            cr = (W[s0] >= mw) & (W[s1] >= mw) & (((t0 < 0) & (t1 >= 0)) | ((t0 >= 0) & (t1 < 0)))
            cross[s0 + (a,)] = cr
            pts[s0 + (a, a)] = C[s0 + (a,)] + vol["vs"] * (t0 / (t0 - t1))
    assert pts.dtype == F
    return pts[cross].reshape(-1, 3)


def frame_plane(points, w, h):
    """D[v][u] = 1.0f / idepth of the LAST record at (u, v) of a dense list in append order, 0 where there is none"""
    D = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for u, v, idp in zip(points["u"].tolist(), points["v"].tolist(), points["idepth"]):
            D[v, u] = F(1.0) / F(idp)
    return D
