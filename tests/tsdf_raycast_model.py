"""The literal model of "The ray-cast" of the TSDF section of include/nalo_gpu.h over the volume dict of tests/tsdf_model.py (with tests/tsdf_color_model.py's
"colour" for the colour image): raycast_literal loops over pixels and over EVERY sample number n exactly as the header reads, raycast is the same operations
in the same order on whole images. Everything in float32, one rounding per operation. Neither skips a sample outside the grid: that the device, which visits
only a conservative interval of n, equals them is what shows the interval to be conservative. No device."""
import numpy as np

from tsdf_color_model import colour_byte

F = np.float32
MAX_N = 4096


def steps(min_depth, max_depth, step):
    """the number of n in 0..4096 with z_n = min_depth + (float)n * step <= max_depth, in float32; 4097 is what nalo_tsdf_raycast_steps refuses"""
    mn, mx, st = F(min_depth), F(max_depth), F(step)
    n = 0
    with np.errstate(all="ignore"):
        while n <= MAX_N and mn + F(n) * st <= mx:
            n += 1
    return n


def pose_f32(cam_to_world):
    c = np.asarray(cam_to_world, np.float64).reshape(3, 4).astype(F)
    return c[:, :3], c[:, 3]


def _empty(w, h, normals, colour, N):
    out = dict(depth=np.zeros((h, w), F), n_hit=0, n_back=0, n_normal=0, n_steps=N)
    if normals:
        out["normal"] = np.zeros((h, w, 3), F)
    if colour:
        out["rgba"] = np.zeros((h, w, 4), np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the literal form
def field_literal(vol, arr, q, min_weight):
    """S(q) on arr ([nz][ny][nx]) -> (VALID, S). min_weight None: the colour planes' index test alone"""
    nx, ny, nz = vol["dims"]
    i = [np.floor(q[a]) for a in range(3)]
    for a, n in enumerate((nx, ny, nz)):
        if not (i[a] >= F(0.0) and i[a] <= F(n - 2)):                            # compared in float before any conversion: a NaN or an infinity fails
            return False, F(np.nan)
    f = [q[a] - i[a] for a in range(3)]
    ix, iy, iz = (int(v) for v in i)
    t = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                tv = arr[iz + dz, iy + dy, ix + dx]
                if min_weight is not None and not (vol["weight"][iz + dz, iy + dy, ix + dx] >= min_weight and not np.isnan(tv)):
                    return False, F(np.nan)
                t[dz, dy, dx] = tv                                              # t_zyx
    a00 = t[0, 0, 0] + f[0] * (t[0, 0, 1] - t[0, 0, 0])                          # a_yz
    a10 = t[0, 1, 0] + f[0] * (t[0, 1, 1] - t[0, 1, 0])
    a01 = t[1, 0, 0] + f[0] * (t[1, 0, 1] - t[1, 0, 0])
    a11 = t[1, 1, 0] + f[0] * (t[1, 1, 1] - t[1, 1, 0])
    b0 = a00 + f[1] * (a10 - a00)
    b1 = a01 + f[1] * (a11 - a01)
    S = b0 + f[2] * (b1 - b0)
    assert S.dtype == F
    if min_weight is not None and np.isnan(S):
        return False, S
    return True, S


def pixel_literal(vol, u, v, K, R, t, mn, st, N, mw, normals, colour):
    """one pixel -> (depth, normal [3], rgba [4], code): code 1 a hit, 2 a back face, 0 a miss"""
    fx, fy, cx, cy = (F(k) for k in K)
    o, vs = vol["origin"], vol["vs"]
    rx, ry = (F(u) - cx) / fx, (F(v) - cy) / fy
    d = [(R[a, 0] * rx + R[a, 1] * ry) + R[a, 2] for a in range(3)]

    def grid(z):
        return [((t[a] + d[a] * z) - o[a]) / vs - F(0.5) for a in range(3)]

    nrm, rgba = np.zeros(3, F), np.zeros(4, np.uint8)
    prev = None
    code, depth = 0, F(0.0)
    for n in range(N):                                                          # every n, inside the grid or not
        z = mn + F(n) * st
        ok, S = field_literal(vol, vol["tsdf"], grid(z), mw)
        if ok and prev is not None and (prev < 0) != (S < 0):
            if prev >= 0:
                s = prev / (prev - S)
                depth = (mn + F(n - 1) * st) + st * s
                code = 1
            else:
                code = 2
            break
        prev = S if ok else None
    if code != 1:
        return F(0.0), nrm, rgba, code
    q = grid(depth)
    if normals:
        G, good = [], True
        for a in range(3):
            qp, qm = list(q), list(q)
            qp[a], qm[a] = q[a] + F(1.0), q[a] - F(1.0)
            okp, sp = field_literal(vol, vol["tsdf"], qp, mw)
            okm, sm = field_literal(vol, vol["tsdf"], qm, mw)
            good = good and okp and okm
            G.append(sp - sm)
        if good:
            ln = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
            assert ln.dtype == F
            if ln > 0 and np.isfinite(ln):
                nrm = np.array([G[0] / ln, G[1] / ln, G[2] / ln], F)
    if colour:
        rgba[3] = 255
        for X in range(3):                                                      # the planes are B, G, R
            ok, c = field_literal(vol, vol["colour"][X], q, None)
            if ok:
                rgba[2 - X] = colour_byte(c)
    return depth, nrm, rgba, code


def raycast_literal(vol, w, h, K, cam_to_world, min_depth, max_depth, step, min_weight, normals=False, colour=False, pixels=None):
    """the definition, one pixel and one sample at a time. pixels: a list of (u, v) to evaluate instead of the whole view (the others stay a miss)"""
    N = steps(min_depth, max_depth, step)
    assert 1 <= N <= MAX_N
    R, t = pose_f32(cam_to_world)
    out = _empty(w, h, normals, colour, N)
    todo = [(u, v) for v in range(h) for u in range(w)] if pixels is None else pixels
    with np.errstate(all="ignore"):
        for u, v in todo:
            depth, nrm, rgba, code = pixel_literal(vol, u, v, K, R, t, F(min_depth), F(step), N, F(min_weight), normals, colour)
            out["depth"][v, u] = depth
            out["n_hit"] += code == 1
            out["n_back"] += code == 2
            if normals:
                out["normal"][v, u] = nrm
                out["n_normal"] += bool(nrm.any())
            if colour:
                out["rgba"][v, u] = rgba
    return out


# ------------------------------------------------------------------------------------------------ the same on whole images
def field(vol, arr, qx, qy, qz, min_weight):
    """S(q) for arrays of coordinates -> (VALID, S); S is NaN where the sample is not valid"""
    nx, ny, nz = vol["dims"]
    ix, iy, iz = np.floor(qx), np.floor(qy), np.floor(qz)
    ok = (ix >= F(0.0)) & (ix <= F(nx - 2)) & (iy >= F(0.0)) & (iy <= F(ny - 2)) & (iz >= F(0.0)) & (iz <= F(nz - 2))
    S = np.full(qx.shape, np.nan, F)
    if not ok.any():
        return ok, S
    i, j, k = ix[ok].astype(np.int64), iy[ok].astype(np.int64), iz[ok].astype(np.int64)
    fx, fy, fz = qx[ok] - ix[ok], qy[ok] - iy[ok], qz[ok] - iz[ok]
    t = {(dz, dy, dx): arr[k + dz, j + dy, i + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
    a00 = t[0, 0, 0] + fx * (t[0, 0, 1] - t[0, 0, 0])
    a10 = t[0, 1, 0] + fx * (t[0, 1, 1] - t[0, 1, 0])
    a01 = t[1, 0, 0] + fx * (t[1, 0, 1] - t[1, 0, 0])
    a11 = t[1, 1, 0] + fx * (t[1, 1, 1] - t[1, 1, 0])
    b0 = a00 + fy * (a10 - a00)
    b1 = a01 + fy * (a11 - a01)
    s = b0 + fz * (b1 - b0)
    assert s.dtype == F
    if min_weight is None:
        S[ok] = s
        return ok, S
    good = ~np.isnan(s)
    W = vol["weight"]
    for key, tv in t.items():
        good &= (W[k + key[0], j + key[1], i + key[2]] >= min_weight) & ~np.isnan(tv)
    valid = ok.copy()
    valid[ok] = good
    S[ok] = np.where(good, s, F(np.nan))
    return valid, S


def raycast(vol, w, h, K, cam_to_world, min_depth, max_depth, step, min_weight, normals=False, colour=False):
    """raycast_literal's operations in its order, on [h][w] arrays; every n is evaluated for every pixel that has not ended"""
    N = steps(min_depth, max_depth, step)
    assert 1 <= N <= MAX_N
    R, t = pose_f32(cam_to_world)
    fx, fy, cx, cy = (F(k) for k in K)
    mn, st, mw = F(min_depth), F(step), F(min_weight)
    o, vs = vol["origin"], vol["vs"]
    out = _empty(w, h, normals, colour, N)
    with np.errstate(all="ignore"):
        vv, uu = np.mgrid[0:h, 0:w]
        rx, ry = (uu.astype(F) - cx) / fx, (vv.astype(F) - cy) / fy
        d = [(R[a, 0] * rx + R[a, 1] * ry) + R[a, 2] for a in range(3)]
        assert d[0].dtype == F

        def grid(z, sel=slice(None)):
            return [((t[a] + d[a][sel] * z) - o[a]) / vs - F(0.5) for a in range(3)]

        live = np.ones((h, w), bool)                                            # rays that have not ended
        pv, ps = np.zeros((h, w), bool), np.zeros((h, w), F)
        hit, back = np.zeros((h, w), bool), np.zeros((h, w), bool)
        depth = out["depth"]
        for n in range(N):
            if not live.any():
                break
            z = mn + F(n) * st
            ok, S = field(vol, vol["tsdf"], *grid(z), mw)
            end = live & ok & pv & ((ps < 0) != (S < 0))
            front = end & (ps >= 0)
            if front.any():
                s = ps[front] / (ps[front] - S[front])
                depth[front] = (mn + F(n - 1) * st) + st * s
            hit |= front
            back |= end & ~front
            live &= ~end
            pv, ps = ok, S
        assert depth.dtype == F
        out["n_hit"], out["n_back"] = int(hit.sum()), int(back.sum())
        q = grid(depth)
        if normals:
            G, good = [], hit.copy()
            for a in range(3):
                qp, qm = list(q), list(q)
                qp[a], qm[a] = q[a] + F(1.0), q[a] - F(1.0)
                okp, sp = field(vol, vol["tsdf"], *qp, mw)
                okm, sm = field(vol, vol["tsdf"], *qm, mw)
                good &= okp & okm
                G.append(sp - sm)
            ln = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
            assert ln.dtype == F
            good &= (ln > 0) & np.isfinite(ln)
            for a in range(3):
                out["normal"][..., a][good] = (G[a] / ln)[good]
            out["n_normal"] = int(good.sum())
        if colour:
            out["rgba"][..., 3][hit] = 255
            for X in range(3):
                ok, c = field(vol, vol["colour"][X], *q, None)
                sel = hit & ok
                out["rgba"][..., 2 - X][sel] = colour_byte(c[sel])
    return out
