"""The literal model of the "Colour" part of the TSDF section of include/nalo_gpu.h, on top of tests/tsdf_model.py and tests/tsdf_mesh_model.py (imported
unchanged): the per-voxel colour update one voxel at a time next to tm.integrate_literal and as whole-array operations next to tm.integrate, the colour plane
nalo_tsdf_integrate_frame makes of a dense list, the vertex colours of nalo_tsdf_mesh_color one vertex at a time and on whole arrays, and the bytes of the
coloured PLY file. Everything in float32, one rounding per operation. A colour image is uint8 [h][w][3] in B, G, R order; the colour volume is float32
[3][nz][ny][nx] with the planes in that order. No device."""
import struct

import numpy as np

import tsdf_mesh_model as mm
import tsdf_model as tm

F = np.float32


def volume(origin, voxel_size, dims, trunc, max_weight):
    vol = tm.volume(origin, voxel_size, dims, trunc, max_weight)
    vol["colour"] = np.zeros((3,) + vol["tsdf"].shape, F)
    return vol


def integrate_literal(vol, depth, bgr, K, cam_to_world, min_depth, max_depth):
    """tm.integrate_literal, and at every voxel it updated, with w0 the weight BEFORE: X = (X0 * w0 + (float)x) / (w0 + 1.0f) for the three planes, x the byte at
    the voxel's pixel. The pixel is worked out again here, operation by operation as the header states it. Returns (updated count, code per voxel)."""
    w_before = vol["weight"].copy()
    n, code = tm.integrate_literal(vol, depth, K, cam_to_world, min_depth, max_depth)
    M = tm.world_to_cam(cam_to_world)
    fx, fy, cx, cy = (F(k) for k in K)
    o, vs = vol["origin"], vol["vs"]
    nx, ny, nz = vol["dims"]
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    if code[k, j, i] != tm.UPDATED:
                        continue
                    px, py, pz = o[0] + (F(i) + F(0.5)) * vs, o[1] + (F(j) + F(0.5)) * vs, o[2] + (F(k) + F(0.5)) * vs
                    xc = ((M[0, 0] * px + M[0, 1] * py) + M[0, 2] * pz) + M[0, 3]
                    yc = ((M[1, 0] * px + M[1, 1] * py) + M[1, 2] * pz) + M[1, 3]
                    zc = ((M[2, 0] * px + M[2, 1] * py) + M[2, 2] * pz) + M[2, 3]
                    pu, pv = int(((fx * (xc / zc)) + cx) + F(0.5)), int(((fy * (yc / zc)) + cy) + F(0.5))
                    w0 = w_before[k, j, i]
                    for X in range(3):
                        x0 = vol["colour"][X, k, j, i]
                        vol["colour"][X, k, j, i] = (x0 * w0 + F(bgr[pv, pu, X])) / (w0 + F(1.0))
    return n, code


def integrate(vol, depth, bgr, K, cam_to_world, min_depth, max_depth):
    """the same operations on whole arrays: tm.integrate's result"""
    w_before = vol["weight"].copy()
    r = tm.integrate(vol, depth, K, cam_to_world, min_depth, max_depth)
    up = r["code"] == tm.UPDATED
    pu, pv = r["uf"][up].astype(np.int32), r["vf"][up].astype(np.int32)
    w0 = w_before[up]
    with np.errstate(all="ignore"):
        for X in range(3):
            plane = vol["colour"][X]
            plane[up] = (plane[up] * w0 + bgr[pv, pu, X].astype(F)) / (w0 + F(1.0))
    assert vol["colour"].dtype == F
    return r


def frame_color_plane(points, w, h):
    """uint8 [h][w][3]: the bgr of the LAST record at (u, v) of a dense list in append order, (0, 0, 0) where there is none"""
    Cp = np.zeros((h, w, 3), np.uint8)
    for u, v, c in zip(points["u"].tolist(), points["v"].tolist(), points["bgr"]):
        Cp[v, u] = c
    return Cp


def colour_byte(c):
    """(uint8)(int)(fminf(fmaxf(c, 0.0f), 255.0f) + 0.5f): fmaxf turns a NaN into 0"""
    with np.errstate(all="ignore"):
        return (np.fmin(np.fmax(np.asarray(c, F), F(0.0)), F(255.0)) + F(0.5)).astype(np.int32).astype(np.uint8)


def mesh_colours_literal(vol, min_weight, lo=None, size=None):
    """uint8 [nv][4], R, G, B, 255 per vertex of mm.mesh_literal in its order: cX = X(v) + s * (X(n) - X(v)) with the s of the position"""
    owner = mm.mesh_literal(vol, min_weight, lo, size)[2]
    T, Cv = vol["tsdf"], vol["colour"]
    out = np.zeros((len(owner), 4), np.uint8)
    with np.errstate(all="ignore"):
        for q, (i, j, k, m) in enumerate(owner):
            d = mm.bits(m)
            n = (i + d[0], j + d[1], k + d[2])
            t0, t1 = T[k, j, i], T[n[2], n[1], n[0]]
            s = t0 / (t0 - t1)
            for X in range(3):
                xv, xn = Cv[X, k, j, i], Cv[X, n[2], n[1], n[0]]
                out[q, 2 - X] = colour_byte(xv + s * (xn - xv))
            out[q, 3] = 255
    return out


def mesh_colours(vol, min_weight, lo=None, size=None):
    """the same on whole arrays; the vertices are found and ordered as mm.mesh finds and orders them"""
    lo, size = mm._box(vol, lo, size)
    sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
    T, W, mw = vol["tsdf"][sl], vol["weight"][sl], F(min_weight)
    Cv = vol["colour"][(slice(None),) + sl]
    sz, sy, sx = T.shape
    keys, parts = [], []
    with np.errstate(all="ignore"):
        valid = (W >= mw) & ~np.isnan(T)
        inside = T < 0
        for m in range(1, 8):
            d = mm.bits(m)
            if sx - d[0] < 1 or sy - d[1] < 1 or sz - d[2] < 1:
                continue
            s0 = (slice(0, sz - d[2]), slice(0, sy - d[1]), slice(0, sx - d[0]))
            s1 = (slice(d[2], sz), slice(d[1], sy), slice(d[0], sx))
            z, y, x = np.nonzero(valid[s0] & valid[s1] & (inside[s0] != inside[s1]))
            if len(z) == 0:
                continue
            t0, t1 = T[z, y, x], T[z + d[2], y + d[1], x + d[0]]
            s = t0 / (t0 - t1)
            c = np.full((len(z), 4), 255, np.uint8)
            for X in range(3):
                xv, xn = Cv[X, z, y, x], Cv[X, z + d[2], y + d[1], x + d[0]]
                cx = xv + s * (xn - xv)
                assert cx.dtype == F
                c[:, 2 - X] = colour_byte(cx)
            keys.append(((z.astype(np.int64) * sy + y) * sx + x) * 8 + m)
            parts.append(c)
    if not keys:
        return np.zeros((0, 4), np.uint8)
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(parts)[order]


def ply_bytes(xyz, rgba, tri):
    """binary_little_endian 1.0: float x y z and uchar red green blue alpha per vertex, list uchar int vertex_indices per face"""
    x, c, t = np.asarray(xyz, "<f4").reshape(-1, 3), np.asarray(rgba, np.uint8).reshape(-1, 4), np.asarray(tri, "<i4").reshape(-1, 3)
    assert len(x) == len(c)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
            "property uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(x), len(t)))
    out = [head.encode("ascii")]
    for p, q in zip(x, c):
        out.append(p.tobytes() + q.tobytes())
    for row in t:
        out.append(struct.pack("<Biii", 3, int(row[0]), int(row[1]), int(row[2])))
    return b"".join(out)
