"""The literal model of nalo_map_render_mesh's triangles (include/nalo_gpu.h, "The mesh in the 3-D panel"), which tests/test_map_render_mesh_gpu.py compares the
device against bit for bit, and a vectorised form of it for the cases beyond the planted shapes (tests/test_map_render_mesh_cpu.py holds the two equal).

The literal form is the header read aloud: every triangle, every pixel of the VIEWPORT (not of the box: the box only decides the class `large`), Python integers
for the snapped coordinates and the edge functions, numpy.float32 scalars up to the snap, numpy.float64 scalars from the weights on. Points and lines are
tests/render_model.py's; the pictures are joined per pixel with the minimum of the 64-bit keys, which is what one key plane does.

  cam      render_model.make_cam's dict
  mesh     (xyz float32 [nv][3] WORLD coordinates, tri int [nt][3], rgba uint8 [nv][4] or None)"""
import math

import numpy as np

import render_model as rm

f32, f64 = np.float32, np.float64
DRAWN, BAD_INDEX, NEAR, GUARD, DEGENERATE, LARGE = 0, 1, 2, 3, 4, 5
GUARD_PIXELS = 131072
DEFAULT_BOX = 65536
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTS = ("n_triangles", "n_tri_bad_index", "n_tri_near", "n_tri_guard", "n_tri_degenerate", "n_tri_large", "n_tri_pixels")
CLASS_COUNT = {BAD_INDEX: "n_tri_bad_index", NEAR: "n_tri_near", GUARD: "n_tri_guard", DEGENERATE: "n_tri_degenerate", LARGE: "n_tri_large"}


def view_vertices(view, xyz):
    """world -> view space through V_f = (float)viewFromWorld with render_model.apply's rounded products"""
    return rm.apply(np.asarray(view, f64).reshape(12).astype(f32), np.asarray(xyz, f32).reshape(-1, 3))


def top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def classify(cam, P, max_box_pixels=0):
    """rules 2-5 for one triangle from its view-space vertices P float32 [3][3] -> dict(cls, X, Y, box, swapped); X, Y Python ints after the exchange"""
    max_box = DEFAULT_BOX if max_box_pixels == 0 else int(max_box_pixels)
    out = dict(cls=DRAWN, X=[0, 0, 0], Y=[0, 0, 0], box=(0, -1, 0, -1), swapped=False)
    P = np.asarray(P, f32).reshape(3, 3)
    for i in range(3):
        if not all(math.isfinite(float(P[i, k])) for k in range(3)) or not (P[i, 2] > cam["znear"]):
            out["cls"] = NEAR
            return out
    X, Y = [], []
    with np.errstate(all="ignore"):
        for i in range(3):
            u = cam["fx"] * (P[i, 0] / P[i, 2]) + cam["cx"]
            v = cam["fy"] * (P[i, 1] / P[i, 2]) + cam["cy"]
            assert u.dtype == f32 and v.dtype == f32
            if not (u > f32(-GUARD_PIXELS) and u < f32(GUARD_PIXELS) and v > f32(-GUARD_PIXELS) and v < f32(GUARD_PIXELS)):
                out["cls"] = GUARD
                return out
            X.append(int(np.floor(u * f32(256) + f32(0.5))))
            Y.append(int(np.floor(v * f32(256) + f32(0.5))))
    A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if A < 0:
        X[1], X[2], Y[1], Y[2] = X[2], X[1], Y[2], Y[1]
        out["swapped"] = True
    out["X"], out["Y"] = X, Y
    if A == 0:
        out["cls"] = DEGENERATE
        return out
    # centres 256 i + 128 inside [min, max]: i from ceil((min - 128) / 256) to floor((max - 128) / 256), clipped to the viewport
    x0, x1 = max(-((128 - min(X)) // 256), 0), min((max(X) - 128) // 256, cam["vw"] - 1)
    y0, y1 = max(-((128 - min(Y)) // 256), 0), min((max(Y) - 128) // 256, cam["vh"] - 1)
    if x1 < x0 or y1 < y0:
        return out
    if (x1 - x0 + 1) * (y1 - y0 + 1) > max_box:
        out["cls"] = LARGE
    out["box"] = (x0, x1, y0, y1)
    return out


def grey(P):
    """colour_mode 1: the byte of a triangle from its view-space vertices in submitted order"""
    P = np.asarray(P, f32).reshape(3, 3).astype(f64)
    with np.errstate(all="ignore"):
        e1, e2 = [P[1, k] - P[0, k] for k in range(3)], [P[2, k] - P[0, k] for k in range(3)]
        nx, ny, nz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        s = abs(nz) / ln if ln > 0 else f64(0)
        return int(np.floor(f64(64.0) + f64(191.0) * s))


def pixel(cam, X, Y, z, col, ix, iy, colour_mode):
    """one pixel of a triangle after the exchange (z float32 [3], col: [3] of (R, G, B), or the grey) -> None or (depth float32, colour word)"""
    px, py = 256 * ix + 128, 256 * iy + 128
    E = []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        dx, dy = X[b] - X[a], Y[b] - Y[a]
        e = dx * (py - Y[a]) - dy * (px - X[a])
        if not (e > 0 or (e == 0 and top_left(dx, dy))):
            return None
        E.append(e)
    w = (E[1], E[2], E[0])                                                       # w0 = E12, w1 = E20, w2 = E01
    A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    assert w[0] + w[1] + w[2] == A and A < 2 ** 53
    t = [f64(w[i]) / f64(z[i]) for i in range(3)]
    q = (t[0] + t[1]) + t[2]
    depth = f32(f64(A) / q)
    if not (depth > cam["znear"] and depth < cam["zfar"]):
        return None
    if colour_mode == 1:
        return depth, col * 0x010101
    word = 0
    for k in range(3):
        val = (((t[0] * f64(col[0][k])) + (t[1] * f64(col[1][k]))) + (t[2] * f64(col[2][k]))) / q
        word = (word << 8) | min(255, int(np.floor(val + f64(0.5))))
    return depth, word


def tris_literal(cam, view, meshes, colour_mode=0, max_box_pixels=0):
    """-> (key plane uint64 [vh * vw], counts)"""
    vw, vh = cam["vw"], cam["vh"]
    best = {}
    counts = dict.fromkeys(COUNTS, 0)
    for xyz, tri, rgba in meshes:
        P = view_vertices(view, xyz)
        tri = np.asarray(tri).reshape(-1, 3)
        nv = len(P)
        for i0, i1, i2 in tri.tolist():
            counts["n_triangles"] += 1
            if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= nv:
                counts["n_tri_bad_index"] += 1
                continue
            idx = [i0, i1, i2]
            T = classify(cam, P[idx], max_box_pixels)
            if T["cls"] != DRAWN:
                counts[CLASS_COUNT[T["cls"]]] += 1
                continue
            if T["swapped"]:
                idx = [i0, i2, i1]
            z = [P[i, 2] for i in idx]
            col = grey(P[[i0, i1, i2]]) if colour_mode == 1 else [[int(c) for c in rgba[i][:3]] for i in idx]
            for iy in range(vh):
                for ix in range(vw):
                    r = pixel(cam, T["X"], T["Y"], z, col, ix, iy, colour_mode)
                    if r is None:
                        continue
                    x0, x1, y0, y1 = T["box"]
                    assert x0 <= ix <= x1 and y0 <= iy <= y1                    # the box holds every covered pixel
                    counts["n_tri_pixels"] += 1
                    cur = best.get((ix, iy))
                    if cur is None or r[0] < cur[0] or (r[0] == cur[0] and r[1] < cur[1]):
                        best[(ix, iy)] = r
    plane = np.full(vw * vh, EMPTY, np.uint64)
    for (ix, iy), (d, word) in best.items():
        plane[iy * vw + ix] = (np.uint64(np.asarray(d, f32).view(np.uint32)) << np.uint64(32)) | np.uint64(word)
    return plane, counts


def tris_vector(cam, view, meshes, colour_mode=0, max_box_pixels=0):
    """the same plane with arrays: every (triangle, box pixel) pair at once"""
    vw, vh = cam["vw"], cam["vh"]
    max_box = DEFAULT_BOX if max_box_pixels == 0 else int(max_box_pixels)
    plane = np.full(vw * vh, EMPTY, np.uint64)
    counts = dict.fromkeys(COUNTS, 0)
    i64 = np.int64
    with np.errstate(all="ignore"):
        for xyz, tri, rgba in meshes:
            Pv = view_vertices(view, xyz)
            tri = np.asarray(tri, i64).reshape(-1, 3)
            nv = len(Pv)
            counts["n_triangles"] += len(tri)
            bad = ((tri < 0) | (tri >= nv)).any(1)
            counts["n_tri_bad_index"] += int(bad.sum())
            tri = tri[~bad]
            if not len(tri):
                continue
            P = Pv[tri]                                                          # [n][3][3]
            near = (~np.isfinite(P)).any((1, 2)) | ~(P[:, :, 2] > cam["znear"]).all(1)
            counts["n_tri_near"] += int(near.sum())
            tri, P = tri[~near], P[~near]
            u = (cam["fx"] * (P[:, :, 0] / P[:, :, 2]).astype(f32)).astype(f32) + cam["cx"]
            v = (cam["fy"] * (P[:, :, 1] / P[:, :, 2]).astype(f32)).astype(f32) + cam["cy"]
            g = f32(GUARD_PIXELS)
            guard = ~((u > -g) & (u < g) & (v > -g) & (v < g)).all(1)
            counts["n_tri_guard"] += int(guard.sum())
            tri, P, u, v = tri[~guard], P[~guard], u[~guard], v[~guard]
            X = np.floor((u * f32(256)).astype(f32) + f32(0.5)).astype(i64)
            Y = np.floor((v * f32(256)).astype(f32) + f32(0.5)).astype(i64)
            A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
            counts["n_tri_degenerate"] += int((A == 0).sum())
            keep = A != 0
            tri, P, X, Y, A = tri[keep], P[keep], X[keep], Y[keep], A[keep]
            order = np.where((A < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))       # the exchange
            rows = np.arange(len(tri))[:, None]
            Xs, Ys, zs, idx, A = X[rows, order], Y[rows, order], P[rows, order, 2], tri[rows, order], np.abs(A)
            x0 = np.maximum(-((128 - Xs.min(1)) // 256), 0)
            x1 = np.minimum((Xs.max(1) - 128) // 256, vw - 1)
            y0 = np.maximum(-((128 - Ys.min(1)) // 256), 0)
            y1 = np.minimum((Ys.max(1) - 128) // 256, vh - 1)
            bw, bh = x1 - x0 + 1, y1 - y0 + 1
            empty = (bw <= 0) | (bh <= 0)
            n = np.where(empty, 0, bw * bh)
            large = n > max_box
            counts["n_tri_large"] += int(large.sum())
            n = np.where(large, 0, n)
            if colour_mode == 1:
                Pd = P.astype(f64)
                e1, e2 = Pd[:, 1] - Pd[:, 0], Pd[:, 2] - Pd[:, 0]
                nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
                ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
                nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
                ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
                s = np.where(ln > 0, np.abs(nz) / np.where(ln > 0, ln, 1.0), 0.0)
                grey_word = np.floor(64.0 + 191.0 * s).astype(np.uint64) * np.uint64(0x010101)
            total = int(n.sum())
            if total == 0:
                continue
            k = np.repeat(np.arange(len(n)), n)
            off = np.arange(total, dtype=i64) - np.repeat(np.cumsum(n) - n, n)
            ix, iy = x0[k] + off % bw[k], y0[k] + off // bw[k]
            px, py = 256 * ix + 128, 256 * iy + 128
            inside = np.ones(total, bool)
            E = []
            for a, b in ((0, 1), (1, 2), (2, 0)):
                dx, dy = (Xs[:, b] - Xs[:, a])[k], (Ys[:, b] - Ys[:, a])[k]
                e = dx * (py - Ys[k, a]) - dy * (px - Xs[k, a])
                inside &= (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
                E.append(e)
            k, ix, iy = k[inside], ix[inside], iy[inside]
            w = [E[1][inside], E[2][inside], E[0][inside]]
            t = [w[i].astype(f64) / zs[k, i].astype(f64) for i in range(3)]
            q = (t[0] + t[1]) + t[2]
            depth = (A[k].astype(f64) / q).astype(f32)
            ok = (depth > cam["znear"]) & (depth < cam["zfar"])
            counts["n_tri_pixels"] += int(ok.sum())
            if colour_mode == 1:
                word = grey_word[k]
            else:
                col = np.asarray(rgba, np.uint8).reshape(-1, 4)
                word = np.zeros(len(k), np.uint64)
                for ch in range(3):
                    c = [col[idx[k, i], ch].astype(f64) for i in range(3)]
                    val = (((t[0] * c[0]) + (t[1] * c[1])) + (t[2] * c[2])) / q
                    word = (word << np.uint64(8)) | np.minimum(255, np.floor(val + 0.5)).astype(np.uint64)
            key = (np.ascontiguousarray(depth).view(np.uint32).astype(np.uint64) << np.uint64(32)) | word
            np.minimum.at(plane, (iy * vw + ix)[ok], key[ok])
    return plane, counts


def key_plane(picture):
    """a render_model picture as the key plane that produced it (a candidate's depth is finite)"""
    depth = np.ascontiguousarray(picture["depth"], f32).reshape(-1)
    rgb = picture["rgb"].reshape(-1, 3).astype(np.uint64)
    key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (rgb[:, 0] << np.uint64(16)) | (rgb[:, 1] << np.uint64(8)) | rgb[:, 2]
    return np.where(np.isfinite(depth), key, EMPTY)


def resolve(cam, background, plane, counts):
    vw, vh = cam["vw"], cam["vh"]
    hit = plane != EMPTY
    bg = (int(background[0]) << 16) | (int(background[1]) << 8) | int(background[2])
    col = np.where(hit, (plane & np.uint64(0xFFFFFF)).astype(np.uint32), np.uint32(bg))
    rgb = np.stack([(col >> 16) & 255, (col >> 8) & 255, col & 255], 1).astype(np.uint8).reshape(vh, vw, 3)
    depth = np.where(hit, (plane >> np.uint64(32)).astype(np.uint32).view(f32), f32(np.inf)).astype(f32).reshape(vh, vw)
    return dict(rgb=rgb, depth=depth, **counts)


def render(cam, background, view, meshes, colour_mode=0, max_box_pixels=0, clouds=(), segs=(), literal=True):
    """nalo_map_render_mesh's picture and its eleven counts: render_model's points and lines and the triangles in one depth test"""
    base = (rm.render_literal if literal else rm.render_vector)(cam, background, list(clouds), list(segs))
    plane, counts = (tris_literal if literal else tris_vector)(cam, view, meshes, colour_mode, max_box_pixels)
    counts.update({k: base[k] for k in ("n_vertices", "n_drawn_points", "n_segments", "n_line_samples")})
    return resolve(cam, background, np.minimum(key_plane(base), plane), counts)


def seeded_mesh(seed, n_tri, cam, view, size=4.0, odd=True):
    """n_tri triangles of three vertices each (world coordinates) around points that project into or near the viewport under `view`, about `size` pixels across,
    with random colours; odd: every 7th triangle is planted into a drop class (behind the near plane, a NaN, far outside, a repeated vertex, a bad index) and
    every 11th is ten times as large -> (xyz float32 [3 n][3], tri int32 [n][3], rgba uint8 [3 n][4])"""
    rng = np.random.RandomState(seed)
    V = np.asarray(view, f64).reshape(3, 4)
    R, t = V[:, :3], V[:, 3]
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    xyz = np.zeros((3 * n_tri, 3), f32)
    tri = np.arange(3 * n_tri, dtype=np.int32).reshape(n_tri, 3)
    for k in range(n_tri):
        z = rng.uniform(0.6, 6.0)
        u, v = rng.uniform(-3, cam["vw"] + 3), rng.uniform(-3, cam["vh"] + 3)
        s = size * (10.0 if odd and k % 11 == 10 else 1.0)
        for j in range(3):
            uj, vj, zj = u + rng.uniform(-s, s), v + rng.uniform(-s, s), z * rng.uniform(0.8, 1.25)
            if rng.randint(3) == 0:
                uj, vj = np.round(uj) + 0.5, np.round(vj) + 0.5                    # a vertex near a pixel centre
            p = np.array([(uj - cx) / fx * zj, (vj - cy) / fy * zj, zj])
            if odd and k % 7 == 6:
                kind = (k // 7) % 5
                if kind == 0 and j == 1:
                    p[2] = -p[2]
                elif kind == 1 and j == 2:
                    p[rng.randint(3)] = np.nan
                elif kind == 2 and j == 0:
                    p[0] = 1e7 * p[2]
                elif kind == 3 and j == 2:
                    xyz[3 * k + 2] = xyz[3 * k]
                    continue
                elif kind == 4 and j == 1:
                    tri[k, 1] = 3 * n_tri if (k // 35) % 2 else -1
            xyz[3 * k + j] = (R.T @ (p - t)).astype(f32)
    rgba = rng.randint(0, 256, (3 * n_tri, 4)).astype(np.uint8)
    return xyz, tri, rgba


def same(a, b):
    """bit for bit over every pixel of rgb and depth and over the eleven counts -> list of what differs"""
    return rm.same(a, b) + [k for k in COUNTS if int(a[k]) != int(b[k])]
