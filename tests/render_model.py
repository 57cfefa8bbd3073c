"""The literal model of nalo_map_render's DEFINED rasteriser (include/nalo_gpu.h, "The 3-D panel of PangolinDSOViewer"), which tests/test_map_render_gpu.py
compares the device against bit for bit, and a vectorised form of it for the full-size cases (tests/test_map_render_cpu.py holds the two equal).

Points come in as camera-space vertices with colours: what map_model.refresh_pc (draws=None) gives for a frame's records and dense_map_model.refresh_pc_fast for
its dense points - models the device is already pinned against by tests/test_map_gpu.py and tests/test_dense_map_gpu.py. From there every float operation is
explicit: np.float32 scalars for the vertices, np.float64 for the lines, a dictionary per pixel for the depth test.

  cam        dict(vw, vh, fx, fy, cx, cy, znear, zfar), the six camera values np.float32
  cloud      (M float32 [12], xyz float32 [n][3], col uint32 [n] = R << 16 | G << 8 | B)
  segment    (a float32 [3], b float32 [3], col, width): view-space ends"""
import math

import numpy as np

import dense_map_model as dm
import map_model as mm

f32, f64 = np.float32, np.float64
RED, GREEN, BLUE = 0xFF0000, 0x00FF00, 0x0000FF
CAM_EDGES = ((0, 1), (0, 2), (0, 3), (0, 4), (4, 3), (3, 2), (2, 1), (1, 4))        # drawCam's eight segments over frustum()'s points


def make_cam(vw, vh, fx=400.0, fy=400.0, cx=None, cy=None, znear=0.1, zfar=1000.0):
    return dict(vw=int(vw), vh=int(vh), fx=f32(fx), fy=f32(fy), cx=f32(vw / 2 if cx is None else cx), cy=f32(vh / 2 if cy is None else cy), znear=f32(znear), zfar=f32(zfar))


def look_at(eye, target, up):
    """pangolin::ModelViewLookAt in double, rows x, -y, -z -> viewFromWorld [3][4]"""
    e, l, u = (np.asarray(a, f64).reshape(3) for a in (eye, target, up))
    z = e - l
    z = z / np.sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2])
    x = np.array([u[1] * z[2] - u[2] * z[1], u[2] * z[0] - u[0] * z[2], u[0] * z[1] - u[1] * z[0]])
    y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]])
    lx, ly = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), np.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
    R = np.stack([x / lx, -(y / ly), -z])
    t = np.array([-((R[r, 0] * e[0] + R[r, 1] * e[1]) + R[r, 2] * e[2]) for r in range(3)])
    return np.concatenate([R, t[:, None]], 1)


def transform(view, c2w):
    """(float)(viewFromWorld . camToWorld): k = 0, 1, 2 left to right, then the translation, then the cast"""
    V, Cm = np.asarray(view, f64).reshape(3, 4), np.asarray(c2w, f64).reshape(3, 4)
    M = np.zeros((3, 4), f32)
    with np.errstate(all="ignore"):
        for r in range(3):
            for q in range(4):
                s = V[r, 0] * Cm[0, q]
                s = s + V[r, 1] * Cm[1, q]
                s = s + V[r, 2] * Cm[2, q]
                if q == 3:
                    s = s + V[r, 3]
                M[r, q] = f32(s)
    return M.reshape(12)


def apply(M, p):
    """row r: ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3] in float; p [3] or [n][3]"""
    M = np.asarray(M, f32).reshape(3, 4)
    p = np.asarray(p, f32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], -1).astype(f32)


def frustum(cf, w, h, sz):
    """drawCam's apex and corners (KeyFrameDisplay.cpp:630-649) in float: (x0,y0) (x0,y1) (x1,y1) (x1,y0)"""
    fx, fy, cx, cy = (f32(v) for v in cf)
    sz = f32(sz)
    x0, x1 = sz * (f32(0) - cx) / fx, sz * (f32(w - 1) - cx) / fx
    y0, y1 = sz * (f32(0) - cy) / fy, sz * (f32(h - 1) - cy) / fy
    return np.array([[0, 0, 0], [x0, y0, sz], [x0, y1, sz], [x1, y1, sz], [x1, y0, sz]], f32)


def segments(view, frames, cf, w, h, show_kf_cams=False, current_cam=None, connections=None, show_active=False, show_all=False, show_trajectory=False, all_poses=None):
    """the segment list in view space. frames: [(frame_id, camToWorld)]; connections: nalo_map_graph_connections' records"""
    out = []
    Vf = np.asarray(view, f64).reshape(12).astype(f32)
    trans = [np.asarray(m, f64).reshape(3, 4)[:, 3].astype(f32) for _, m in frames]
    index_of = {int(fid): i for i, (fid, _) in enumerate(frames)}

    def cam_lines(M, sz, col, width):
        p = apply(M, frustum(cf, w, h, sz))
        out.extend((p[a], p[b], col, width) for a, b in CAM_EDGES)

    if show_kf_cams:
        for _, m in frames:
            cam_lines(transform(view, m), 0.1, BLUE, 1)
    if current_cam is not None:
        cam_lines(transform(view, current_cam), 0.2, RED, 2)
    for g in (connections if connections is not None else []):
        a, b = index_of.get(int(g["from_id"])), index_of.get(int(g["to_id"]))
        if a is None or b is None:
            continue
        n_act, n_marg = int(g["bwdAct"]) + int(g["fwdAct"]), int(g["bwdMarg"]) + int(g["fwdMarg"])
        pa, pb = apply(Vf, trans[a]), apply(Vf, trans[b])
        if show_all and n_act == 0 and n_marg > 0:
            out.append((pa, pb, GREEN, 1))
        if show_active and n_act > 0:
            out.append((pa, pb, BLUE, 3))
    if show_trajectory:
        out.extend((apply(Vf, trans[i]), apply(Vf, trans[i + 1]), RED, 3) for i in range(len(frames) - 1))
    if all_poses is not None:
        P = apply(Vf, np.asarray(all_poses, f32).reshape(-1, 3))
        out.extend((P[i], P[i + 1], GREEN, 3) for i in range(len(P) - 1))
    return out


def clip_line(cam, a, b):
    """drop rules, near clip, projection, viewport clip in double -> None (dropped) or dict(ua, va, ub, vb, za, zb, n, k0, count)"""
    A, B = [f64(v) for v in a], [f64(v) for v in b]
    if not all(math.isfinite(v) for v in A + B):
        return None
    zn = f64(cam["znear"])
    if A[2] <= zn and B[2] <= zn:
        return None
    if A[2] < zn or B[2] < zn:
        t = (zn - A[2]) / (B[2] - A[2])
        P = [A[i] + t * (B[i] - A[i]) for i in range(3)]
        if A[2] < zn:
            A = P
        else:
            B = P
    fx, fy, cx, cy = (f64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        ua, va, ub, vb = fx * (A[0] / A[2]) + cx, fy * (A[1] / A[2]) + cy, fx * (B[0] / B[2]) + cx, fy * (B[1] / B[2]) + cy
    if not all(math.isfinite(v) for v in (ua, va, ub, vb)):
        return None
    du, dv = ub - ua, vb - va
    n = f64(np.ceil(max(abs(du), abs(dv))))
    t0, t1, inside = f64(0), f64(1), True
    for p, q in ((-du, ua - f64(-2.0)), (du, (f64(cam["vw"]) + f64(2.0)) - ua), (-dv, va - f64(-2.0)), (dv, (f64(cam["vh"]) + f64(2.0)) - va)):
        if p == 0:
            if q < 0:
                inside = False
                break
            continue
        r = q / p
        if p < 0:
            if r > t1:
                inside = False
                break
            if r > t0:
                t0 = r
        else:
            if r < t0:
                inside = False
                break
            if r < t1:
                t1 = r
    k0, count = f64(0), 0
    if inside:
        if n == 0:
            count = 1
        else:
            k0 = f64(np.ceil(t0 * n))
            k1 = f64(np.floor(t1 * n))
            if k1 >= k0:
                count = int(min(k1 - k0 + f64(1), f64(cam["vw"]) + f64(cam["vh"]) + f64(10)))
    return dict(ua=ua, va=va, ub=ub, vb=vb, za=A[2], zb=B[2], n=n, k0=k0, count=count)


def width_block(L):
    return range(-(L // 2), (L - 1) // 2 + 1)


def line_samples(cam, L):
    """the kept samples of a clipped segment -> [(floor(u), floor(v), depth float32)] (floors as Python ints)"""
    out = []
    du, dv = L["ub"] - L["ua"], L["vb"] - L["va"]
    with np.errstate(all="ignore"):
        for j in range(L["count"]):
            k = L["k0"] + f64(j)
            t = f64(0) if L["n"] == 0 else k / L["n"]
            u, v = L["ua"] + t * du, L["va"] + t * dv
            z = f32(f64(1) / ((f64(1) - t) / L["za"] + t / L["zb"]))
            if not (z > cam["znear"] and z < cam["zfar"]):
                continue
            out.append((int(math.floor(u)), int(math.floor(v)), z))
    return out


def sparse_vertices(rec, ci, mode, scaledTH, absTH, minBS):
    xyz, rgb, _, _ = mm.refresh_pc(rec, scaledTH, absTH, mode, minBS, ci, None)
    return xyz, (rgb[:, 0].astype(np.uint32) << 16) | (rgb[:, 1].astype(np.uint32) << 8) | rgb[:, 2].astype(np.uint32)


def dense_vertices(pts, ci):
    xyz, rgb = dm.refresh_pc_fast(pts["u"], pts["v"], pts["idepth"], pts["bgr"], ci)
    return xyz, (rgb[:, 0].astype(np.uint32) << 16) | (rgb[:, 1].astype(np.uint32) << 8) | rgb[:, 2].astype(np.uint32)


def _finish(cam, background, best, counts):
    vw, vh = cam["vw"], cam["vh"]
    rgb = np.empty((vh, vw, 3), np.uint8)
    rgb[:] = np.asarray(background, np.uint8)
    depth = np.full((vh, vw), np.inf, f32)
    for (x, y), (z, col) in best.items():
        rgb[y, x] = ((col >> 16) & 255, (col >> 8) & 255, col & 255)
        depth[y, x] = z
    return dict(rgb=rgb, depth=depth, **counts)


def render_literal(cam, background, clouds, segs):
    """a plain loop over vertices and samples, a dictionary per pixel"""
    vw, vh = cam["vw"], cam["vh"]
    best = {}
    counts = dict(n_vertices=0, n_drawn_points=0, n_segments=0, n_line_samples=0)

    def put(x, y, z, col):
        cur = best.get((x, y))
        if cur is None or z < cur[0] or (z == cur[0] and col < cur[1]):
            best[(x, y)] = (z, int(col))

    with np.errstate(all="ignore"):
        for M, xyz, col in clouds:
            M = np.asarray(M, f32)
            for i in range(len(xyz)):
                counts["n_vertices"] += 1
                x, y, z = f32(xyz[i, 0]), f32(xyz[i, 1]), f32(xyz[i, 2])
                xv = ((M[0] * x + M[1] * y) + M[2] * z) + M[3]
                yv = ((M[4] * x + M[5] * y) + M[6] * z) + M[7]
                zv = ((M[8] * x + M[9] * y) + M[10] * z) + M[11]
                if not (zv > cam["znear"] and zv < cam["zfar"]):
                    continue
                u = cam["fx"] * (xv / zv) + cam["cx"]
                v = cam["fy"] * (yv / zv) + cam["cy"]
                if not (u >= 0 and u < f32(vw) and v >= 0 and v < f32(vh)):
                    continue
                counts["n_drawn_points"] += 1
                put(int(np.floor(u)), int(np.floor(v)), zv, int(col[i]))
        for a, b, col, width in segs:
            L = clip_line(cam, a, b)
            if L is None:
                continue
            counts["n_segments"] += 1
            for px, py, z in line_samples(cam, L):
                counts["n_line_samples"] += 1
                for oy in width_block(width):
                    for ox in width_block(width):
                        if 0 <= px + ox < vw and 0 <= py + oy < vh:
                            put(px + ox, py + oy, z, col)
    return _finish(cam, background, best, counts)


def render_vector(cam, background, clouds, segs):
    """the same picture with arrays: one 64-bit key per pixel, (depth bits << 32) | colour, lowered with np.minimum.at"""
    vw, vh = cam["vw"], cam["vh"]
    plane = np.full(vw * vh, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    counts = dict(n_vertices=0, n_drawn_points=0, n_segments=0, n_line_samples=0)
    with np.errstate(all="ignore"):
        for M, xyz, col in clouds:
            counts["n_vertices"] += len(xyz)
            if not len(xyz):
                continue
            p = apply(M, xyz)
            xv, yv, zv = p[:, 0], p[:, 1], p[:, 2]
            ok = (zv > cam["znear"]) & (zv < cam["zfar"])
            u = (cam["fx"] * (xv / zv).astype(f32)).astype(f32) + cam["cx"]
            v = (cam["fy"] * (yv / zv).astype(f32)).astype(f32) + cam["cy"]
            ok &= (u >= 0) & (u < f32(vw)) & (v >= 0) & (v < f32(vh))
            counts["n_drawn_points"] += int(ok.sum())
            ix, iy = np.floor(u[ok]).astype(np.int64), np.floor(v[ok]).astype(np.int64)
            key = (np.ascontiguousarray(zv[ok]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(col, np.uint32)[ok].astype(np.uint64)
            np.minimum.at(plane, iy * vw + ix, key)
        for a, b, col, width in segs:
            L = clip_line(cam, a, b)
            if L is None:
                continue
            counts["n_segments"] += 1
            if L["count"] == 0:
                continue
            k = L["k0"] + np.arange(L["count"], dtype=f64)
            t = np.zeros(L["count"], f64) if L["n"] == 0 else k / L["n"]
            u, v = L["ua"] + t * (L["ub"] - L["ua"]), L["va"] + t * (L["vb"] - L["va"])
            z = (f64(1) / ((f64(1) - t) / L["za"] + t / L["zb"])).astype(f32)
            ok = (z > cam["znear"]) & (z < cam["zfar"])
            counts["n_line_samples"] += int(ok.sum())
            px, py = np.floor(u[ok]).astype(np.int64), np.floor(v[ok]).astype(np.int64)
            key = (np.ascontiguousarray(z[ok]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(col)
            for oy in width_block(width):
                for ox in width_block(width):
                    x, y = px + ox, py + oy
                    m = (x >= 0) & (x < vw) & (y >= 0) & (y < vh)
                    np.minimum.at(plane, y[m] * vw + x[m], key[m])
    hit = plane != np.uint64(0xFFFFFFFFFFFFFFFF)
    col = (plane & np.uint64(0xFFFFFF)).astype(np.uint32)
    bg = (int(background[0]) << 16) | (int(background[1]) << 8) | int(background[2])
    col = np.where(hit, col, np.uint32(bg))
    rgb = np.stack([(col >> 16) & 255, (col >> 8) & 255, col & 255], 1).astype(np.uint8).reshape(vh, vw, 3)
    depth = np.where(hit, (plane >> np.uint64(32)).astype(np.uint32).view(f32), f32(np.inf)).astype(f32).reshape(vh, vw)
    return dict(rgb=rgb, depth=depth, **counts)


def same(a, b):
    """bit for bit over every pixel of rgb and depth and over the four counts -> list of what differs"""
    bad = [k for k in ("n_vertices", "n_drawn_points", "n_segments", "n_line_samples") if int(a[k]) != int(b[k])]
    if a["rgb"].shape != b["rgb"].shape or not np.array_equal(a["rgb"], b["rgb"]):
        bad.append("rgb")
    if a["depth"].shape != b["depth"].shape or not np.array_equal(np.ascontiguousarray(a["depth"]).view(np.uint32), np.ascontiguousarray(b["depth"]).view(np.uint32)):
        bad.append("depth")
    return bad
