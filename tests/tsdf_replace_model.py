"""The literal model of "The replacement" in the TSDF section of include/nalo_gpu.h, on top of tests/tsdf_model.py and tests/tsdf_color_model.py (imported
unchanged): the estimate's matrix, the culling box with a scale and the box shift in float64 / integers, the removal and the add at an estimate one voxel at a
time over EVERY voxel and as whole-array operations, and the fusion log as a list of dicts. Everything per voxel in float32, one rounding per operation. A
side is a dict (side()); its colour image is uint8 [h][w][3] in B, G, R order; a coloured volume is tsdf_color_model.volume's. Neither form culls: that the
device, which visits only the hull of the two boxes, equals them is what shows the boxes to be conservative. No device."""
import numpy as np

import tsdf_color_model as cm
import tsdf_model as tm

F = np.float32


def est_world_to_cam(cam_to_world, s):
    """M_aj = Rt[a][j] / s, M_a3 = -(((Rt_a0 t0 + Rt_a1 t1) + Rt_a2 t2)) / s in float64, every entry then rounded to float32: [3][4]"""
    c = np.asarray(cam_to_world, np.float64).reshape(3, 4)
    s = np.float64(s)
    M = np.zeros((3, 4), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            a, b, e = c[0, r], c[1, r], c[2, r]
            M[r, 0], M[r, 1], M[r, 2] = F(a / s), F(b / s), F(e / s)
            M[r, 3] = F(-((a * c[0, 3] + b * c[1, 3]) + e * c[2, 3]) / s)
    return M


def frustum_box_est(vol, w, h, K, cam_to_world, s, max_depth):
    """nalo_tsdf_frustum_box_est in float64: tm.frustum_box with z = max_depth + trunc / s and every far corner at (((c0 X + c1 Y) + c2 z) * s) + c3"""
    c = np.asarray(cam_to_world, np.float64).reshape(3, 4)
    s = np.float64(s)
    fx, fy, cx, cy = (np.float64(F(k)) for k in K)
    with np.errstate(all="ignore"):
        z = np.float64(F(max_depth)) + np.float64(vol["trunc"]) / s
        pts = [c[:, 3].copy()]
        for vf in (0.0, float(h)):
            for uf in (0.0, float(w)):
                X, Y = (((uf - 0.5) - cx) / fx) * z, (((vf - 0.5) - cy) / fy) * z
                pts.append(np.array([(((c[a, 0] * X + c[a, 1] * Y) + c[a, 2] * z) * s) + c[a, 3] for a in range(3)]))
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


def box_shift(dims, shift, lo, size):
    """nalo_tsdf_box_shift: the box [lo, lo + size) translated by -shift and clipped to the grid, (lo, size); zeros when nothing is left. Python integers"""
    l = [int(lo[a]) - int(shift[a]) for a in range(3)]
    u = [l[a] + int(size[a]) for a in range(3)]
    l = [max(v, 0) for v in l]
    u = [min(u[a], int(dims[a])) for a in range(3)]
    if any(int(size[a]) < 1 or l[a] >= u[a] for a in range(3)):
        return (0, 0, 0), (0, 0, 0)
    return tuple(l), tuple(u[a] - l[a] for a in range(3))


def side(depth, K, cam_to_world, s, min_depth, max_depth, bgr=None):
    return dict(depth=np.asarray(depth, F), K=tuple(K), c2w=np.asarray(cam_to_world, np.float64).reshape(3, 4), s=float(s), mn=F(min_depth), mx=F(max_depth),
                bgr=None if bgr is None else np.asarray(bgr, np.uint8))


def fminf(a, b):
    """C's fminf on two float32 scalars: the other operand when one is a NaN"""
    return b if a != a else a if b != b else min(a, b)


def sample_one(vol, sd, M, i, j, k):
    """the predicate at one voxel: None when the side leaves it alone, else (d, pu, pv)"""
    fx, fy, cx, cy = (F(v) for v in sd["K"])
    h, w = sd["depth"].shape
    o, vs, trunc = vol["origin"], vol["vs"], vol["trunc"]
    px, py, pz = o[0] + (F(i) + F(0.5)) * vs, o[1] + (F(j) + F(0.5)) * vs, o[2] + (F(k) + F(0.5)) * vs
    xc = ((M[0, 0] * px + M[0, 1] * py) + M[0, 2] * pz) + M[0, 3]
    yc = ((M[1, 0] * px + M[1, 1] * py) + M[1, 2] * pz) + M[1, 3]
    zc = ((M[2, 0] * px + M[2, 1] * py) + M[2, 2] * pz) + M[2, 3]
    uf = ((fx * (xc / zc)) + cx) + F(0.5)
    vf = ((fy * (yc / zc)) + cy) + F(0.5)
    if not (zc > 0 and uf >= 0 and uf < F(w) and vf >= 0 and vf < F(h)):
        return None
    pu, pv = int(uf), int(vf)
    D = sd["depth"][pv, pu]
    if not (D >= sd["mn"] and D <= sd["mx"]):
        return None
    sdf = (D - zc) * F(sd["s"])
    if sdf < -trunc:
        return None
    return fminf(F(1.0), sdf / trunc), pu, pv


def _in_box(box, i, j, k):
    return box is None or all(box[0][a] <= v < box[0][a] + box[1][a] for a, v in enumerate((i, j, k)))


def replace_literal(vol, remove=None, add=None, box=None):
    """the definition, one voxel at a time over EVERY voxel: the removal where `remove` accepts the voxel (and the box holds it), then the add where `add`
    does. Returns dict(removed, reset, added, written)"""
    nx, ny, nz = vol["dims"]
    Mr = None if remove is None else est_world_to_cam(remove["c2w"], remove["s"])
    Ma = None if add is None else est_world_to_cam(add["c2w"], add["s"])
    T, W, Cv, mw = vol["tsdf"], vol["weight"], vol.get("colour"), vol["max_weight"]
    n = dict(removed=0, reset=0, added=0, written=0)
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    fired = False
                    r = sample_one(vol, remove, Mr, i, j, k) if remove is not None and _in_box(box, i, j, k) else None
                    if r is not None:
                        d, pu, pv = r
                        t0, w0 = T[k, j, i], W[k, j, i]
                        w1 = w0 - F(1.0)
                        rs = not w1 > 0
                        T[k, j, i], W[k, j, i] = (F(1.0), F(0.0)) if rs else ((t0 * w0 - d) / w1, w1)
                        if remove["bgr"] is not None:
                            for X in range(3):
                                Cv[X, k, j, i] = F(0.0) if rs else (Cv[X, k, j, i] * w0 - F(remove["bgr"][pv, pu, X])) / w1
                        n["removed"] += 1
                        n["reset"] += rs
                        fired = True
                    r = sample_one(vol, add, Ma, i, j, k) if add is not None else None
                    if r is not None:
                        d, pu, pv = r
                        t0, w0 = T[k, j, i], W[k, j, i]
                        T[k, j, i], W[k, j, i] = (t0 * w0 + d) / (w0 + F(1.0)), fminf(w0 + F(1.0), mw)
                        if add["bgr"] is not None:
                            for X in range(3):
                                Cv[X, k, j, i] = (Cv[X, k, j, i] * w0 + F(add["bgr"][pv, pu, X])) / (w0 + F(1.0))
                        n["added"] += 1
                        fired = True
                    n["written"] += fired
    return n


def sample(vol, sd):
    """the predicate on whole arrays: (accepted [nz][ny][nx] bool, d, pu, pv), the last three meaningful where accepted"""
    M = est_world_to_cam(sd["c2w"], sd["s"])
    fx, fy, cx, cy = (F(v) for v in sd["K"])
    h, w = sd["depth"].shape
    o, vs, trunc = vol["origin"], vol["vs"], vol["trunc"]
    nx, ny, nz = vol["dims"]
    px = (o[0] + (np.arange(nx, dtype=F) + F(0.5)) * vs)[None, None, :]
    py = (o[1] + (np.arange(ny, dtype=F) + F(0.5)) * vs)[None, :, None]
    pz = (o[2] + (np.arange(nz, dtype=F) + F(0.5)) * vs)[:, None, None]
    with np.errstate(all="ignore"):
        xc = ((M[0, 0] * px + M[0, 1] * py) + M[0, 2] * pz) + M[0, 3]
        yc = ((M[1, 0] * px + M[1, 1] * py) + M[1, 2] * pz) + M[1, 3]
        zc = ((M[2, 0] * px + M[2, 1] * py) + M[2, 2] * pz) + M[2, 3]
        uf = ((fx * (xc / zc)) + cx) + F(0.5)
        vf = ((fy * (yc / zc)) + cy) + F(0.5)
        assert xc.dtype == F and uf.dtype == F and vf.dtype == F
        vis = np.broadcast_to((zc > 0) & (uf >= 0) & (uf < F(w)) & (vf >= 0) & (vf < F(h)), (nz, ny, nx))
        pu = np.where(vis, uf, F(0)).astype(np.int32)
        pv = np.where(vis, vf, F(0)).astype(np.int32)
        D = sd["depth"][pv, pu]
        usable = vis & (D >= sd["mn"]) & (D <= sd["mx"])
        sdf = (D - zc) * F(sd["s"])
        assert sdf.dtype == F
        acc = usable & ~(sdf < -trunc)
        d = np.fmin(F(1.0), sdf / trunc)
    return acc, d, pu, pv


def replace(vol, remove=None, add=None, box=None):
    """the same operations on whole arrays. Returns dict(removed, reset, added, written, rem, add): the counts and the two masks"""
    nx, ny, nz = vol["dims"]
    T, W, Cv, mw = vol["tsdf"], vol["weight"], vol.get("colour"), vol["max_weight"]
    rem_m, add_m = np.zeros((nz, ny, nx), bool), np.zeros((nz, ny, nx), bool)
    n = dict(removed=0, reset=0, added=0)
    with np.errstate(all="ignore"):
        if remove is not None:
            acc, d, pu, pv = sample(vol, remove)
            if box is not None:
                inb = np.zeros((nz, ny, nx), bool)
                inb[box[0][2]:box[0][2] + box[1][2], box[0][1]:box[0][1] + box[1][1], box[0][0]:box[0][0] + box[1][0]] = True
                acc = acc & inb
            t0, w0 = T[acc], W[acc]
            w1 = w0 - F(1.0)
            rs = ~(w1 > 0)
            T[acc] = np.where(rs, F(1.0), (t0 * w0 - d[acc]) / w1)
            W[acc] = np.where(rs, F(0.0), w1)
            if remove["bgr"] is not None:
                for X in range(3):
                    Cv[X][acc] = np.where(rs, F(0.0), (Cv[X][acc] * w0 - remove["bgr"][pv[acc], pu[acc], X].astype(F)) / w1)
            rem_m = acc
            n["removed"], n["reset"] = int(acc.sum()), int(rs.sum())
        if add is not None:
            acc, d, pu, pv = sample(vol, add)
            t0, w0 = T[acc], W[acc]
            T[acc] = (t0 * w0 + d[acc]) / (w0 + F(1.0))
            W[acc] = np.fmin(w0 + F(1.0), mw)
            if add["bgr"] is not None:
                for X in range(3):
                    Cv[X][acc] = (Cv[X][acc] * w0 + add["bgr"][pv[acc], pu[acc], X].astype(F)) / (w0 + F(1.0))
            add_m = acc
            n["added"] = int(acc.sum())
    assert T.dtype == F and W.dtype == F and (Cv is None or Cv.dtype == F)
    n.update(written=int((rem_m | add_m).sum()), rem=rem_m, add=add_m)
    return n


def hull(vol, remove=None, add=None, box=None):
    """what nalo_tsdf_last reports after nalo_tsdf_replace_depth: (lo, hi, visited) of the hull of the two sides' boxes, the remove side's cut by `box`"""
    boxes = []
    for sd, cut in ((remove, box), (add, None)):
        if sd is None:
            continue
        h, w = sd["depth"].shape
        lo, hi = frustum_box_est(vol, w, h, sd["K"], sd["c2w"], sd["s"], sd["mx"])
        if cut is not None:
            lo = tuple(max(lo[a], cut[0][a]) for a in range(3))
            hi = tuple(min(hi[a], cut[0][a] + cut[1][a]) for a in range(3))
        if all(lo[a] < hi[a] for a in range(3)):
            boxes.append((lo, hi))
    if not boxes:
        return (0, 0, 0), (0, 0, 0), 0
    lo = tuple(min(b[0][a] for b in boxes) for a in range(3))
    hi = tuple(max(b[1][a] for b in boxes) for a in range(3))
    return lo, hi, (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])


# ---- the fusion log: a list of dicts in the order the frames were first fused
def log_put(log, dims, frame_id, n_records, cam_to_world, s, K, min_depth, max_depth, coloured=True):
    """the frame's entry, new or rewritten in place: fused just now (coloured: into a volume that holds colour), resident in the whole grid"""
    e = next((e for e in log if e["frame_id"] == frame_id), None)
    if e is None:
        e = dict(frame_id=frame_id)
        log.append(e)
    e.update(n_records=int(n_records), cam_to_world=np.asarray(cam_to_world, np.float64).reshape(3, 4).copy(), s=float(s), K=tuple(float(F(k)) for k in K),
             min_depth=float(F(min_depth)), max_depth=float(F(max_depth)), lo=(0, 0, 0), size=tuple(int(v) for v in dims), coloured=bool(coloured))


def log_shift(log, dims, shift):
    """behind a non-zero shift: every resident box through box_shift, entries whose box is empty dropped"""
    if not any(int(v) for v in shift):
        return
    kept = []
    for e in log:
        lo, size = box_shift(dims, shift, e["lo"], e["size"])
        if size[0] > 0:
            kept.append(dict(e, lo=lo, size=size))
    log[:] = kept


def log_drop(log, frame_id):
    log[:] = [e for e in log if e["frame_id"] != frame_id]


def log_equal(a, b):
    """two logs (the model's, or binding.Context.tsdf_log_get's) entry by entry"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if any(x[k] != y[k] for k in ("frame_id", "n_records", "s", "min_depth", "max_depth", "coloured")) or tuple(x["lo"]) != tuple(y["lo"]) or tuple(x["size"]) != tuple(y["size"]):
            return False
        if tuple(x["K"]) != tuple(y["K"]) or np.asarray(x["cam_to_world"], np.float64).tobytes() != np.asarray(y["cam_to_world"], np.float64).tobytes():
            return False
    return True


def coloured_volume(origin, voxel_size, dims, trunc, max_weight):
    return cm.volume(origin, voxel_size, dims, trunc, max_weight)
