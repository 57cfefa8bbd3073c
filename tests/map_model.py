"""The literal model of the map side that tests/test_map_gpu.py compares the device against (reference paths relative to src/):

  flag_points_push   the push-backs of FullSystem::flagPointsForRemoval (FullSystem/FullSystem.cpp:968, 996, 1001, 1008) given the decisions
  add_point_rewrite  what marginalizePointsF's accSSE_bot->addPoint(p, false) writes back into the PointHessian (OptimizationBackend/AccumulatedSCHessian.cpp:36-50)
  set_from_kf        KeyFrameDisplay::setFromKF (IOWrapper/Pangolin/KeyFrameDisplay.cpp:92-177)
  refresh_pc         KeyFrameDisplay::refreshPC (:297-410)
  world_points       SampleOutputWrapper::publishKeyframes(final = true) (IOWrapper/OutputWrapper/SampleOutputWrapper.h:110-118)

Every float operation is explicit in np.float32 / np.float64, in the reference's order; arrays are used only to run the same scalar statement over all records.
A record is a row of RECORD (the library's nalo_map_record plus nothing)."""
import numpy as np

f32, f64 = np.float32, np.float64
RECORD = np.dtype([("u", f32), ("v", f32), ("idepth", f32), ("idepth_hessian", f32), ("maxRelBaseline", f32),
                   ("status", np.int32), ("decision", np.int32), ("frame_id", np.int32), ("color", f32, 8)])
KEEP, DROP_NORES, DROP, MARGINALIZE = 0, 1, 2, 3
IDEPTH_FIX_PRIOR = f32(50 * 50)                 # setting_idepthFixPrior (util/settings.cpp:60)
IDEPTH_FIX_PRIOR_MARG_FAC = f32(600 * 600)      # setting_idepthFixPriorMargFac (:61)
SCALE_IDEPTH = f32(1)
RAND_MAX = 2147483647
PATTERN = np.array([[0, -2], [-1, -1], [1, -1], [-2, 0], [0, 0], [2, 0], [-1, 1], [0, 2]], np.int32)      # staticPattern[8] (util/settings.cpp:297)


def add_point_rewrite(idepth_hessian, max_rel_baseline, Hdd_post, HdiF_post, has_prior):
    """addPoint on a marginalised point: priorF *= setting_idepthFixPriorMargFac happened just before (EnergyFunctional.cpp:630). No active residual
    (the accumulation left HdiF = 0): idepth_hessian = maxRelBaseline = 0; else idepth_hessian = H, floor 1e-10, maxRelBaseline stays."""
    prior = np.where(np.asarray(has_prior).astype(bool), IDEPTH_FIX_PRIOR * SCALE_IDEPTH * SCALE_IDEPTH, f32(0)).astype(f32)
    prior = (prior * IDEPTH_FIX_PRIOR_MARG_FAC).astype(f32)
    H = (np.asarray(Hdd_post, f32) + prior).astype(f32)
    H = np.where(H < f32(1e-10), f32(1e-10), H).astype(f32)
    none = np.asarray(HdiF_post, f32) == 0
    return np.where(none, f32(0), H).astype(f32), np.where(none, f32(0), np.asarray(max_rel_baseline, f32)).astype(f32)


def flag_points_push(host, frame_ids, u, v, idepth, color, dec, H_flag, max_rel_baseline, Hdd_post, HdiF_post, has_prior):
    """-> {frame_id: (pointHessiansMarginalized, pointHessiansOut)} as RECORD arrays, each in submission order, for one flagPointsForRemoval +
    marginalizePointsF. H_flag / max_rel_baseline: PointHessian::idepth_hessian / maxRelBaseline when the decisions are made; *_post: the point sums
    after the marginalisation's accumulation."""
    dec = np.asarray(dec)
    H2, rb2 = add_point_rewrite(H_flag, max_rel_baseline, Hdd_post, HdiF_post, has_prior)
    out = {}
    for h, fid in enumerate(frame_ids):
        lists = []
        for status in (2, 3):
            idx = np.nonzero((np.asarray(host) == h) & ((dec == MARGINALIZE) if status == 2 else ((dec == DROP) | (dec == DROP_NORES))))[0]
            r = np.zeros(len(idx), RECORD)
            r["u"], r["v"] = np.asarray(u, f32)[idx], np.asarray(v, f32)[idx]
            r["idepth"] = (SCALE_IDEPTH * np.asarray(idepth, f32)[idx]).astype(f32)                   # idepth_scaled
            r["idepth_hessian"] = (H2 if status == 2 else np.asarray(H_flag, f32))[idx]
            r["maxRelBaseline"] = (rb2 if status == 2 else np.asarray(max_rel_baseline, f32))[idx]
            r["status"], r["decision"], r["frame_id"] = status, dec[idx], fid
            r["color"] = np.asarray(color, f32).reshape(-1, 8)[idx]
            lists.append(r)
        out[fid] = tuple(lists)
    return out


def set_from_kf(immature=None, active=None, marginalized=None, out=None):
    """the sparse input list of the display. immature: dict(u, v, idepth_min, idepth_max, color); the others: RECORD arrays (status is set here)"""
    parts = []
    if immature is not None:
        n = len(immature["u"])
        r = np.zeros(n, RECORD)
        r["u"], r["v"] = immature["u"], immature["v"]
        with np.errstate(all="ignore"):
            r["idepth"] = ((np.asarray(immature["idepth_max"], f32) + np.asarray(immature["idepth_min"], f32)).astype(f32) * f32(0.5)).astype(f32)
        r["idepth_hessian"], r["maxRelBaseline"], r["status"] = f32(1000), f32(0), 0
        r["color"] = np.asarray(immature["color"], f32).reshape(n, 8)
        parts.append(r)
    for status, a in ((1, active), (2, marginalized), (3, out)):
        if a is not None:
            a = a.copy()
            a["status"] = status
            parts.append(a)
    return np.concatenate(parts) if parts else np.zeros(0, RECORD)


def color_byte(x):
    """float -> unsigned char by truncation toward zero, defined as saturating to 0..255 with NaN -> 0"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        t = np.where(np.isnan(x), f32(0), np.clip(x, f32(0), f32(255)))
    return np.trunc(t).astype(np.uint8)


def refresh_pc(rec, scaledTH, absTH, mode, minBS, calib_inv, draws=None):
    """-> vertices [n][3] float32, colours [n][3] uint8, records per status [4], survivors per status [4]. calib_inv = float {fxi, fyi, cxi, cyi};
    draws: the rand() stream (one value per output vertex); None: the no-jitter form, rand() / (float)RAND_MAX - 0.5f == 0"""
    fxi, fyi, cxi, cyi = (f32(x) for x in calib_inv)
    scaledTH, absTH, minBS = f32(scaledTH), f32(absTH), f32(minBS)
    st = rec["status"]
    with np.errstate(all="ignore"):
        skip = np.zeros(len(rec), bool)
        if mode == 1:
            skip |= (st != 1) & (st != 2)
        if mode == 2:
            skip |= st != 1
        if mode > 2:
            skip |= True
        idepth = rec["idepth"].astype(f32)
        skip |= idepth < 0
        depth = (f32(1.0) / idepth).astype(f32)
        depth4 = (depth * depth).astype(f32)
        depth4 = (depth4 * depth4).astype(f32)
        var = (f64(1.0) / (rec["idepth_hessian"].astype(f64) + f64(0.01))).astype(f32)     # 1.0f / (float + double literal): a double division, stored in a float
        skip |= (var * depth4).astype(f32) > scaledTH
        skip |= var > absTH
        skip |= rec["maxRelBaseline"].astype(f32) < minBS
        keep = np.nonzero(~skip)[0]
        n = len(keep)
        u, v, d = rec["u"][keep].astype(f32), rec["v"][keep].astype(f32), depth[keep]
        xyz = np.zeros((n, 8, 3), f32)
        rgb = np.zeros((n, 8, 3), np.uint8)
        for pnt in range(8):
            dx, dy = f32(PATTERN[pnt, 0]), f32(PATTERN[pnt, 1])
            xyz[:, pnt, 0] = ((((u + dx).astype(f32) * fxi).astype(f32) + cxi).astype(f32) * d).astype(f32)
            xyz[:, pnt, 1] = ((((v + dy).astype(f32) * fyi).astype(f32) + cyi).astype(f32) * d).astype(f32)
            if draws is None:
                jit = np.zeros(n, f32)
            else:
                r = np.asarray(draws)[8 * np.arange(n) + pnt]                               # vertexBufferNumPoints when the vertex is written
                jit = ((r.astype(f32) / f32(RAND_MAX)).astype(f32) - f32(0.5)).astype(f32)
            xyz[:, pnt, 2] = (d * (f32(1) + ((f32(2) * fxi).astype(f32) * jit).astype(f32)).astype(f32)).astype(f32)
            if mode == 0:
                s = st[keep]
                rgb[:, pnt, 0] = np.where(s == 3, 255, 0)
                rgb[:, pnt, 1] = np.where((s == 0) | (s == 1), 255, 0)
                rgb[:, pnt, 2] = np.where((s == 0) | (s == 2), 255, 0)
            else:
                rgb[:, pnt, :] = color_byte(rec["color"][keep, pnt])[:, None]
    records = np.bincount(st, minlength=4)[:4]
    survivors = np.bincount(st[keep], minlength=4)[:4]
    return xyz.reshape(-1, 3), rgb.reshape(-1, 3), records, survivors


def world_points(u, v, idepth, calib_inv, m):
    """depth, x, y, z in float; the row sums ((m0*x + m1*y) + m2*z) + m3 in double. m: camToWorld [3][4]"""
    fxi, fyi, cxi, cyi = (f32(x) for x in calib_inv)
    u, v, idepth = np.asarray(u, f32), np.asarray(v, f32), np.asarray(idepth, f32)
    m = np.asarray(m, f64).reshape(3, 4)
    with np.errstate(all="ignore"):
        depth = (f32(1.0) / idepth).astype(f32)
        x = (((u * fxi).astype(f32) + cxi).astype(f32) * depth).astype(f32)
        y = (((v * fyi).astype(f32) + cyi).astype(f32) * depth).astype(f32)
        z = (depth * (f32(1) + (f32(2) * fxi).astype(f32)).astype(f32)).astype(f32)
        x, y, z = x.astype(f64), y.astype(f64), z.astype(f64)
        return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] * f64(1.0) for r in range(3)], 1)


def calib_inverse(K):
    """fxi, fyi, cxi, cyi as floats of the float calibration (KeyFrameDisplay::setFromF :78-86, SampleOutputWrapper.h:89-96)"""
    fx, fy, cx, cy = (f32(k) for k in K)
    return np.array([f32(1) / fx, f32(1) / fy, -cx / fx, -cy / fy], f32)


def bits_equal(a, b):
    """bit for bit, NaN equal to NaN whatever its payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    ia = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    ib = b.view(ia.dtype)
    return bool(np.all((ia == ib) | (np.isnan(a) & np.isnan(b))))


def records_equal(a, b):
    return len(a) == len(b) and all(bits_equal(a[k], b[k]) for k in RECORD.names)
