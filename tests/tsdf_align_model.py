"""The literal model of "The alignment" of the TSDF section of include/nalo_gpu.h over the volume dict of tests/tsdf_model.py, with the field of
tests/tsdf_raycast_model.py: pixel_literal is one pixel exactly as the header reads, records_literal loops it over the visited pixels, records is the same
operations in the same order on whole planes. Everything per pixel in float32, one rounding per operation. sums adds the 37 exact products with math.fsum;
step and align are the Levenberg-Marquardt step and loop in float64. No device."""
import math

import numpy as np

import tsdf_raycast_model as rm

F = np.float32
CONVERGED, ITERATION_LIMIT, TOO_FEW, SOLVE_FAILED = 0, 1, 2, 3
PAIRS = [(i, j) for i in range(7) for j in range(i, 7)]                          # H's upper triangle, row-major


def matrix(cam_to_world, s=1.0):
    """M = [s R | t], formed in double and rounded to float32"""
    c = np.asarray(cam_to_world, np.float64).reshape(3, 4)
    M = np.empty((3, 4), F)
    M[:, :3] = (np.float64(s) * c[:, :3]).astype(F)
    M[:, 3] = c[:, 3].astype(F)
    return M


# ------------------------------------------------------------------------------------------------ the literal form
def pixel_literal(vol, D, u, v, K, M, min_depth, max_depth, min_weight, huber, dof):
    """one visited pixel -> its record [10]: r, hw, J0..J6, state; every field but the state is 0 unless the state is 0"""
    rec = np.zeros(10, F)
    D, mn, mx, mw, hb = F(D), F(min_depth), F(max_depth), F(min_weight), F(huber)
    if not (D >= mn and D <= mx):
        rec[9] = 1
        return rec
    fx, fy, cx, cy = (F(k) for k in K)
    o, vs = vol["origin"], vol["vs"]
    rx, ry = (F(u) - cx) / fx, (F(v) - cy) / fy
    pc = [rx * D, ry * D, D]
    pw = [((M[a, 0] * pc[0] + M[a, 1] * pc[1]) + M[a, 2] * pc[2]) + M[a, 3] for a in range(3)]
    q = [(pw[a] - o[a]) / vs - F(0.5) for a in range(3)]
    ok, S = rm.field_literal(vol, vol["tsdf"], q, mw)
    if not ok:
        rec[9] = 2
        return rec
    G, good = [], True
    for a in range(3):
        qp, qm = list(q), list(q)
        qp[a], qm[a] = q[a] + F(1.0), q[a] - F(1.0)
        okp, sp = rm.field_literal(vol, vol["tsdf"], qp, mw)
        okm, sm = rm.field_literal(vol, vol["tsdf"], qm, mw)
        good = good and okp and okm
        G.append(sp - sm)
    if not good:
        rec[9] = 3
        return rec
    k = F(0.5) / vs
    g = [G[a] * k for a in range(3)]
    J = [g[0], g[1], g[2], pw[1] * g[2] - pw[2] * g[1], pw[2] * g[0] - pw[0] * g[2], pw[0] * g[1] - pw[1] * g[0], F(0.0)]
    if dof == 7:
        J[6] = (g[0] * (pw[0] - M[0, 3]) + g[1] * (pw[1] - M[1, 3])) + g[2] * (pw[2] - M[2, 3])
    hw = F(1.0) if np.abs(S) <= hb else hb / np.abs(S)
    assert all(x.dtype == F for x in J) and hw.dtype == F and S.dtype == F
    rec[0], rec[1], rec[2:9] = S, hw, J
    return rec


def records_literal(vol, depth, K, cam_to_world, s, min_depth, max_depth, min_weight, huber, step, dof, fill=np.nan, pixels=None):
    """[h][w][10], the visited pixels' records; every other word holds `fill`. pixels: a list of (u, v) to evaluate instead of all the visited ones"""
    h, w = depth.shape
    M = matrix(cam_to_world, s)
    out = np.full((h, w, 10), fill, F)
    todo = [(u, v) for v in range(0, h, step) for u in range(0, w, step)] if pixels is None else pixels
    with np.errstate(all="ignore"):
        for u, v in todo:
            assert u % step == 0 and v % step == 0
            out[v, u] = pixel_literal(vol, depth[v, u], u, v, K, M, min_depth, max_depth, min_weight, huber, dof)
    return out


# ------------------------------------------------------------------------------------------------ the same on whole planes
def records(vol, depth, K, cam_to_world, s, min_depth, max_depth, min_weight, huber, step, dof, fill=np.nan):
    """records_literal's operations in its order on the [ceil(h / step)][ceil(w / step)] visited pixels at once"""
    h, w = depth.shape
    M = matrix(cam_to_world, s)
    fx, fy, cx, cy = (F(k) for k in K)
    mn, mx, mw, hb = F(min_depth), F(max_depth), F(min_weight), F(huber)
    o, vs = vol["origin"], vol["vs"]
    out = np.full((h, w, 10), fill, F)
    with np.errstate(all="ignore"):
        vv, uu = np.mgrid[0:h:step, 0:w:step]
        D = np.ascontiguousarray(depth[::step, ::step], F)
        usable = (D >= mn) & (D <= mx)
        rx, ry = (uu.astype(F) - cx) / fx, (vv.astype(F) - cy) / fy
        pc = [rx * D, ry * D, D]
        pw = [((M[a, 0] * pc[0] + M[a, 1] * pc[1]) + M[a, 2] * pc[2]) + M[a, 3] for a in range(3)]
        q = [(pw[a] - o[a]) / vs - F(0.5) for a in range(3)]
        ok, S = rm.field(vol, vol["tsdf"], *q, mw)
        G, good = [], np.ones(D.shape, bool)
        for a in range(3):
            qp, qm = list(q), list(q)
            qp[a], qm[a] = q[a] + F(1.0), q[a] - F(1.0)
            okp, sp = rm.field(vol, vol["tsdf"], *qp, mw)
            okm, sm = rm.field(vol, vol["tsdf"], *qm, mw)
            good &= okp & okm
            G.append(sp - sm)
        state = np.where(~usable, 1, np.where(~ok, 2, np.where(~good, 3, 0)))
        k = F(0.5) / vs
        g = [G[a] * k for a in range(3)]
        J = [g[0], g[1], g[2], pw[1] * g[2] - pw[2] * g[1], pw[2] * g[0] - pw[0] * g[2], pw[0] * g[1] - pw[1] * g[0], np.zeros(D.shape, F)]
        if dof == 7:
            J[6] = (g[0] * (pw[0] - M[0, 3]) + g[1] * (pw[1] - M[1, 3])) + g[2] * (pw[2] - M[2, 3])
        hw = np.where(np.abs(S) <= hb, F(1.0), hb / np.abs(S)).astype(F)
        assert all(x.dtype == F for x in J) and S.dtype == F
        used = state == 0
        rec = np.zeros(D.shape + (10,), F)
        rec[..., 0] = np.where(used, S, F(0.0))
        rec[..., 1] = np.where(used, hw, F(0.0))
        for i in range(7):
            rec[..., 2 + i] = np.where(used, J[i], F(0.0))
        rec[..., 9] = state.astype(F)
        out[::step, ::step] = rec
    return out


# ------------------------------------------------------------------------------------------------ the sums
def terms(rec, huber, step=1):
    """the used pixels' terms of the 37 sums as float64 [n][37], every product exact, and the four state counts"""
    r = np.asarray(rec)[::step, ::step].reshape(-1, 10)
    st = r[:, 9]
    count = tuple(int((st == k).sum()) for k in range(4))
    assert sum(count) == len(r), "a word of the visited pixels holds no state"
    u = r[st == 0].astype(np.float64)
    res, J = u[:, 0], u[:, 2:9]
    Jw = (r[st == 0][:, 1:2] * r[st == 0][:, 2:9]).astype(np.float64)             # hw * J_i, rounded to float32 once
    hb = float(F(huber))
    T = np.empty((len(u), 37))
    for k, (i, j) in enumerate(PAIRS):
        T[:, k] = Jw[:, i] * J[:, j]
    for i in range(7):
        T[:, 28 + i] = Jw[:, i] * res
    a = np.abs(res)
    with np.errstate(all="ignore"):
        T[:, 35] = np.where(a <= hb, res * res, hb * (2.0 * a - hb))
    T[:, 36] = res * res
    return T, count


def sums(rec, huber, step=1):
    """dict(H [28], b [7], E, rr, count, abs [37]: the sums of the terms' magnitudes, for the summation bound) with math.fsum; a sum with a term that is not
    finite is numpy's"""
    T, count = terms(rec, huber, step)
    fs = lambda col: math.fsum(col) if np.isfinite(col).all() else float(np.sum(col))
    with np.errstate(all="ignore"):
        tot = np.array([fs(T[:, k]) for k in range(37)])
        mag = np.array([fs(np.abs(T[:, k])) for k in range(37)])
    return dict(H=tot[:28], b=tot[28:35], E=float(tot[35]), rr=float(tot[36]), count=count, abs=mag)


def gamma(n):
    """gamma_n with u = 2^-53: the worst case of any summation order over n + 1 exact terms is gamma_n * sum |term|"""
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


def full(H28):
    """the symmetric 7 x 7 matrix of the 28 entries"""
    H = np.zeros((7, 7))
    for k, (i, j) in enumerate(PAIRS):
        H[i, j] = H[j, i] = H28[k]
    return H


# ------------------------------------------------------------------------------------------------ the step and the loop, float64
def se3_exp(xi):
    """(upsilon, omega) -> [3][4]: R = exp([omega]x), t = V upsilon"""
    xi = np.asarray(xi, np.float64)
    w = xi[3:6]
    th = np.linalg.norm(w)
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        R, V = np.eye(3) + O + 0.5 * O @ O, np.eye(3) + 0.5 * O
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        R, V = np.eye(3) + A * O + B * O @ O, np.eye(3) + B * O + Cc * O @ O
    return np.hstack([R, (V @ xi[:3])[:, None]])


def step(H28, b, lam, dof, cam_to_world, s):
    """-> (inc [7], camToWorld [3][4], s), or None where the header refuses: a system that is not finite or not positive definite"""
    H, b = full(H28)[:dof, :dof], np.asarray(b, np.float64)[:dof]
    Hl = H + lam * np.diag(np.diag(H))
    if not (np.isfinite(Hl).all() and np.isfinite(b).all()):
        return None
    try:
        np.linalg.cholesky(Hl)
    except np.linalg.LinAlgError:
        return None
    inc = np.zeros(7)
    inc[:dof] = np.linalg.solve(Hl, -b)
    E = se3_exp(inc[:6])
    T = np.asarray(cam_to_world, np.float64).reshape(3, 4)
    out = np.hstack([E[:, :3] @ T[:, :3], (E[:, :3] @ T[:, 3] + E[:, 3])[:, None]])
    return inc, out, float(s) * math.exp(inc[6])


def align(vol, depth, K, cam_to_world, s, min_depth, max_depth, min_weight, huber, step_px, dof, max_iterations, min_used, lambda0, eps):
    """the header's loop -> dict as binding.Context.tsdf_align_depth returns it (without `last`)"""
    need = max(int(min_used), 1)
    ev = lambda T, sc: sums(records(vol, depth, K, T, sc, min_depth, max_depth, min_weight, huber, step_px, dof), huber, step_px)
    T, sc = np.asarray(cam_to_world, np.float64).reshape(3, 4), float(s)
    lam = 0.01 if lambda0 == 0 else float(lambda0)
    S = ev(T, sc)
    trace = [dict(cam_to_world=T, s=sc, lam=lam, E=S["E"], count=S["count"], accepted=True)]
    out = dict(E_first=S["E"], n_first=S["count"][0], iterations=0, status=ITERATION_LIMIT)
    if S["count"][0] < need:
        out["status"] = TOO_FEW
    else:
        for _ in range(max_iterations):
            st = step(S["H"], S["b"], lam, dof, T, sc)
            if st is None:
                out["status"] = SOLVE_FAILED
                break
            out["iterations"] += 1
            inc, Tn, sn = st
            Sn = ev(Tn, sn)
            ok = Sn["count"][0] >= need and Sn["E"] / Sn["count"][0] < S["E"] / S["count"][0]
            trace.append(dict(cam_to_world=Tn, s=sn, lam=lam, E=Sn["E"], count=Sn["count"], accepted=bool(ok)))
            if ok:
                T, sc, S, lam = Tn, sn, Sn, lam * 0.5
            else:
                lam *= 4.0
            if math.sqrt(float(inc @ inc)) <= eps:
                out["status"] = CONVERGED
                break
    out.update(cam_to_world=T, s=sc, evaluations=len(trace), E_last=S["E"], n_last=S["count"][0], trace=trace)
    return out
