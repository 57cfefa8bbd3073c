"""The literal model of the seam between two keyframes that tests/test_ba_carry_gpu.py compares nalo_ba_carry_window against: which points, residuals and
history entries a window holds after frames left it (FullSystem::marginalizeFrame, reference FullSystemMarginalize.cpp:155-212), after a keyframe entered
(FullSystem.cpp:1335-1348: a residual from every active point to the new frame, the shift of lastResiduals) and after step 4 of activatePointsMT
(FullSystem.cpp:893-917) with the tail of optimizeImmaturePoint (FullSystemOptPoint.cpp:170-200).

It is written from those lines, point by point, on what the public read-backs give: the points' hosts and validity, the residual states [P][W] (-1 = no
residual), the history of tests/lifecycle_model.py (lastResiduals[k] = (window index or -1, state)). Nothing here knows about device slots or layouts: the
output is a point list in submission order, which the test hands to nalo_ba_set_points / nalo_ba_set_residuals / nalo_ba_set_point_history."""
import numpy as np

import lifecycle_model as lm


def carry(host, valid, res_state, hist, rows, entering):
    """The window re-issued for the frames that remain.
    host [P], res_state [P][W_old] in the indices of the window the points were issued for; valid [P]; hist = (numGood, last_target, last_state) or None, its targets
    ALREADY in the indices of the remaining frames (every marginalizeFrame remapped them, FullSystemMarginalize.cpp:174-177); rows[t_new] = the old index of the
    frame that is t_new now; entering: one more frame is appended as the newest.
    -> dict(old_p [P_new], host [P_new] (new indices), exists [P_new][W_new], hist or None)"""
    P, W_rem = len(host), len(rows)
    W_new = W_rem + (1 if entering else 0)
    new_of_old = {int(r): t for t, r in enumerate(rows)}
    old_p, nhost, exists = [], [], []
    ng, lt, ls = [], [], []
    for p in range(P):
        if not valid[p]:
            continue                                             # removed points are gone (dropPointsF / marginalizePointsF)
        assert int(host[p]) in new_of_old, "marginalizeFrame asserts that the frame hosts no point (EnergyFunctional.cpp:505)"
        row = [0] * W_new
        for t_new, r in enumerate(rows):                         # a residual survives iff its target does (FullSystemMarginalize.cpp:161-199)
            row[t_new] = 1 if res_state[p][r] >= 0 else 0
        if entering:
            row[W_new - 1] = 1                                   # FullSystem.cpp:1340-1343
        old_p.append(p); nhost.append(new_of_old[int(host[p])]); exists.append(row)
        if hist is not None:
            g, t, s = int(hist[0][p]), [int(x) for x in hist[1][p]], [int(x) for x in hist[2][p]]
            if entering:                                         # :1344-1345
                t[1], s[1] = t[0], s[0]
                t[0], s[0] = W_new - 1, lm.IN
            ng.append(g); lt.append(t); ls.append(s)
    out = dict(old_p=np.array(old_p, np.int32).reshape(-1), host=np.array(nhost, np.int32).reshape(-1), exists=np.array(exists, np.uint8).reshape(-1, W_new), hist=None)
    if hist is not None:
        out["hist"] = (np.array(ng, np.int32).reshape(-1), np.array(lt, np.int8).reshape(-1, 2), np.array(ls, np.int8).reshape(-1, 2))
    return out


def insert(win, result, res_in, imm_host, sel):
    """Step 4 of activatePointsMT on a window `win` (a dict as carry() returns it): every selected point k whose optimizeImmaturePoint returned a PointHessian
    (result[k] == 1; 0 = the null pointer, -1 = the (PointHessian*)-1 of a point to delete) is pushed behind the points of the window, in toOptimize order, with
    the residuals that ended IN (res_in[k][t]) and a fresh PointHessian's history.
    -> dict like carry()'s, old_p = -(k + 1) for an inserted point, plus from_k [P_new] (-1 for a carried point)"""
    W = win["exists"].shape[1]
    old_p, host, exists = list(win["old_p"]), list(win["host"]), [list(r) for r in win["exists"]]
    from_k = [-1] * len(old_p)
    hist = win["hist"]
    ng, lt, ls = ([list(x) for x in (hist[0], hist[1].tolist(), hist[2].tolist())] if hist is not None else (None, None, None))
    for k in range(len(sel)):
        if result[k] != 1:
            continue                                             # FullSystem.cpp:896: newpoint != 0 && newpoint != (PointHessian*)-1
        row = [1 if res_in[k][t] else 0 for t in range(W)]       # FullSystemOptPoint.cpp:181-189
        old_p.append(-(k + 1)); host.append(int(imm_host[sel[k]])); exists.append(row); from_k.append(k)
        if hist is not None:
            t2, s2 = [-1, -1], [lm.OOB, lm.OOB]                  # :173-176
            if row[W - 1]:
                t2[0], s2[0] = W - 1, lm.IN                      # :190-194 (frameHessians.back())
            if W >= 2 and row[W - 2]:
                t2[1], s2[1] = W - 2, lm.IN                      # :195-199
            ng.append(0); lt.append(t2); ls.append(s2)
    out = dict(old_p=np.array(old_p, np.int32).reshape(-1), host=np.array(host, np.int32).reshape(-1), exists=np.array(exists, np.uint8).reshape(-1, W),
               from_k=np.array(from_k, np.int32).reshape(-1), hist=None)
    if hist is not None:
        out["hist"] = (np.array(ng, np.int32).reshape(-1), np.array(lt, np.int8).reshape(-1, 2), np.array(ls, np.int8).reshape(-1, 2))
    return out


def extend_prior(HM, bM):
    """EnergyFunctional::insertFrame on the prior (EnergyFunctional.cpp:437-442): conservativeResize by one frame, the new rows / columns zero"""
    n = HM.shape[0]
    H2, b2 = np.zeros((n + 8, n + 8)), np.zeros(n + 8)
    H2[:n, :n], b2[:n] = HM, bM
    return H2, b2
