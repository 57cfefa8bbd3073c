"""The literal model of the point lifecycle that tests/test_point_lifecycle_gpu.py compares the device against: PointHessian::isOOB / isInlierNew (reference
HessianBlocks.h:484-514), FullSystem::flagPointsForRemoval (FullSystem.cpp:937-1031) with removeOutliers' predicate (FullSystemOptimize.cpp:631-653), and the
bookkeeping of numGoodResiduals / lastResiduals in linearizeAll(true) (FullSystemOptimize.cpp:52-87, 169-205), at keyframe insertion (FullSystem.cpp:1344-1345)
and in marginalizeFrame (FullSystemMarginalize.cpp:174-177).

The functions are the reference's, statement by statement, on what the public read-backs give: residual states [P][W] (-1 = no residual), the point sums of
the last accumulation, the prior flag. lastResiduals[k] is (window index of the frame .first targets or -1 for a null pointer, .second). A pointer to a residual
that has been deleted compares unequal to every live residual, which is what -1 does: it is written as -1. Nothing here is vectorised over the rules."""
import numpy as np

IN, OOB, OUTLIER = 0, 1, 2
KEEP, DROP_NORES, DROP, MARGINALIZE = 0, 1, 2, 3
MIN_GOOD_ACTIVE_RES_FOR_MARG = 3            # setting_minGoodActiveResForMarg (settings.cpp:115)
MIN_GOOD_RES_FOR_MARG = 4                   # setting_minGoodResForMarg (settings.cpp:116)
MIN_IDEPTH_H_MARG = np.float32(50)          # setting_minIdepthH_marg (settings.cpp:77)
IDEPTH_FIX_PRIOR = np.float32(50 * 50)      # setting_idepthFixPrior (settings.cpp:60); priorF = it * SCALE_IDEPTH^2 (EnergyFunctionalStructs.cpp:79-85), SCALE_IDEPTH = 1
SCALE_IDEPTH = np.float32(1)
f32 = np.float32


def is_oob(res_state, to_marg, num_good, last_state):
    """PointHessian::isOOB. res_state: the states of the point's residuals by target ([W], -1 = none); to_marg: window indices of the flagged frames"""
    vis_in_to_marg = 0
    n = 0
    for t, s in enumerate(res_state):
        if s < 0:
            continue
        n += 1
        if s != IN:
            continue
        for k in to_marg:
            if t == k:
                vis_in_to_marg += 1
    if n >= MIN_GOOD_ACTIVE_RES_FOR_MARG and num_good > MIN_GOOD_RES_FOR_MARG + 10 and n - vis_in_to_marg < MIN_GOOD_ACTIVE_RES_FOR_MARG:
        return True, 1
    if last_state[0] == OOB:
        return True, 2
    if n < 2:
        return False, 3
    if last_state[0] == OUTLIER and last_state[1] == OUTLIER:
        return True, 4
    return False, 0


def is_inlier_new(n_res, num_good):
    """PointHessian::isInlierNew"""
    return n_res >= MIN_GOOD_ACTIVE_RES_FOR_MARG and num_good >= MIN_GOOD_RES_FOR_MARG


def idepth_hessian(Hdd_accAF, HdiF, has_prior):
    """the float H of AccumulatedSCHessianSSE::addPoint (AccumulatedSCHessian.cpp:36-50) from the stored addends: one float add, the floor, 0 when the point had
    no active residual at that accumulation (HdiF = 0)"""
    prior = np.where(np.asarray(has_prior).astype(bool), IDEPTH_FIX_PRIOR * SCALE_IDEPTH * SCALE_IDEPTH, f32(0)).astype(f32)
    H = np.asarray(Hdd_accAF, f32) + prior
    H = np.where(H < f32(1e-10), f32(1e-10), H).astype(f32)
    return np.where(np.asarray(HdiF, f32) == 0, f32(0), H).astype(f32)


def flag_point(res_state, idepth, H, host_flagged, to_marg, num_good, last_state):
    """one point of flagPointsForRemoval -> (decision, the isOOB clause that fired: 1..4, 0 = none, -1 = not reached)"""
    n = int(sum(1 for s in res_state if s >= 0))
    if SCALE_IDEPTH * f32(idepth) < 0 or n == 0:
        return DROP_NORES, -1
    oob, clause = is_oob(res_state, to_marg, num_good, last_state)
    if oob or host_flagged:
        if is_inlier_new(n, num_good):
            if f32(H) > MIN_IDEPTH_H_MARG:
                return MARGINALIZE, clause
            return DROP, clause
        return DROP, clause
    return KEEP, clause


def flag_points(host, res_state, idepth, H, frame_flagged, num_good, last_state, valid=None):
    """-> decision [P], counts [W][4] = {kept, drop_nores, drop, marginalised} per host, clause [P], reached_H [P] (the point got as far as the test on H)"""
    P, W = res_state.shape
    to_marg = [i for i in range(W) if frame_flagged[i]]
    dec = np.zeros(P, np.uint8)
    clause = np.full(P, -1, np.int8)
    reached = np.zeros(P, bool)
    counts = np.zeros((W, 4), np.int32)
    rs, ng, ls = res_state.tolist(), np.asarray(num_good).tolist(), np.asarray(last_state).tolist()
    for p in range(P):
        if valid is not None and not valid[p]:
            continue
        h = int(host[p])
        d, c = flag_point(rs[p], idepth[p], H[p], bool(frame_flagged[h]), to_marg, ng[p], ls[p])
        dec[p], clause[p] = d, c
        counts[h, d] += 1
        reached[p] = d != DROP_NORES and (c in (1, 2, 4) or bool(frame_flagged[h])) and is_inlier_new(sum(1 for s in rs[p] if s >= 0), ng[p])
    return dec, counts, clause, reached


def removed_states(st_nofix, st_pre, st_post):
    """state_state of the residuals a linearizeAll(true) removed, from the passes around it: st_nofix = the states after a linearizeAll(false) at the same
    geometry, st_pre / st_post = before / after the fix pass. A removed residual that was OOB after the first pass is OOB (geometry did not move and OOB is
    sticky, Residuals.cpp:82-83), any other one is OUTLIER. -> [P][W], -1 where nothing was removed"""
    removed = (st_pre >= 0) & (st_post < 0)
    return np.where(removed, np.where(st_nofix == OOB, OOB, OUTLIER), -1).astype(np.int8)


def history_update(num_good, last_target, last_state, st_pre, st_post, active_post, removed_state):
    """linearizeAll(true): st_pre >= 0 marks the residuals that took part, st_post / active_post their state and isActive() after applyRes for the survivors,
    removed_state the state_state of the removed ones"""
    ng, lt, ls = np.array(num_good, np.int64), np.array(last_target, np.int8), np.array(last_state, np.int8)
    P, W = st_pre.shape
    for p in range(P):
        to_remove = []
        for t in range(W):                                       # linearizeAll_Reductor
            if st_pre[p, t] < 0:
                continue
            if st_post[p, t] >= 0 and active_post[p, t]:
                ng[p] += 1                                       # isNew is never cleared (Residuals.cpp:72)
            else:
                to_remove.append(t)
        for t in range(W):                                       # :172-179
            if st_pre[p, t] < 0:
                continue
            state = st_post[p, t] if st_post[p, t] >= 0 else removed_state[p, t]
            if lt[p, 0] == t:
                ls[p, 0] = state
            elif lt[p, 1] == t:
                ls[p, 1] = state
        for t in to_remove:                                      # :187-194 (a deleted residual's pointer: -1, see the module text)
            assert st_post[p, t] < 0, "a residual that is not active after a fix pass is removed"
            if lt[p, 0] == t:
                lt[p, 0] = -1
            if lt[p, 1] == t:
                lt[p, 1] = -1
    return ng, lt, ls


def default_history(exists):
    """what optimizeImmaturePoint leaves on a freshly activated point (FullSystemOptPoint.cpp:173-199)"""
    P, W = exists.shape
    lt, ls = np.full((P, 2), -1, np.int8), np.full((P, 2), OOB, np.int8)
    for k, t in ((0, W - 1), (1, W - 2)):
        m = exists[:, t] != 0
        lt[m, k], ls[m, k] = t, IN
    return np.zeros(P, np.int32), lt, ls


def shift_at_insertion(last_target, last_state, gets_residual, new_index):
    """FullSystem.cpp:1344-1345 for the points that get a residual to the new keyframe (window index new_index)"""
    lt, ls = np.array(last_target, np.int8), np.array(last_state, np.int8)
    m = np.asarray(gets_residual, bool)
    lt[m, 1], ls[m, 1] = lt[m, 0], ls[m, 0]
    lt[m, 0], ls[m, 0] = new_index, IN
    return lt, ls


def remap_at_frame_marginalization(last_target, idx):
    """FullSystemMarginalize.cpp:174-177 in window indices: the residuals to frame idx are deleted, the frames behind it move one down"""
    lt = np.array(last_target, np.int8)
    lt[lt == idx] = -1
    lt[lt > idx] -= 1
    return lt
