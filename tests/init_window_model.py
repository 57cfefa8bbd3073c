"""The literal model of the first window that tests/test_init_window_gpu.py compares nalo_ba_window_from_initializer against:
FullSystem::initializeFromInitializer (reference FullSystem.cpp:1589-1648) and the insertion of the second frame that follows it (makeKeyFrame, :1335-1348).

It is written from those lines, point by point, on what the public read-backs give: the level-0 Pnt arrays u, v, iR (nalo_init_get_points), thisToNext
(nalo_init_get_state), the caller's rand() draws, and - for the points the draws keep - the energyTH of the ImmaturePoint constructor (nalo_imm_create, which the
test calls between select() and window()). Floats are np.float32 scalars in explicit loops, the poses fp64. Nothing here knows about device slots or layouts: the
output is a point list in submission order, which the test hands to nalo_ba_set_points / nalo_ba_set_residuals / nalo_ba_set_point_history."""
import numpy as np

import lifecycle_model as lm

F32 = np.float32
RAND_MAX_F = F32(2147483648.0)                                   # (float)RAND_MAX of a libc whose rand() has 31 bits


def scale(iR):
    """:1589-1595 -> (sumID, numID, rescaleFactor), all float"""
    sumID, numID = F32(1e-5), F32(1e-5)
    for i in range(len(iR)):
        sumID = F32(sumID + F32(iR[i]))
        numID = F32(numID + F32(1))                              # numID++
    rescale = F32(F32(1) / F32(sumID / numID))
    return sumID, numID, rescale


def keep_percentage(density, n):
    """:1598: float / int"""
    return F32(F32(density) / F32(n))


def skipped(draw, keep):
    """:1607: rand() / (float)RAND_MAX > keepPercentage"""
    return bool(F32(F32(int(draw)) / RAND_MAX_F) > keep)


def select(draws, density):
    """the points the draws keep, in index order; every point consumes exactly one draw"""
    n = len(draws)
    keep = keep_percentage(density, n)
    return np.array([i for i in range(n) if not skipped(draws[i], keep)], np.int32).reshape(-1)


def pixel(u, v):
    """:1610: the ImmaturePoint is constructed at (int)(u + 0.5f), (int)(v + 0.5f) (its constructor takes ints)"""
    return int(F32(F32(u) + F32(0.5))), int(F32(F32(v) + F32(0.5)))


def se3_inverse(T):
    """Sophus' inverse of a 3x4 [R | t] in fp64: [R^T | -(R^T t)]"""
    R, t = T[:, :3], T[:, 3]
    Rt = R.T.copy()
    return np.concatenate([Rt, -(Rt @ t)[:, None]], axis=1)


def entering_pose(thisToNext, rescale):
    """:1631-1646: firstToNew = thisToNext with translation() /= rescaleFactor (a float, promoted); camToWorld = firstToNew.inverse();
    worldToCam_evalPT = camToWorld.inverse()"""
    T = np.array(thisToNext, np.float64).reshape(3, 4).copy()
    T[:, 3] = T[:, 3] / np.float64(rescale)
    return se3_inverse(se3_inverse(T))


def window(u, v, iR, sel, energyTH, thisToNext):
    """sel = select(draws, density); energyTH [len(sel)] of the constructor at pixel(u, v) of those points.
    -> dict(src [P] level-0 indices, host, u, v, idepth (= idepth_zero), has_prior, exists [P][2], hist = (numGood, last_target, last_state), rejected,
            scale = (sumID, numID, rescaleFactor), poses [2][3][4] worldToCam_evalPT; state = state_zero = 0 for both frames)"""
    sumID, numID, rescale = scale(iR)
    src, uu, vv, idepth = [], [], [], []
    rejected = 0
    for k, i in enumerate(sel):
        if not np.isfinite(energyTH[k]):                         # :1612 (and :1618: the PointHessian copies the same energyTH)
            rejected += 1
            continue
        ui, vi = pixel(u[i], v[i])
        src.append(int(i)); uu.append(F32(ui)); vv.append(F32(vi))
        idepth.append(F32(F32(iR[i]) * rescale))                 # setIdepthScaled(iR * rescaleFactor); setIdepthZero(idepth): SCALE_IDEPTH = 1
    P = len(src)
    # the insertion of newFrame (:1335-1348): one residual per point to frame 1; lastResiduals, value-initialised to {(0, IN), (0, IN)} by PointHessian (it has
    # no initialiser for the pair, ResState(0) = IN), is shifted: [1] = [0] = (null, IN), [0] = (the new residual, IN)
    exists = np.zeros((P, 2), np.uint8)
    exists[:, 1] = 1
    hist = (np.zeros(P, np.int32), np.tile(np.array([1, -1], np.int8), (P, 1)), np.full((P, 2), lm.IN, np.int8))
    poses = np.stack([np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), entering_pose(thisToNext, rescale)])
    return dict(src=np.array(src, np.int32).reshape(-1), host=np.zeros(P, np.int32), u=np.array(uu, np.float32).reshape(-1), v=np.array(vv, np.float32).reshape(-1),
                idepth=np.array(idepth, np.float32).reshape(-1), has_prior=np.ones(P, np.int32), exists=exists, hist=hist, rejected=rejected,
                scale=(sumID, numID, rescale), poses=poses)


def pairwise_sum(iR):
    """what a tree reduction gives: float adds over halves (the order test 2 must tell from the sequential one)"""
    a = np.concatenate([[F32(1e-5)], np.asarray(iR, np.float32)]).astype(np.float32)
    while len(a) > 1:
        if len(a) % 2:
            a = np.concatenate([a, [F32(0)]]).astype(np.float32)
        a = (a[0::2] + a[1::2]).astype(np.float32)
    return F32(a[0])


def fp64_sum(iR):
    """summed in fp64, rounded once"""
    return F32(np.float64(F32(1e-5)) + np.asarray(iR, np.float64).sum())
