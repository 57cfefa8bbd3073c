"""FullSystem::trackNewCoarse's hypothesis loop (FullSystem.cpp:595-666) and its hypothesis list (:535-579) as plain numpy fp64: the model nalo_trk_track_tries
and nalo_trk_motion_tries are tested against.

track_new_coarse() runs the literal loop over ANY callable track(T0, aff0, min_res) -> (ok, T, aff, lastRes, flow): a scripted tracker (the hand-worked cases
of test_track_tries_cpu.py), the fp32 oracle (orc.Tracker.track) or nalo_trk_track on a twin context (the bit contract of test_track_tries_gpu.py)."""
import numpy as np


def finite_as_float(x):
    """std::isfinite((float)x): a double beyond FLT_MAX is not finite as a float"""
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.isfinite(np.float32(x)))


def track_new_coarse(track, tries, aff_init, last_coarse_rmse0, retrack_threshold=1.5):
    """The loop of :595-666. Returns a dict: T, aff, flow, achievedRes (= the new lastCoarseRMSE, :666), have_one_good, try_iterations, winner (-1: none) and
    records, one dict per try that ran: ok, taken, abort_lvl, lastResiduals, flow, T, aff (T / aff: what the callable returned, i.e. the try's input when
    it stopped on min_res) and whatever else the callable returned after its first five values, under 'extra'."""
    tries = np.asarray(tries, np.float64).reshape(-1, 3, 4)
    assert len(tries) >= 1                                        # the reference indexes tries[0] (:663)
    thr = float(last_coarse_rmse0) * float(np.float32(retrack_threshold))       # lastCoarseRMSE[0] * setting_reTrackThreshold: double * float
    achieved = np.full(5, np.nan)
    have, winner = False, -1
    T, aff, flow = tries[0].copy(), np.array(aff_init, np.float64), np.zeros(3)   # :658-664, what stays when no try is good
    records = []
    for i, T_try in enumerate(tries):
        out = track(T_try.copy(), np.array(aff_init, np.float64), achieved.copy())
        ok, T_i, aff_i, lr, fl = out[:5]
        lr, fl = np.asarray(lr, np.float64), np.asarray(fl, np.float64)
        abort_lvl = -1                                            # CoarseTracker.cpp:1227: the first level of the descent whose residual exceeds 1.5 x the bound
        if not ok:
            for l in range(4, -1, -1):
                if lr[l] > 1.5 * achieved[l]:
                    abort_lvl = l
                    break
        taken = bool(ok) and finite_as_float(lr[0]) and not (lr[0] >= achieved[0])     # :633
        if taken:
            T, aff, flow, have, winner = np.array(T_i, np.float64).reshape(3, 4), np.array(aff_i, np.float64), fl.copy(), True, i
        if have:                                                  # :643-650
            for l in range(5):
                if not finite_as_float(achieved[l]) or achieved[l] > lr[l]:
                    achieved[l] = lr[l]
        records.append(dict(ok=int(bool(ok)), taken=int(taken), abort_lvl=abort_lvl, lastResiduals=lr.copy(), flow=fl.copy(),
                            T=np.array(T_i, np.float64).reshape(3, 4), aff=np.array(aff_i, np.float64), extra=tuple(out[5:])))
        if have and achieved[0] < thr:                            # :653, strict
            break
    return dict(T=T, aff=aff, flow=flow, achievedRes=achieved, have_one_good=int(have), try_iterations=len(records), winner=winner, records=records)


# ---- SE(3) as 3x4 [R|t], fp64
def se3_mul(A, B):
    A, B = np.asarray(A, np.float64).reshape(3, 4), np.asarray(B, np.float64).reshape(3, 4)
    return np.hstack([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]])


def se3_inv(A):
    A = np.asarray(A, np.float64).reshape(3, 4)
    return np.hstack([A[:, :3].T, (-A[:, :3].T @ A[:, 3])[:, None]])


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def se3_exp(xi):
    """(upsilon, omega) -> [R|t], Rodrigues and the closed-form V"""
    xi = np.asarray(xi, np.float64)
    w, th = xi[3:], np.linalg.norm(xi[3:])
    O = _hat(w)
    if th < 1e-10:
        R, V = np.eye(3) + O, np.eye(3) + 0.5 * O
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        R, V = np.eye(3) + a * O + b * O @ O, np.eye(3) + b * O + c * O @ O
    return np.hstack([R, (V @ xi[:3])[:, None]])


def se3_log(T):
    T = np.asarray(T, np.float64).reshape(3, 4)
    R = T[:, :3]
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    w = 0.5 * v if th < 1e-10 else th / (2 * np.sin(th)) * v       # rotations well below pi, which is all the hypothesis list needs
    O = _hat(w)
    if th < 1e-10:
        Vi = np.eye(3) - 0.5 * O
    else:
        Vi = np.eye(3) - 0.5 * O + (1 - th / (2 * np.tan(th / 2))) / th ** 2 * O @ O
    return np.concatenate([Vi @ T[:, 3], w])


def quat_rotation(w, x, y, z):
    """Sophus' SO3(Quaterniond) normalises, then Eigen's toRotationMatrix"""
    q = np.array([w, x, y, z], np.float64)
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# the sign patterns of :547-572, in the reference's order
ROT_SIGNS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (-1, 1, 0), (0, -1, 1), (-1, 0, 1),
             (1, -1, 0), (0, 1, -1), (1, 0, -1), (-1, -1, 0), (0, -1, -1), (-1, 0, -1), (-1, -1, -1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1),
             (1, -1, -1), (1, -1, 1), (1, 1, -1), (1, 1, 1)]
ROT_DELTA = float(np.float32(0.02))                               # `float rotDelta = 0.02`; the loop's rotDelta++ ends it after one pass


def motion_tries(slast_2_sprelast, lastF_2_slast, poses_valid=True):
    """lastF_2_fh_tries of :535-579 as [n, 3, 4]"""
    if not poses_valid:
        return np.hstack([np.eye(3), np.zeros((3, 1))])[None].copy()
    fh_2_slast = np.asarray(slast_2_sprelast, np.float64).reshape(3, 4)
    lastF = np.asarray(lastF_2_slast, np.float64).reshape(3, 4)
    inv = se3_inv(fh_2_slast)
    constant = se3_mul(inv, lastF)
    out = [constant, se3_mul(se3_mul(inv, inv), lastF), se3_mul(se3_inv(se3_exp(0.5 * se3_log(fh_2_slast))), lastF), lastF.copy(),
           np.hstack([np.eye(3), np.zeros((3, 1))])]
    for s in ROT_SIGNS:
        Rq = np.hstack([quat_rotation(1.0, s[0] * ROT_DELTA, s[1] * ROT_DELTA, s[2] * ROT_DELTA), np.zeros((3, 1))])
        out.append(se3_mul(constant, Rq))
    return np.array(out)
