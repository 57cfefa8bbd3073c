"""Inputs for the immature-point tests (shared by the CPU oracle test and the GPU parity test)."""
import numpy as np

from nalo_slam_amd import synth


def imm_points(win, per_host=1000, seed=1, margin=8):
    """integer pixel positions (PixelSelector output) for every host frame of the window -> u, v (int32), host (int32)"""
    rng = np.random.RandomState(seed)
    u, v, host = [], [], []
    for h in range(win.W):
        u.append(rng.randint(margin, win.w - margin, per_host))
        v.append(rng.randint(margin, win.h - margin, per_host))
        host.append(np.full(per_host, h))
    u, v, host = np.concatenate(u).astype(np.int32), np.concatenate(v).astype(np.int32), np.concatenate(host).astype(np.int32)
    ok = np.isfinite(win.depth[host, v, u]) if isinstance(win.depth, np.ndarray) else np.array([np.isfinite(win.depth[h][y, x]) for h, y, x in zip(host, v, u)])
    return u[ok], v[ok], host[ok]


def host_to_new(win, new, aff=None, exposure=None):
    """what FullSystem::traceNewCoarse computes per host (FullSystem.cpp:713-721): KRKi [W,9], Kt [W,3], affine pair [W,2]. Without aff / exposure the
    brightness is the identity [1, 0]; with them (per frame of the window and its extras: aff [F,2] = (a, b), exposure [F]) the pair is
    AffLight::fromToVecExposure(e_h, e_new, aff_h, aff_new) = (exp(a_new - a_h) e_new / e_h, b_new - a_ht b_h), in fp64, cast to fp32 once."""
    fx, fy, cx, cy = win.K
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    Ki = np.linalg.inv(K)
    KRKi, Kt, pair = [], [], []
    for h in range(win.W):
        T = synth.se3_mul(win.world_to_cam[new], synth.se3_inv(win.world_to_cam[h]))
        KRKi.append((K @ T[:, :3] @ Ki).reshape(-1)); Kt.append(K @ T[:, 3])
        if aff is None and exposure is None:
            pair.append([1.0, 0.0])
            continue
        ah, bh = (0.0, 0.0) if aff is None else (float(aff[h][0]), float(aff[h][1]))
        an, bn = (0.0, 0.0) if aff is None else (float(aff[new][0]), float(aff[new][1]))
        eh, en = (1.0, 1.0) if exposure is None else (float(np.float32(exposure[h])), float(np.float32(exposure[new])))      # ab_exposure is a float
        if eh == 0 or en == 0:
            eh = en = 1.0
        a = np.exp(an - ah) * en / eh
        pair.append([a, bn - a * bh])
    return np.asarray(KRKi, np.float32), np.asarray(Kt, np.float32), np.asarray(pair, np.float64).astype(np.float32)


def true_idepth(win, u, v, host):
    return np.array([1.0 / win.depth[h][y, x] for h, y, x in zip(host, v, u)], np.float32)
