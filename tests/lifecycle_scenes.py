"""The windows, planted histories and the model side of the step-API route that tests/test_point_lifecycle_gpu.py runs on the device and
tests/test_point_lifecycle_cpu.py runs on the fp32 oracle (the coverage of the scenes is checked there, without a device).

Scenes: the synthetic corridor at the project's window shapes, but with a LOW-PARALLAX trajectory (baselines of a fraction of a millimetre per keyframe, against
wall and ground 2-40 m away): Hdd = sum JIdx2 Jpdd^2 then spreads over both sides of setting_minIdepthH_marg = 50, where the stock trajectory (0.8 m per keyframe)
puts every H above 1e7. A third of the residual graph is missing (nres 0..W-1), 2 % of the points carry a negative inverse depth, 1 % no residual at all, the points
of host 0 the depth prior of the initialiser; the pose perturbation makes about a third of the residuals outliers, so every fix pass removes thousands."""
import dataclasses

import numpy as np

import lifecycle_model as lm
from nalo_slam_amd import synth

SCENES = {
    # min_points: what every class / clause must be reached by; the fp32 oracle gives the KITTI-shaped scene 152 points for its rarest clause (isOOB's first), the
    # W = 16 scene 111; the 250 k-point window is the KITTI-shaped scene 125 times over
    "kitti": dict(w=1224, h=368, W=8, P=2000, scale=3e-4, min_points=100),
    "w12": dict(w=640, h=480, W=12, P=6000, scale=1.5e-4, min_points=50),
    "w16": dict(w=640, h=480, W=16, P=8000, scale=1.5e-4, min_points=50),
    "stress250k": dict(w=1920, h=1072, W=8, P=250000, scale=3e-4, min_points=5000),
}
SEED = 7


def make_scene(name, every=1):
    """every > 1: the scene's points thinned to one in `every` (the same frames and trajectory)"""
    s = SCENES[name]
    win = synth.make_window(w=s["w"], h=s["h"], W=s["W"], P=s["P"], seed=SEED, n_extra=0, step_z=0.8 * s["scale"], step_x=0.03 * s["scale"], full_graph=False)
    if every > 1:
        idx = np.arange(0, len(win.host), every)
        win = dataclasses.replace(win, host=win.host[idx], u=win.u[idx], v=win.v[idx], idepth=win.idepth[idx], idepth_true=win.idepth_true[idx],
                                  color=win.color[idx], weights=win.weights[idx], exists=win.exists[idx])
    rng = np.random.RandomState(SEED + 1)
    P = len(win.host)
    idepth = win.idepth.copy()
    neg = rng.rand(P) < 0.02
    idepth[neg] = -idepth[neg]
    exists = win.exists.copy()
    exists[rng.rand(P) < 0.01] = 0
    win = dataclasses.replace(win, idepth=idepth, exists=exists)
    st6 = synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)
    has_prior = (win.host == 0).astype(np.int32)
    return win, st6, has_prior


def flag_sets(W):
    """0, 1 and 2 flagged frames: a host of points, then that host and the second-newest frame"""
    one = np.zeros(W, np.uint8); one[1] = 1
    two = one.copy(); two[W - 2] = 1
    return [np.zeros(W, np.uint8), one, two]


def plant_history(P, W, seed=SEED + 2):
    """numGood over 0..20, all nine last_state pairs, targets over the whole window with a third of them null"""
    rng = np.random.RandomState(seed)
    ng = rng.randint(0, 21, P).astype(np.int32)
    ls = np.stack([np.arange(P) % 3, (np.arange(P) // 3) % 3], 1).astype(np.int8)
    ls = ls[rng.permutation(P)]
    lt = rng.randint(0, W, (P, 2)).astype(np.int8)
    lt[rng.rand(P, 2) < 1.0 / 3] = -1
    half = rng.rand(P) < 0.5                                      # half of the points keep the pointers a running system has: the two newest frames
    lt[half, 0] = np.where(lt[half, 0] >= 0, W - 1, -1)
    lt[half, 1] = np.where(lt[half, 1] >= 0, W - 2, -1)
    return ng, lt, ls


def model_route(win, has_prior, planted, st1, st2, ac2, pts):
    """the model's side of: plant, linearizeAll(false) -> st1, linearizeAll(true) -> st2 / ac2, accumulate -> pts, flagPointsForRemoval for flag_sets"""
    W = win.W
    removed = lm.removed_states(st1, st1, st2)
    ng, lt, ls = lm.history_update(planted[0], planted[1], planted[2], st1, st2, ac2, removed)
    H = lm.idepth_hessian(pts["Hdd"], pts["HdiF"], has_prior)
    out = dict(ng=ng, lt=lt, ls=ls, H=H, removed=removed, flags=[])
    for ff in flag_sets(W):
        dec, counts, clause, reached = lm.flag_points(win.host, st2, pts["idepth"], H, ff, ng, ls)
        out["flags"].append(dict(ff=ff, dec=dec, counts=counts, clause=clause, reached=reached))
    return out


def assert_coverage(name, m, every=1):
    """every class, every clause of isOOB and both sides of H = 50 are reached, over the three flag sets, by the scene's stated minimum of points
    (divided by `every` for a thinned scene)"""
    n_min = SCENES[name]["min_points"] // every
    dec = np.concatenate([f["dec"] for f in m["flags"]])
    clause = np.concatenate([f["clause"] for f in m["flags"]])
    for d in (lm.KEEP, lm.DROP_NORES, lm.DROP, lm.MARGINALIZE):
        assert (dec == d).sum() >= n_min, (name, "decision", d, int((dec == d).sum()))
    for c in (0, 1, 2, 3, 4):
        assert (clause == c).sum() >= n_min, (name, "clause", c, int((clause == c).sum()))
    for f in m["flags"]:
        r = f["reached"]
        assert r.sum() >= n_min
        above = (m["H"][r] > lm.MIN_IDEPTH_H_MARG).mean()
        assert 0.05 <= above <= 0.95, (name, above)
    removed = (m["removed"] >= 0).sum()
    assert removed >= n_min and (m["removed"] == lm.OOB).sum() >= 1 and (m["removed"] == lm.OUTLIER).sum() >= n_min
    assert (m["lt"] >= 8).sum() >= n_min or name in ("kitti", "stress250k")      # W = 16: targets beyond the 3-bit range


REPLICAS = 20


def plant_cases(cases):
    """The hand-built points of tests/test_point_lifecycle_cpu.py in a real window: REPLICAS copies of every case, each on a point of the case's host frame of a
    4000-point KITTI-shaped scene, with the case's residual pattern, sign of the inverse depth, numGood and lastResiduals states (null pointers, so that no pass
    rewrites them). What a real window decides itself - which residuals are IN, and H - is read back; a replica REALISES its case when nres, visInToMarg, the
    sign of idepth and (where the decision gets that far) the side of H are the case's, and then the device must take the decision of the table. -> win, st6, has_prior, history, rows [(case, point)]"""
    s = dict(SCENES["kitti"], P=4000)
    win = synth.make_window(w=s["w"], h=s["h"], W=s["W"], P=s["P"], seed=SEED, n_extra=0, step_z=0.8 * s["scale"], step_x=0.03 * s["scale"], full_graph=False)
    P = len(win.host)
    idepth, exists = np.abs(win.idepth), win.exists.copy()
    ng, lt, ls = plant_history(P, win.W)
    rows, used = [], {h: 0 for h in range(win.W)}
    for ci, c in enumerate(cases):
        cand = np.nonzero(win.host == c["host"])[0]
        for _ in range(REPLICAS):
            p = cand[used[c["host"]]]
            used[c["host"]] += 1
            exists[p] = [1 if x >= 0 else 0 for x in c["res"]]
            assert exists[p, c["host"]] == 0
            if c["idepth"] < 0:
                idepth[p] = -idepth[p]
            ng[p], ls[p], lt[p] = c["ng"], c["ls"], (-1, -1)
            rows.append((ci, int(p)))
    win = dataclasses.replace(win, idepth=idepth.astype(np.float32), exists=exists)
    return win, synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004), np.zeros(P, np.int32), (ng, lt, ls), rows


def realised(case, st_row, H, idepth):
    """does a point with these read-backs realise the case (see plant_cases)? The side of H counts where the decision reaches the test on H"""
    def sig(res, idv):
        return sum(1 for x in res if x >= 0), sum(1 for t, x in enumerate(res) if x == lm.IN and t in case["flagged"]), idv < 0
    if sig(case["res"], case["idepth"]) != sig(list(st_row), idepth):
        return False
    d = [lm.flag_point(list(st_row), idepth, h, case["host"] in case["flagged"], case["flagged"], case["ng"], case["ls"])[0] for h in (0.0, 1e9)]
    return d[0] == d[1] or bool(np.float32(H) > lm.MIN_IDEPTH_H_MARG) == bool(np.float32(case["H"]) > lm.MIN_IDEPTH_H_MARG)
