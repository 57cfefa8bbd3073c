"""nalo_trk_fit_ground (include/nalo_gpu.h): the ground choice of setCoarseTrackingRef (reference src/FullSystem/CoarseTracker.cpp:582-625), the marking of the
window points on it (:669-693) and the chain down to nalo_ba_plane_scale_fix, against tests/ground_model.py - bit for bit.

The model scores with the planes of the DEVICE's records: a refined plane is held to a tolerance only (test_plane_fit_gpu.py), and mid_z, score, winner and
gp_raw are compared exactly here. Clusters, member order and the cloud's Z come from the model (tests/plane_model.py)."""
import ctypes as C

import numpy as np
import pytest

import ground_cases as gc
import ground_model as gm
import plane_cases as pc
import plane_model as pm
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4


def bits(x):
    return np.atleast_1d(np.asarray(x, F)).view(np.uint32).tolist()


def context(sc, n_slots=2, seed=0):
    c = binding.Context(sc["w"], sc["h"], sc["K"], n_slots=n_slots)
    img = np.random.RandomState(seed).uniform(0, 255, (sc["h"], sc["w"])).astype(F)
    c.frame_upload(0, img, mask=sc["mask"])
    c.trk_set_pc(0, 0, sc["u"], sc["v"], sc["idp"], np.full(len(sc["u"]), 100, F))
    return c


def sentinel_pick():
    k = binding.GroundPick()
    k.ran, k.cluster, k.ground_height, k.n_ground_points = -7, -7, 9.0, -7
    for j in range(4):
        k.gp_raw[j] = 9.0
    return k


def pick_tuple(k):
    return (k.ran, k.cluster, bits(list(k.gp_raw)), bits(k.ground_height), k.n_ground_points)


def assert_pick(pick, want, n_ground=0):
    assert pick.ran == want["ran"] == 1 and pick.cluster == want["cluster"], (pick.cluster, want["cluster"])
    assert bits(list(pick.gp_raw)) == bits(want["gp_raw"]), (list(pick.gp_raw), want["gp_raw"])
    if want["cluster"] >= 0:
        assert bits(pick.ground_height) == bits(want["ground_height"])
    assert pick.n_ground_points == n_ground


def fit_and_choose(c, sc, draws, min_points=20, **kw):
    """the call, the model's clusters held against the records, the model's choice from the records' planes"""
    model = pm.fit_planes(sc["u"], sc["v"], sc["idp"], sc["mask"], sc["w"], sc["h"], sc["K"], draws, min_points=min_points, fast=len(sc["u"]) > 5000)
    recs, n, pick, scores, on = c.trk_fit_ground(draws, min_points=min_points, **kw)
    assert n == len(model)
    for g, m in zip(recs, model):
        assert (g["mask_value"], g["n"], g["n_cloud"], g["fitted"]) == (m["mask_value"], m["n"], m["n_cloud"], m["fitted"])
    want = gm.choose(model, sc["idp"], sc["K"], planes=recs["plane"], min_points=min_points)
    return model, recs, pick, scores, on, want


# ------------------------------------------------------------------------------------------------ (a) score and choice
@pytest.mark.parametrize("w,h", [(64, 48), (80, 48)])
def test_score_and_choice(w, h):
    for name, (sc, seed, append) in gc.score_scenes(w, h).items():
        c = context(sc)
        model, recs, pick, scores, _, want = fit_and_choose(c, sc, pm.make_draws(seed), append=append, pick=sentinel_pick())
        if name == "three":
            # fewer than four clusters: ran = 0 and nothing else is written
            assert len(recs) == 3 and want["ran"] == 0 and pick_tuple(pick) == (0,) + pick_tuple(sentinel_pick())[1:] and not scores.view(np.uint32).any()
            c.close()
            continue
        for r, (s, ws) in enumerate(zip(scores, want["scores"])):
            print("%s %dx%d cluster %d n=%d: scored %d mid_z %r score %r (model %r %r)" % (name, w, h, r, recs["n"][r], s["scored"], s["mid_z"], s["score"], ws[1], ws[2]))
            assert (int(s["scored"]), bits(s["mid_z"]), bits(s["score"])) == (ws[0], bits(ws[1]), bits(ws[2])), (name, r)
        assert_pick(pick, want)
        win = pick.cluster
        if name == "zero_mask_wins":                                    # chosen, and not appended (CoarseTracker.cpp:635)
            assert win == 0 and recs["mask_value"][0] == 0 and recs["appended"][0] == 0 and (recs["appended"][1:] > 0).all()
        if name == "b_positive":
            assert recs["plane"][win][1] > 0 and bits(list(pick.gp_raw)) == bits(-recs["plane"][win])
        if name == "column":
            s = scores["score"]
            assert s[win] == F(-1000) and (s == F(-1000)).sum() == 2 and win == int(np.argmax(s == F(-1000)))           # a tie: the first
            assert recs["plane"][win][1] == 0 and np.signbit(recs["plane"][win][1]) and bits(list(pick.gp_raw)) == bits(recs["plane"][win])
        if name == "zero_idepth":
            assert recs["fitted"][0] == 1 and scores["scored"][0] == 0 and win != 0
        if name == "big":
            assert recs["n"][0] == 1025 and scores["scored"][0] == 1
        c.close()


# ------------------------------------------------------------------------------------------------ (b) the fit is nalo_trk_fit_planes'
@pytest.mark.parametrize("append", [0, 1])
def test_records_members_and_cloud_equal_fit_planes(append):
    for sc, mp in ((pc.planted_scenes(320, 240)["many"], 10), (gc.score_scenes(80, 48)["sizes"][0], 20)):
        a, b = context(sc), context(sc)
        draws = pm.make_draws(3)
        ra, na, pick, _, _ = a.trk_fit_ground(draws, min_points=mp, append=append)
        rb, nb = b.trk_fit_planes(draws, min_points=mp, append=append)
        assert na == nb >= 4 and ra.tobytes() == rb.tobytes() and pick.ran == 1
        members = int(ra["n"].sum())
        for x, y in zip(a.plane_fit_members(len(sc["u"]), members), b.plane_fit_members(len(sc["u"]), members)):     # this call is the "last completed fit"
            assert np.array_equal(x, y)
        for x, y in zip(a.trk_get_pc(0), b.trk_get_pc(0)):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert (ra["appended"].sum() > 0) == bool(append)
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ (c) marking
def issue_window(c, win, st6, host, u, v, idepth, color, weights, exists):
    for i in range(win.W):
        c.frame_upload(i, win.images[i])
    c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=st6)
    c.ba_set_points(host, u, v, idepth, color, weights)
    c.ba_set_residuals(exists)
    c.ba_set_point_history()                                            # lastResiduals as optimizeImmaturePoint leaves them; the fix passes keep them


def read_tested(c):
    """(tested, cpt_u, cpt_v) read back through the C-ABI: lastResiduals[0] names frame W-1 as IN, and that residual is IN"""
    st, _, _, _, cp = c.ba_get_residuals()
    _, lt, ls = c.ba_get_point_history()
    W = c.W
    return (lt[:, 0] == W - 1) & (ls[:, 0] == 0) & (st[:, W - 1] == 0), cp[:, W - 1, 0].copy(), cp[:, W - 1, 1].copy(), st[:, W - 1].copy()


def plant_ground(w, h, K, pix_a, pix_b, seed):
    """A mask and a level-0 cloud with four clusters: A (255) over the pixels pix_a, B (250) over pix_b, each filled up to 120 members with other pixels, and
    two small ones. -> (mask, u, v, idp, is_a, is_b): flipping the sign of a cluster's inverse depths takes it out of the real scores (mid_z < 0)."""
    rng = np.random.RandomState(seed)
    mask = np.full((h, w), 1.0, F)
    taken = set()
    px, val = [], []
    for pix, value in ((pix_a, 255.0), (pix_b, 250.0)):
        for p in pix:
            assert p not in taken and 3 <= p[0] < w - 2 and 3 <= p[1] < h - 2
            taken.add(p); px.append(p); val.append(value)
    for value, n in ((255.0, 120 - len(pix_a)), (250.0, 120 - len(pix_b)), (5.0, 30), (6.0, 30)):
        k = 0
        while k < n:
            p = (int(rng.randint(3, w - 2)), int(rng.randint(3, h - 2)))
            if p in taken:
                continue
            taken.add(p); px.append(p); val.append(value); k += 1
    px, val = np.array(px), np.array(val, F)
    mask[px[:, 1], px[:, 0]] = val
    fx, fy, cx, cy = K
    nrm = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    ray = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(len(px))], 1)
    Z = (3.0 + rng.uniform(-0.002, 0.002, len(px))) / (ray @ nrm)
    u = (px[:, 0] + rng.uniform(0, 0.99, len(px))).astype(F)
    v = (px[:, 1] + rng.uniform(0, 0.99, len(px))).astype(F)
    p = rng.permutation(len(px))
    return mask, u[p], v[p], (1.0 / Z).astype(F)[p], (val == 255.0)[p], (val == 250.0)[p]


def run_marking(c, win_K, w, h, slot, tested, cu, cv, pix_a, pix_b, expect_on_a, expect_on_b):
    """cloud 1: B's inverse depths negative, A is the ground; cloud 2 the other way round; then cloud 1 again. Flags and count against the model's double loop."""
    mask, u, v, idp, is_a, is_b = plant_ground(w, h, win_K, pix_a, pix_b, 3)
    img = np.random.RandomState(1).uniform(0, 255, (h, w)).astype(F)
    c.frame_upload(slot, img, mask=mask)
    draws = pm.make_draws(12)
    P = len(tested)
    seen = []
    for flip, expect in ((is_b, expect_on_a), (is_a, expect_on_b), (is_b, expect_on_a)):
        idp_k = np.where(flip, -idp, idp).astype(F)
        sc = dict(w=w, h=h, K=win_K, mask=mask, u=u, v=v, idp=idp_k)
        c.trk_set_pc(slot, 0, u, v, idp_k, np.full(len(u), 100, F))
        model, recs, pick, scores, on, want = fit_and_choose(c, sc, draws, mark=True, n_points=P)
        assert recs["mask_value"][pick.cluster] == (255.0 if flip is is_b else 250.0)
        on_m, num = gm.mark(want["g_u"], want["g_v"], tested, cu, cv)
        print("ground cluster %d (mask %g): %d of %d tested points on the ground" % (pick.cluster, recs["mask_value"][pick.cluster], num, int(tested.sum())))
        assert_pick(pick, want, n_ground=num)
        assert on.dtype == np.uint8 and np.array_equal(on, on_m)
        assert set(expect) <= set(np.nonzero(on)[0].tolist()), (sorted(np.nonzero(on)[0]), sorted(expect))       # (a filler member may lie under further points)
        seen.append(on.copy())
    assert np.array_equal(seen[0], seen[2]) and not (seen[0] & seen[1]).any()      # the same bytes twice; the second ground found none of the first one's bits


def round_pix(cu, cv, p):
    return (gm.c_int_round(cu[p]), gm.c_int_round(cv[p]))


def test_marking_after_optimize():
    """a window after nalo_ba_optimize and nalo_trk_set_ref_from_window: members planted under read-back centerProjectedTo - under tested points, under points
    whose lastResiduals[0] says OOB / OUTLIER or names another frame, under points whose residual the fix pass removed or that never had one; two points on one pixel"""
    win = synth.make_window(w=320, h=240, W=4, P=300, seed=31)
    host, u, v, idp, col, wts, ex = [a.copy() for a in (win.host, win.u, win.v, win.idepth, win.color, win.weights, win.exists)]
    W = win.W
    hosted_old = np.nonzero(host < W - 1)[0]
    col[hosted_old[:6]] += 120.0                                         # photometric outliers
    idp[hosted_old[6:12]] *= 40.0                                        # projected far outside: OOB
    ex[hosted_old[12:18], W - 1] = 0                                     # no residual to the newest frame
    twins = hosted_old[20:26]                                            # two points on one pixel: copies of six points
    host, u, v, idp = np.append(host, host[twins]), np.append(u, u[twins]), np.append(v, v[twins]), np.append(idp, idp[twins])
    col, wts, ex = np.vstack([col, col[twins]]), np.vstack([wts, wts[twins]]), np.vstack([ex, ex[twins]])
    c = binding.Context(win.w, win.h, win.K, n_slots=W + 1)
    issue_window(c, win, synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003), host, u, v, idp, col, wts, ex)
    c.ba_optimize(6)
    c.trk_set_ref_from_window()
    tested, cu, cv, st = read_tested(c)
    P = len(host)
    # the fix pass removes a residual it finds OOB or OUTLIER (FullSystemOptimize.cpp:187-194): the corrupted points end without one, lastResiduals[0] null
    print("states of the corrupted points' newest residuals:", st[hosted_old[:12]].tolist())
    gone = hosted_old[:18]
    assert (st[gone] == -1).all() and not tested[gone].any() and (c.ba_get_point_history()[1][hosted_old[:12], 0] == -1).all()
    legal = lambda p: 3 <= round_pix(cu, cv, p)[0] < win.w - 2 and 3 <= round_pix(cu, cv, p)[1] < win.h - 2
    cand = [p for p in np.nonzero(tested)[0] if legal(p) and p not in twins and p < P - len(twins)]
    # a history that says OOB / OUTLIER, or names no or another frame, for points whose residual IS IN: untested (CoarseTracker.cpp:675)
    ng, lt, ls = c.ba_get_point_history()
    planted_off = cand[41:46]
    ls[planted_off[0], 0], ls[planted_off[1], 0], ls[planted_off[2], 0], lt[planted_off[3], 0], lt[planted_off[4], 0] = 1, 2, 1, -1, W - 2
    c.ba_set_point_history(ng, lt, ls)
    tested, cu, cv, st = read_tested(c)
    assert not tested[planted_off].any() and (st[planted_off] == 0).all()
    pairs = [(int(a), P - len(twins) + j) for j, a in enumerate(twins) if tested[a] and tested[P - len(twins) + j] and legal(a)]
    assert len(cand) > 50 and pairs and all(round_pix(cu, cv, a) == round_pix(cu, cv, b) for a, b in pairs)
    twin, twin2 = pairs[0]
    pix_a, pix_b, on_a, on_b = [], [], set(), set()
    used = {}
    for k, p in enumerate([twin] + cand[:40]):                          # tested points, alternately on A's and B's pixels
        px = round_pix(cu, cv, p)
        if px in used:
            continue
        used[px] = "a" if k % 2 == 0 else "b"
        (pix_a if k % 2 == 0 else pix_b).append(px)
    for p in planted_off:                                               # untested points: a member under them changes nothing
        px = round_pix(cu, cv, p)
        if px not in used:
            used[px] = "a"; pix_a.append(px)
    for p in gone:                                                      # no residual, no centerProjectedTo: a member on the point's own pixel
        px = (int(u[p]), int(v[p]))
        if px not in used:
            used[px] = "a"; pix_a.append(px)
    for p in np.nonzero(tested)[0]:
        side = used.get(round_pix(cu, cv, p))
        if side:
            (on_a if side == "a" else on_b).add(int(p))
    assert twin in on_a and twin2 in on_a and len(on_a) > 10 and len(on_b) > 10
    run_marking(c, win.K, win.w, win.h, W, tested, cu, cv, pix_a, pix_b, on_a, on_b)
    c.close()


def bilinear(img, x, y):
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - x0, y - y0
    return (1 - fx) * (1 - fy) * img[y0, x0] + fx * (1 - fy) * img[y0, x0 + 1] + (1 - fx) * fy * img[y0 + 1, x0] + fx * fy * img[y0 + 1, x0 + 1]


def test_marking_half_pixels_and_last_legal_pixel():
    """the two newest frames share pose and image, so that centerProjectedTo of a point hosted in W-2 is its own (u, v) to a few ulp. Two fans of points, one ulp
    apart around x = 200.5 and around y = 150.5 (right of and below the principal point, where the projection's intermediate values are finer than the
    result's grid), hold a centerProjectedTo of exactly x.5 and of the float just below it; further: two points on one pixel, a point
    at the largest IN position, a member on the last legal row and column (w - 3, h - 3). One linearizeAll(true), no optimisation."""
    win = synth.make_window(w=320, h=240, W=3, P=120, seed=32)
    W, w, h = win.W, win.w, win.h
    win.world_to_cam[W - 1] = win.world_to_cam[W - 2]
    win.images[W - 1] = win.images[W - 2]
    ulps = lambda x, j: float((np.array([x], F).view(np.int32) + j).view(F)[0])
    fan = range(-24, 25)
    pts = [(ulps(200.5, j), 30.0 + 2 * (j + 24)) for j in fan] + [(150.0 + 2 * (j + 24), ulps(150.5, j)) for j in fan]
    pts += [(100.25, 109.75), (100.375, 109.875), (w - 5.25, h - 5.25), (120.0, 150.25)]
    nu, nv = np.array([p[0] for p in pts], F), np.array([p[1] for p in pts], F)
    img = win.images[W - 2].astype(np.float64)
    ncol = np.stack([bilinear(img, nu.astype(np.float64) + dx, nv.astype(np.float64) + dy) for dx, dy in synth.PATTERN], 1).astype(F)
    n0, k = len(win.host), len(pts)
    host = np.append(win.host, np.full(k, W - 2)).astype(np.int32)
    u, v = np.append(win.u, nu).astype(F), np.append(win.v, nv).astype(F)
    idp = np.append(win.idepth, np.full(k, 0.1)).astype(F)
    col, wts = np.vstack([win.color, ncol]), np.vstack([win.weights, np.ones((k, 8), F)])
    ex = np.vstack([win.exists, np.ones((k, W), np.uint8)])
    ex[n0:, W - 2] = 0
    c = binding.Context(w, h, win.K, n_slots=W + 1)
    issue_window(c, win, None, host, u, v, idp, col, wts, ex)
    c.ba_linearize(True)
    tested, cu, cv, st = read_tested(c)
    assert tested[n0:].all(), st[n0:]
    new = np.arange(n0, n0 + k)
    print("centerProjectedTo - planted, in ulp: u %s v %s" % (sorted(set((cu[new].view(np.int32) - nu.view(np.int32)).tolist())), sorted(set((cv[new].view(np.int32) - nv.view(np.int32)).tolist()))))
    below = lambda x: np.nextafter(F(x), F(0))
    half_u, below_u = new[cu[new] == F(200.5)], new[cu[new] == below(200.5)]
    half_v, below_v = new[cv[new] == F(150.5)], new[cv[new] == below(150.5)]
    assert len(half_u) and len(below_u) and len(half_v) and len(below_v), "the fans must hold x.5 and the float just below it: %s" % ((len(half_u), len(below_u), len(half_v), len(below_v)),)
    assert all(round_pix(cu, cv, p)[0] == 201 for p in half_u) and all(round_pix(cu, cv, p)[0] == 200 for p in below_u)
    assert all(round_pix(cu, cv, p)[1] == 151 for p in half_v) and all(round_pix(cu, cv, p)[1] == 150 for p in below_v)
    two, big = (n0 + 98, n0 + 99), n0 + 100
    assert round_pix(cu, cv, two[0]) == round_pix(cu, cv, two[1]) == (100, 110) and round_pix(cu, cv, big) == (w - 5, h - 5)
    # A: the pixel every planted point rounds to. B: the pixel a wrong rounding would reach - one to the right of / below a float just below x.5, the truncated
    # pixel of an exact x.5 - and the last legal member pixel, which no IN residual reaches (every pattern pixel must project inside w - 3)
    pix_a = sorted({round_pix(cu, cv, p) for p in new[:-1]})
    pix_b = [(201, round_pix(cu, cv, p)[1]) for p in below_u] + [(200, round_pix(cu, cv, p)[1]) for p in half_u]
    pix_b += [(round_pix(cu, cv, p)[0], 151) for p in below_v] + [(round_pix(cu, cv, p)[0], 150) for p in half_v]
    pix_b += [(w - 3, h - 3), round_pix(cu, cv, new[-1])]
    pix_b = sorted(set(pix_b) - set(pix_a))
    on_a = {int(p) for p in np.nonzero(tested)[0] if round_pix(cu, cv, p) in set(pix_a)}
    on_b = {int(p) for p in np.nonzero(tested)[0] if round_pix(cu, cv, p) in set(pix_b)}
    assert set(new[:-1].tolist()) <= on_a and not (set(new[:-1].tolist()) & on_b) and int(new[-1]) in on_b
    run_marking(c, win.K, w, h, W, tested, cu, cv, pix_a, pix_b, on_a, on_b)
    c.close()


# ------------------------------------------------------------------------------------------------ (d) the chain at 1224x368
def fresh_state(gp0, W):
    """scale_fix latched as the scripted run of test_ground_cpu.py leaves it: a primed rate, a full old_rate window, the older frames with a ground"""
    h0 = F(abs(gp0[3]))
    mt, mg, mf = [gm.Tracker(), gm.Tracker()], gm.Globals(), [gm.Frame() for _ in range(W)]
    ct, cg, cf = [binding.ground_tracker(), binding.ground_tracker()], binding.ground_globals(), binding.ground_frames(W)
    mg.scale_fix, mg.init_height, mg.last_ScaleRate, mg.last_gp, mg.old_rate = 1, h0, F(1), np.array(gp0, F), [F(1)] * 7
    cg.scale_fix, cg.init_height, cg.last_ScaleRate, cg.n_old = 1, float(h0), 1.0, 7
    for j in range(4):
        cg.last_gp[j] = float(gp0[j])
    for j in range(7):
        cg.old_rate[j] = 1.0
    for t, ctk in zip(mt, ct):
        t.ground_height = t.last_height = h0
        ctk.ground_height = ctk.last_height = float(h0)
    for i in range(W):
        mf[i].groundP, mf[i].haveground = np.array(gp0, F), 1
        cf[i].haveground = 1
        for j in range(4):
            cf[i].groundP[j] = float(gp0[j])
    return (mt, mg, mf), (ct, cg, cf)


def frames_bits_c(cf):
    return [bits(list(f.groundP)) + bits(list(f.last_ground)) + [f.haveground] for f in cf]


def frames_bits_m(mf):
    return [bits(f.groundP) + bits(f.last_ground) + [f.haveground] for f in mf]


def test_chain_1224_three_keyframes():
    """three keyframes of makeKeyFrame's block (FullSystem.cpp:1404, 1420-1443). Context A: nalo_trk_fit_ground (append, marking) + the C host functions.
    Context B, the route before this call: nalo_trk_fit_planes + nalo_plane_fit_members + nalo_trk_get_pc + nalo_ba_get_residuals + the NumPy model."""
    w, h, W = 1224, 368, 7
    win = synth.make_window(w=w, h=h, W=W, P=700, seed=41)
    mask = pc.block_mask(w, h, 3, 2, [210.0, 7.0, 3.0, 255.0, 220.0, 230.0])
    ctx = []
    for _ in range(2):
        c = binding.Context(w, h, win.K, n_slots=W)
        for i in range(W):
            c.frame_upload(i, win.images[i], mask=mask if i == W - 1 else None)
        ctx.append(c)
    A, B = ctx
    P = len(win.host)
    state = None
    fixed_m = fixed_c = False
    gplane_m = gplane_c = lgh_m = lgh_c = None
    scale_fixes = 0
    for kf in range(3):
        st6 = synth.perturbed_poses(win, seed=50 + kf, sigma_t=0.003, sigma_r=0.0003)
        for c in ctx:
            c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=st6)
            c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
            c.ba_set_residuals(win.exists)
            c.ba_set_point_history()
            c.ba_optimize(4)
            c.trk_set_ref_from_window()
        draws = pm.make_draws(60 + kf)
        # ---- B: the host route
        u, v, idp, _ = B.trk_get_pc(0)
        recs_b, n_b = B.trk_fit_planes(draws, min_points=20, append=1)
        cl_of, order = B.plane_fit_members(len(u), int(recs_b["n"].sum()))
        clusters, off = [], 0
        for r in recs_b:
            mem = order[off:off + r["n"]].astype(np.int64)
            off += r["n"]
            clusters.append(dict(members=mem, xx=u[mem].astype(np.int64), yy=v[mem].astype(np.int64), mask_value=r["mask_value"], n=int(r["n"]), n_cloud=int(r["n_cloud"]),
                                 fitted=int(r["fitted"]), plane=r["plane"]))
        want = gm.choose(clusters, idp, win.K)
        tested, cu, cv, _ = read_tested(B)
        on_m, num = gm.mark_fast(want["g_u"], want["g_v"], tested, cu, cv)
        # ---- A: the device route
        recs_a, n_a, pick, scores, on = A.trk_fit_ground(draws, append=1, mark=True, n_points=P)
        assert n_a == n_b >= 4 and recs_a.tobytes() == recs_b.tobytes()
        assert_pick(pick, want, n_ground=num)
        assert np.array_equal(on, on_m)
        for s, ws in zip(scores, want["scores"]):
            assert (int(s["scored"]), bits(s["mid_z"]), bits(s["score"])) == (ws[0], bits(ws[1]), bits(ws[2]))
        print("keyframe %d: ground = cluster %d (mask %g, n %d), height %r, %d of %d tested window points on it" %
              (kf, pick.cluster, recs_a["mask_value"][pick.cluster], recs_a["n"][pick.cluster], pick.ground_height, num, int(tested.sum())))
        assert pick.cluster >= 0 and num > 0
        for x, y in zip(A.trk_get_pc(0), B.trk_get_pc(0)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        # ---- the state machine: the C functions (A) beside the model (B)
        if state is None:
            state = fresh_state(want["gp_raw"], W)
        (mt, mg, mf), (ct, cg, cf) = state
        mf[:] = mf[1:] + [gm.Frame()]                                    # the oldest frame leaves, the new keyframe enters
        for i in range(W - 1):
            C.memmove(C.byref(cf[i]), C.byref(cf[i + 1]), C.sizeof(binding.GroundFrame))
        binding.host_lib().nalo_ground_frame_init(C.byref(cf[W - 1]))
        gm.update(want, mt[kf % 2], mg, mf)
        binding.ground_update(pick, ct[kf % 2], cg, cf)
        assert frames_bits_c(cf) == frames_bits_m(mf) and bits(list(cg.old_rate)) == bits(mg.old_rate) and bits(cg.last_ScaleRate) == bits(mg.last_ScaleRate)
        _, w2c_a, _ = A.ba_get_frames()
        _, w2c_b, _ = B.ba_get_frames()
        assert np.array_equal(w2c_a, w2c_b)
        if mf[-1].haveground and mf[-1].groundP[3] != 0:                 # FullSystem.cpp:1420
            assert cf[W - 1].haveground
            if not fixed_m:
                fixed_m, gplane_m, lgh_m = gm.set_global_plane(mf, w2c_b[1])
                fixed_c, gplane_c, _, lgh_c = binding.ground_set_global_plane(cf, w2c_a[1])
                assert fixed_m == fixed_c
                if fixed_m:
                    assert gplane_c.view(np.uint64).tolist() == gplane_m.view(np.uint64).tolist() and bits(lgh_c) == bits(lgh_m)
            if mg.scale_fix and fixed_m:                                 # :1438
                ls_m, ls_c = gm.local_scale(mf[-1], lgh_m), binding.ground_local_scale(cf[W - 1], lgh_c)
                assert ls_c == ls_m and ls_m is not None
                print("keyframe %d: localscale %r" % (kf, ls_c))
                c2w_ref = synth.se3_inv(w2c_a[W - 2])
                cam2ref = synth.se3_mul(w2c_a[W - 2], synth.se3_inv(w2c_a[W - 1]))
                A.ba_plane_scale_fix(ls_c, cam2ref, c2w_ref)
                B.ba_plane_scale_fix(ls_m, cam2ref, c2w_ref)
                scale_fixes += 1
                assert np.array_equal(A.ba_get_frames()[1], B.ba_get_frames()[1])
                pa, pb = A.ba_get_points(), B.ba_get_points()
                assert all(np.array_equal(pa[k].view(np.uint32), pb[k].view(np.uint32)) for k in pa)
    assert fixed_m and scale_fixes >= 1, "the chain must reach nalo_ba_plane_scale_fix"
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------ (e) refusals
def snapshot(c, with_window):
    s = [a.tobytes() for l in range(c.levels) for a in c.trk_get_pc(l) + list(c.trk_get_depth(l))]
    if with_window:
        s += [a.tobytes() for a in c.ba_get_residuals()]
        try:
            s += [a.tobytes() for a in c.ba_get_point_history()]
        except binding.NaloError:
            s += ["no history"]
        s += [c.ba_get_frames()[1].tobytes()] + [a.tobytes() for a in c.ba_get_points().values()]
    return s


def test_refusals_leave_everything_alone():
    win = synth.make_window(w=320, h=240, W=4, P=300, seed=33)
    W, P = win.W, len(win.host)
    c = binding.Context(win.w, win.h, win.K, n_slots=W + 1)
    sc = gc.score_scenes(80, 48)["sizes"][0]
    draws = pm.make_draws(1)
    d32 = np.ascontiguousarray(draws, np.uint32)
    fit = binding.PlaneFitArgs(0.01, 20, len(d32) // 3, d32.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
    out = np.zeros(64, binding.PLANE_DTYPE)
    n = np.zeros(1, np.int32)
    on = np.zeros(P, np.uint8)

    def call(mark=1, fit_=fit, g="default", cap=64, pick="default", on_cap=P):
        k = sentinel_pick() if pick == "default" else pick
        ga = binding.GroundArgs(mark, binding._u8(on), on_cap, None) if g == "default" else g
        rc = c.L.nalo_trk_fit_ground(c.h_, None if fit_ is None else C.byref(fit_), None if ga is None else C.byref(ga), cap, out.ctypes.data_as(C.c_void_p), binding._i(n),
                                     None if k is None else C.byref(k))
        if k is not None:
            assert pick_tuple(k) == pick_tuple(sentinel_pick()), "a refused call wrote into pick"
        return rc

    assert call(mark=0) == ERR_STATE and b"level-0 cloud" in c.L.nalo_last_error(c.h_)             # nalo_trk_fit_planes' refusals come first
    img = np.random.RandomState(0).uniform(0, 255, (win.h, win.w)).astype(F)
    mask = np.full((win.h, win.w), 1.0, F)
    mask[:, 80:160], mask[:, 160:240], mask[:, 240:] = 255.0, 250.0, 5.0
    rng = np.random.RandomState(2)
    ref = [rng.uniform(5, win.w - 6, 800).astype(F), rng.uniform(5, win.h - 6, 800).astype(F), rng.uniform(0.2, 0.4, 800).astype(F), rng.uniform(1e-5, 1e-3, 800).astype(F)]
    c.frame_upload(W, img)
    c.trk_set_ref(W, *ref)
    assert call(mark=0) == ERR_STATE and b"mask" in c.L.nalo_last_error(c.h_)
    c.frame_upload(W, img, mask=mask)
    c.trk_set_ref(W, *ref)
    n_cloud = len(c.trk_get_pc(0)[0])
    before = snapshot(c, False)
    assert call() == ERR_STATE and b"no window" in c.L.nalo_last_error(c.h_)
    assert snapshot(c, False) == before
    for i in range(W):
        c.frame_upload(i, win.images[i])
    c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003))
    assert call() == ERR_STATE and b"no points" in c.L.nalo_last_error(c.h_)
    assert snapshot(c, False) == before
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(win.exists)
    c.ba_optimize(4)
    assert snapshot(c, False) == before
    before = snapshot(c, True)
    assert call() == ERR_STATE and b"history" in c.L.nalo_last_error(c.h_)                          # no point history
    assert snapshot(c, True) == before
    c.ba_set_point_history()
    c.ba_linearize(False)
    before = snapshot(c, True)
    assert call() == ERR_STATE and b"linearizeAll(true)" in c.L.nalo_last_error(c.h_)               # the last linearisation was not fix = 1
    assert snapshot(c, True) == before
    c.ba_linearize(True)
    before = snapshot(c, True)
    c.ba_set_allreduce(lambda ptr, k: None)
    assert call() == ERR_STATE and b"sharded" in c.L.nalo_last_error(c.h_)
    c.ba_set_allreduce(None)
    assert snapshot(c, True) == before
    assert call(g=None) == ERR_ARG and call(pick=None) == ERR_ARG and call(fit_=None) == ERR_ARG
    assert call(on_cap=P - 1) == ERR_ARG and b"onground_cap" in c.L.nalo_last_error(c.h_)
    bad = binding.PlaneFitArgs(0.01, 20, 0, d32.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
    assert call(fit_=bad) == ERR_ARG
    bad = binding.PlaneFitArgs(-1.0, 20, len(d32) // 3, d32.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
    assert call(fit_=bad) == ERR_ARG
    assert call(cap=2) == ERR_ARG and int(n[0]) == 4                                                 # cap below the need: the need is reported, nothing appended
    assert not on.any() and snapshot(c, True) == before
    # the context is usable: the same call goes through, marks, and appends
    k = sentinel_pick()
    ga = binding.GroundArgs(1, binding._u8(on), P, None)
    assert c.L.nalo_trk_fit_ground(c.h_, C.byref(fit), C.byref(ga), 64, out.ctypes.data_as(C.c_void_p), binding._i(n), C.byref(k)) == 0
    assert k.ran == 1 and int(n[0]) == 4 and k.cluster >= 0 and len(c.trk_get_pc(0)[0]) > n_cloud
    c.close()
