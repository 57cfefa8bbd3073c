"""The immature-point path at the shapes and exposures a running system gives it, against the fp32 oracle, BIT-EXACT (NaNs compare equal).

test_imm_gpu.py stays the fast small case: 640x480, W = 5, identity brightness, window position = slot. Here:

  case  frame      W   hosts x points   what it adds
  K     1224x368   8   8 x ~1500        KITTI's shape: 44-step first searches; ragged 32x32 distance-map tiles (612x184); the brightness term against
                                        an identity-brightness run of the same points on the un-brightened frames
  B     1920x1072  8   8 x ~1500        the front end's shape: 82-step first searches (LDS rows 32..81 of the step buffer); 960x536 distance map
  X     2560x1280  2   2 x ~1500        w + h >= 3630: every uninitialised point that passes the bounds tests runs exactly the 99 clamped steps
  S     640x480    16  16 x ~400        the ABI's largest window: 15 residuals per point (2-bit states up to shift 28, LDS energies of 15 residuals,
                                        res_in rows of 16 bytes), a resident trace over 16 host frames (the 224-float per-host table full)

Every frame i carries its own affine pair (a_i, b_i) and exposure e_i and is rendered as e_i exp(a_i) I_i + b_i, so that
AffLight::fromToVecExposure is exactly the brightness change between any host and target. Frames live in their slots in a fixed random
permutation (a running system's slots are permuted after the first marginalisation); the oracle gets the images in window order. Point counts
are never multiples of the kernels' 32 points per workgroup, and n = 1 runs too.

Each test asserts which branches its inputs reach, from the outputs or from fp64 geometry in numpy: every trace status, OUTLIER -> OOB, entries
with finite and NaN idepth_max, x- and y-dominant epipolar lines, searches of more and of fewer than 10 steps and of more than 32 (and the 99-step
clamp at X); activation results 1, 0 and -1, res_in rows with IN and non-IN targets, and point/target pairs whose first pattern pixel to leave
(1.1, w-3) x (1.1, h-3) at the starting depth is one of pixels 1..7 (the partial sums of linearizeResidual). The histograms are printed (-s)."""
import dataclasses

import numpy as np
import pytest

import orc
from imm_helpers import host_to_new, imm_points, true_idepth
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
PATTERN = synth.PATTERN
CASES = {
    "K": dict(w=1224, h=368, W=8, P=200, per_host=1500, step_z=0.25, yaw=0.4, identity=True),
    "B": dict(w=1920, h=1072, W=8, P=400, per_host=1500, step_z=0.25, yaw=0.4),
    "X": dict(w=2560, h=1280, W=2, P=16, per_host=1500, step_z=0.25, yaw=0.4),
    "S": dict(w=640, h=480, W=16, P=400, per_host=400, step_z=0.08, yaw=0.15),
}


def eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def hist(a, values):
    return [int((a == x).sum()) for x in values]


class Case:
    """a window of W keyframes + 2 later frames, brightened per frame, uploaded into permuted slots (and, with identity, the un-brightened
    frames into slots F..2F-1)"""

    def __init__(self, name):
        s = CASES[name]
        self.name, W = name, s["W"]
        raw = synth.make_window(w=s["w"], h=s["h"], W=W, P=s["P"], seed=9, n_extra=2, step_z=s["step_z"], yaw_deg=s["yaw"])
        F = W + 2
        rng = np.random.RandomState(31 + W)
        # Python floats, as a caller writes them: ba_set_window must turn them into the reference's double state (HessianBlocks.h:247-255)
        self.aff = [(float(a), float(b)) for a, b in zip(rng.uniform(-0.1, 0.1, F), rng.uniform(-8, 8, F))]
        self.exposure = rng.uniform(0.7, 1.4, F).astype(np.float32)
        bright = [(np.float64(e) * np.exp(a) * img.astype(np.float64) + b).astype(np.float32) for (a, b), e, img in zip(self.aff, self.exposure, raw.images)]
        self.raw, self.win = raw, dataclasses.replace(raw, images=np.stack(bright))
        self.W, self.F, self.w, self.h = W, F, raw.w, raw.h
        self.slot = rng.permutation(F)                                         # frame i lives in slot self.slot[i]
        assert (self.slot[:W] != np.arange(W)).any()
        self.c = binding.Context(raw.w, raw.h, raw.K, n_slots=2 * F if s.get("identity") else F)
        for i in range(F):
            self.c.frame_upload(int(self.slot[i]), self.win.images[i])
            if s.get("identity"):
                self.c.frame_upload(F + int(self.slot[i]), raw.images[i])
        self.dI = [orc.make_images(self.win.images[i], 1)[0] for i in range(F)]   # level-0 texels for the oracle, window order

    def points(self, per_host, seed, margin):
        u, v, host = imm_points(self.win, per_host=per_host, seed=seed, margin=margin)
        if len(u) % 32 == 0:                                                   # a ragged last workgroup
            u, v, host = u[:-1], v[:-1], host[:-1]
        assert len(u) % 32 != 0
        return u, v, host

    def create(self, u, v, host, identity=False):
        """ImmaturePoint ctor per host frame; against the oracle bit for bit (not for the identity frames, which only serve the brightness tests)"""
        n = len(u)
        color, weights, gradH, eth = [np.zeros((n, k), np.float32) for k in (8, 8, 3)] + [np.zeros(n, np.float32)]
        for h in range(self.W):
            m = host == h
            got = self.c.imm_create(int(self.slot[h]) + (self.F if identity else 0), u[m], v[m])
            if not identity:
                for g, r in zip(got, orc.imm_create(self.dI[h], self.w, self.h, u[m], v[m])):
                    assert eq(g, r)
            color[m], weights[m], gradH[m], eth[m] = got
        return color, weights, gradH, eth

    def set_window(self, st6, identity=False):
        W = self.W
        if identity:
            self.c.ba_set_window([self.F + int(s) for s in self.slot[:W]], self.win.world_to_cam[:W], state6=st6)
        else:
            self.c.ba_set_window([int(s) for s in self.slot[:W]], self.win.world_to_cam[:W], aff=self.aff[:W], exposure=self.exposure[:W], state6=st6)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
        return made[name]
    yield get
    for cs in made.values():
        cs.c.close()


def fresh_state(n):
    return dict(idmin=np.zeros(n, np.float32), idmax=np.full(n, np.nan, np.float32), status=np.full(n, UNINITIALIZED, np.int32),
                quality=np.full(n, 10000, np.float32))


def search_geometry(cs, u, v, host, KRKi, Kt, idmin, idmax):
    """traceOn's search line in fp64 (ImmaturePoint.cpp:106-263): numSteps before the 99 clamp and whether the line is x-dominant"""
    w, h = cs.w, cs.h
    maxpix = float(np.float32(w + h) * np.float32(0.027))
    M, T = KRKi.astype(np.float64).reshape(-1, 3, 3)[host], Kt.astype(np.float64)[host]
    pr = np.einsum("nij,nj->ni", M, np.stack([u, v, np.ones(len(u))], 1).astype(np.float64))
    fin = np.isfinite(idmax)
    pmin = pr + T * idmin.astype(np.float64)[:, None]
    pmax = pr + T * np.where(fin, idmax, 0.01).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = pmax[:, :2] / pmax[:, 2:] - pmin[:, :2] / pmin[:, 2:]
        dist = np.minimum(np.where(fin, np.hypot(d[:, 0], d[:, 1]), maxpix), maxpix)
        steps = np.floor(1.9999 + dist)
    return steps, d[:, 0] ** 2 > d[:, 1] ** 2


def trace_rounds(cs, u, v, host, pts, oracle=True, pair=True, slot_offset=0):
    """three traceOn rounds against frames W, W+1, W (like successive traceNewCoarse calls), GPU against the oracle; returns per round
    (state in, outputs, KRKi, Kt)"""
    W, n = cs.W, len(u)
    uf, vf = u.astype(np.float32), v.astype(np.float32)
    st = fresh_state(n)
    out = []
    for new in (W, W + 1, W):
        KRKi, Kt, aff = host_to_new(cs.win, new, cs.aff, cs.exposure) if pair else host_to_new(cs.win, new)
        g = cs.c.imm_trace(int(cs.slot[new]) + slot_offset, uf, vf, *pts, host, KRKi, Kt, aff, st["idmin"], st["idmax"], st["status"], st["quality"])
        if oracle:
            o = orc.imm_trace(cs.dI[new], cs.w, cs.h, uf, vf, *pts, host, KRKi, Kt, aff, st["idmin"], st["idmax"], st["status"], st["quality"])
            for name, a, b in zip(("idmin", "idmax", "status", "quality", "lastUV", "lastInterval"), g, o):
                touched = o[2] != OOB if name in ("lastUV", "lastInterval") else slice(None)      # OOB-on-entry points return before writing those
                assert eq(a[touched], b[touched]), (cs.name, new, name)
        out.append((st, g, KRKi, Kt))
        st = dict(idmin=g[0], idmax=g[1], status=g[2], quality=g[3])
    return out


@pytest.mark.parametrize("name", ["K", "B", "X"])
def test_trace_bit_exact_and_coverage(cases, name):
    cs = cases(name)
    u, v, host = cs.points(1500, seed=2, margin=3)
    pts = cs.create(u, v, host)
    rounds = trace_rounds(cs, u, v, host, pts)
    seen, searched_steps, xdom = set(), [], []
    outlier_to_oob = 0
    for r, (st, g, KRKi, Kt) in enumerate(rounds):
        status_in, status = st["status"], g[2]
        seen |= set(np.unique(status).tolist())
        steps, xd = search_geometry(cs, u, v, host, KRKi, Kt, st["idmin"], st["idmax"])
        # GOOD and OUTLIER come only after the search (an OUTLIER that fails the energy test again becomes OOB)
        searched = (status_in != OOB) & ((status == GOOD) | (status == OUTLIER) | ((status_in == OUTLIER) & (status == OOB)))
        searched_steps.append((steps[searched], np.isfinite(st["idmax"][searched])))
        xdom.append(xd[searched & (status == GOOD)])
        if r > 0:
            outlier_to_oob += int(((status_in == OUTLIER) & (status == OOB)).sum())
        print("IMM-COVER trace %s n=%d round %d status GOOD/OOB/OUTLIER/SKIPPED/BADCONDITION = %s, OUTLIER->OOB %d, searched %d (steps > 10: %d, > 32: %d, "
              ">= 99: %d)" % (name, len(u), r, hist(status, range(5)), int(((status_in == OUTLIER) & (status == OOB)).sum()), int(searched.sum()),
                              int((steps[searched] > 10).sum()), int((steps[searched] > 32).sum()), int((steps[searched] >= 99).sum())))
    assert {GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION}.issubset(seen), seen
    assert outlier_to_oob > 0
    first, first_fin = searched_steps[0]
    assert len(first) > 0 and not first_fin.any()                          # searches that enter with idepth_max = NaN (the full maxPixSearch line) ...
    later = np.concatenate([s[f] for s, f in searched_steps[1:]])          # ... and with a finite interval
    assert (later > 10).any() and (later <= 10).any()                      # both sides of `numSteps > 10` in the quality update
    xd = np.concatenate(xdom)
    assert xd.any() and (~xd).any()                                        # x- and y-dominant epipolar lines (the two interval formulas)
    if cs.w + cs.h >= 3630:
        assert (first >= 100).all()                                        # the clamp: every uninitialised search runs 99 steps
    else:
        assert (first > 32).all() and (first < 100).all()                 # beyond the 32 steps of 640x480, below the clamp
    # n = 1 and small ragged batches: the same bit-exact answers as inside the large batch
    st0, g0, KRKi, Kt = rounds[1]
    uf, vf = u.astype(np.float32), v.astype(np.float32)
    for sl in (slice(7, 8), slice(100, 131), slice(200, 233)):
        a = [x[sl] for x in pts]
        g = cs.c.imm_trace(int(cs.slot[cs.W + 1]), uf[sl], vf[sl], *a, host[sl], KRKi, Kt, host_to_new(cs.win, cs.W + 1, cs.aff, cs.exposure)[2],
                           *[st0[k][sl] for k in ("idmin", "idmax", "status", "quality")])
        touched = st0["status"][sl] != OOB
        for k in range(4):
            assert eq(g[k], g0[k][sl])
        assert eq(g[4][touched], g0[4][sl][touched]) and eq(g[5][touched], g0[5][sl][touched])


def test_trace_brightness_term_matters(cases):
    """Without the oracle: with the right affine pair, the brightened frames trace about as well as the un-brightened frames with the identity pair;
    the brightened frames traced with the identity pair give several times more OUTLIERs. Asserted on the two rounds against new frames (the third
    retraces frame W, where most intervals are already too short to search)."""
    cs = cases("K")
    u, v, host = cs.points(1500, seed=2, margin=3)
    pts = cs.create(u, v, host)
    right = trace_rounds(cs, u, v, host, pts, oracle=False)
    wrong = trace_rounds(cs, u, v, host, pts, oracle=False, pair=False)
    ident = trace_rounds(cs, u, v, host, cs.create(u, v, host, identity=True), oracle=False, pair=False, slot_offset=cs.F)
    for r in range(3):
        sr, sw, si = right[r][1][2], wrong[r][1][2], ident[r][1][2]
        print("IMM-COVER brightness K round %d GOOD/OUTLIER right pair %d/%d, identity pair %d/%d, un-brightened frames %d/%d"
              % (r, (sr == GOOD).sum(), (sr == OUTLIER).sum(), (sw == GOOD).sum(), (sw == OUTLIER).sum(), (si == GOOD).sum(), (si == OUTLIER).sum()))
        if r < 2:
            assert (sr == GOOD).sum() >= 0.8 * (si == GOOD).sum()
            assert (sw == OUTLIER).sum() >= 3 * max((sr == OUTLIER).sum(), 1)


def optimize_inputs(cs, per_host, seed):
    u, v, host = cs.points(per_host, seed=seed, margin=3)                  # down to the pattern padding: partial patterns in the targets
    pts = cs.create(u, v, host)
    n = len(u)
    idt = true_idepth(cs.win, u, v, host)
    rng = np.random.RandomState(seed + 1)
    mid = idt * (1 + 0.05 * rng.randn(n)).astype(np.float32)              # a traced interval around a 5 % wrong depth
    far = rng.rand(n) < 0.1
    mid[far] *= rng.choice([0.5, 2.0], far.sum()).astype(np.float32)      # and some far off: outlier residuals
    idmin, idmax = (mid * 0.9).astype(np.float32), (mid * 1.1).astype(np.float32)
    idmin[::50] = np.nan                                                   # broken points: never activated
    return u, v, host, pts, idmin, idmax


def first_failing_pixel(cs, Rt, u, v, host, idepth):
    """linearizeResidual's per-pattern test (ImmaturePoint.cpp:511-525) in fp64 at the starting depth: for every point and target the index of the
    first pattern pixel that is behind the camera or outside (1.1, w-3) x (1.1, h-3), 8 if none; -1 for the host itself"""
    W = cs.W
    fx, fy, cx, cy = [float(np.float32(k)) for k in cs.win.K]
    out = np.full((len(u), W), -1)
    for t in range(W):
        m = host != t
        idx = host[m] * W + t
        R, tt = Rt[idx, :9].astype(np.float64).reshape(-1, 3, 3), Rt[idx, 9:].astype(np.float64)
        ok = np.ones((m.sum(), 8), bool)
        for k in range(8):
            k0, k1 = (u[m] + PATTERN[k, 0] - cx) / fx, (v[m] + PATTERN[k, 1] - cy) / fy
            p = np.einsum("nij,nj->ni", R, np.stack([k0, k1, np.ones(len(k0))], 1)) + tt * idepth[m, None].astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                Ku, Kv = p[:, 0] / p[:, 2] * fx + cx, p[:, 1] / p[:, 2] * fy + cy
                ok[:, k] = (p[:, 2] > 0) & (Ku > 1.1) & (Kv > 1.1) & (Ku < cs.w - 3) & (Kv < cs.h - 3)
        out[m, t] = np.where(ok.all(1), 8, np.argmin(ok, 1))
    return out


@pytest.mark.parametrize("name,min_obs", [("K", 3), ("B", 3), ("S", 6)])
def test_optimize_bit_exact_and_coverage(cases, name, min_obs):
    cs = cases(name)
    W = cs.W
    u, v, host, pts, idmin, idmax = optimize_inputs(cs, CASES[name]["per_host"], seed=3)
    color, weights, gradH, eth = pts
    n = len(u)
    uf, vf = u.astype(np.float32), v.astype(np.float32)
    st6 = synth.perturbed_poses(cs.win, sigma_t=0.002, sigma_r=0.0002)
    cs.set_window(st6)
    ba = orc.ba_from_window(cs.win, "f32", state6=st6, aff=cs.aff[:W], exposure=cs.exposure[:W])
    Rt, af = ba.precalc_rt()
    assert len(np.unique(af[:, 0])) > W                                     # a distinct brightness change for every ordered pair
    results = {}
    for mo in (1, min_obs):
        res_o, idp_o, rin_o = orc.imm_optimize(cs.dI[:W], cs.w, cs.h, cs.win.K, Rt, af, host, uf, vf, color, weights, eth, idmin, idmax, mo)
        res, idp, rin = cs.c.imm_optimize(host, uf, vf, color, weights, eth, idmin, idmax, mo)
        assert eq(res, res_o) and eq(idp, idp_o) and eq(rin, rin_o), (name, mo)
        results[mo] = (res, idp, rin)
        act = res == 1
        nin = rin.sum(1)
        print("IMM-COVER optimize %s W=%d n=%d minObs=%d result 1/0/-1 = %s, activated with IN and non-IN targets %d"
              % (name, W, n, mo, hist(res, (1, 0, -1)), int((act & (nin < W - 1)).sum())))
        assert (nin[act] >= mo).all() and (rin[~act] == 0).all() and (rin[np.arange(n), host] == 0).all()
    res1, res2 = results[1][0], results[min_obs][0]
    assert {1, 0, -1}.issubset(set(res1.tolist()) | set(res2.tolist()))
    assert (res2 == -1).sum() > (res1 == -1).sum()
    act = res1 == 1
    assert act.sum() > 0.3 * n and (act & (results[1][2].sum(1) < W - 1)).sum() > 0
    ff = first_failing_pixel(cs, Rt, u, v, host, (idmax + idmin) * np.float32(0.5))
    partial = (ff >= 1) & (ff <= 7)
    print("IMM-COVER optimize %s partial-pattern point/target pairs %d (first failing pixel 1..7: %s), whole-pattern misses %d, all inside %d"
          % (name, partial.sum(), hist(ff, range(1, 8)), (ff == 0).sum(), (ff == 8).sum()))
    assert partial.sum() >= 30
    # the device-resident set: all points, then a shuffled subset named by index
    c = cs.c
    c.imm_resident_set(uf, vf, color, weights, gradH, eth, host, idmin, idmax, np.zeros(n, np.int32), np.zeros(n, np.float32))
    res_r, idp_r, rin_r = c.imm_resident_optimize(None, 1, n_all=n)
    assert eq(res_r, results[1][0]) and eq(idp_r, results[1][1]) and eq(rin_r, results[1][2])
    sel = np.random.RandomState(8).permutation(n)[:n // 3 + 1].astype(np.int32)
    res_s, idp_s, rin_s = c.imm_resident_optimize(sel, min_obs)
    assert eq(res_s, res2[sel]) and eq(idp_s, results[min_obs][1][sel]) and eq(rin_s, results[min_obs][2][sel])
    # n = 1 and a small ragged batch
    for sl in (slice(5, 6), slice(40, 73)):
        r = c.imm_optimize(host[sl], uf[sl], vf[sl], color[sl], weights[sl], eth[sl], idmin[sl], idmax[sl], 1)
        assert eq(r[0], results[1][0][sl]) and eq(r[1], results[1][1][sl]) and eq(r[2], results[1][2][sl])


def test_optimize_brightness_term_matters(cases):
    """Without the oracle: the brightened window with its affine states and exposures activates about as many points as the un-brightened window
    with identity brightness."""
    cs = cases("K")
    u, v, host, pts, idmin, idmax = optimize_inputs(cs, 1500, seed=3)
    uf, vf = u.astype(np.float32), v.astype(np.float32)
    st6 = synth.perturbed_poses(cs.win, sigma_t=0.002, sigma_r=0.0002)
    cs.set_window(st6)
    res = cs.c.imm_optimize(host, uf, vf, pts[0], pts[1], pts[3], idmin, idmax, 1)[0]
    ipts = cs.create(u, v, host, identity=True)
    cs.set_window(st6, identity=True)
    res_i = cs.c.imm_optimize(host, uf, vf, ipts[0], ipts[1], ipts[3], idmin, idmax, 1)[0]
    print("IMM-COVER brightness K activated: brightened window %d, un-brightened identity window %d of %d" % ((res == 1).sum(), (res_i == 1).sum(), len(u)))
    assert (res == 1).sum() >= 0.8 * (res_i == 1).sum() and (res_i == 1).sum() > 0.3 * len(u)


def test_resident_trace_16_hosts(cases):
    """nalo_imm_resident_trace with nh = 16 host frames (14 x 16 = 224 floats per frame) = three staged traces = the oracle; the argument checks"""
    cs = cases("S")
    W = cs.W
    u, v, host = cs.points(400, seed=6, margin=3)
    assert set(host.tolist()) == set(range(16))
    pts = cs.create(u, v, host)
    n = len(u)
    uf, vf = u.astype(np.float32), v.astype(np.float32)
    st = fresh_state(n)
    c = cs.c
    c.imm_resident_set(uf, vf, *pts, host, st["idmin"], st["idmax"], st["status"], st["quality"])
    rounds = trace_rounds(cs, u, v, host, pts)                             # staged calls, against the oracle
    for new in (W, W + 1, W):
        KRKi, Kt, aff = host_to_new(cs.win, new, cs.aff, cs.exposure)
        assert KRKi.shape == (16, 9)
        c.imm_resident_trace(int(cs.slot[new]), KRKi, Kt, aff)
    uv, li = np.full((n, 2), -1, np.float32), np.zeros(n, np.float32)
    for st_in, g, _, _ in rounds:
        touched = st_in["status"] != OOB
        uv[touched], li[touched] = g[4][touched], g[5][touched]
    r = c.imm_resident_get()
    last = rounds[-1][1]
    for a, b in zip(r[:4], last[:4]):
        assert eq(a, b)
    assert eq(r[4], uv) and eq(r[5], li)
    print("IMM-COVER resident trace S nh=16 n=%d final status GOOD/OOB/OUTLIER/SKIPPED/BADCONDITION = %s" % (n, hist(r[2], range(5))))
    good = rounds[1][1][2] == GOOD                                          # after the second new frame
    assert good.sum() > 0.25 * n and all((good & (host == h)).any() for h in range(16))
    KRKi, Kt, aff = host_to_new(cs.win, W, cs.aff, cs.exposure)
    with pytest.raises(RuntimeError):
        c.imm_resident_trace(int(cs.slot[W]), np.concatenate([KRKi, KRKi[:1]]), np.concatenate([Kt, Kt[:1]]), np.concatenate([aff, aff[:1]]))   # nh = 17
    with pytest.raises(RuntimeError):
        c.imm_resident_trace(int(cs.slot[W]), KRKi[:15], Kt[:15], aff[:15])   # a resident point of host 15 with nh = 15
    cs.set_window(np.zeros((W, 6)))
    h2 = host.copy(); h2[-1] = W
    c.imm_resident_set(uf, vf, *pts, h2, st["idmin"], st["idmax"], st["status"], st["quality"])
    with pytest.raises(RuntimeError):
        c.imm_resident_optimize(None, 1, n_all=n)                          # a resident host index >= W
    with pytest.raises(RuntimeError):
        c.imm_optimize(h2, uf, vf, pts[0], pts[1], pts[3], st["idmin"], st["idmax"], 1)


@pytest.mark.parametrize("name", ["K", "B"])
def test_distance_map_exact(cases, name):
    """CoarseDistanceMap::makeDistanceMap at level 1 of a real shape, permuted slots, exact equality. The 32x32 tiles are ragged on both axes at
    612x184 and on y at 960x536 (960 = 30 x 32)."""
    cs = cases(name)
    win, W = cs.win, cs.W
    w1, h1 = win.w >> 1, win.h >> 1
    assert h1 % 32 and (w1 % 32 or name == "B")
    cs.set_window(np.zeros((W, 6)))
    cs.c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    fx, fy, cx, cy = [np.float32(x) for x in win.K]
    K1 = np.array([[fx * np.float32(0.5), 0, np.float32((cx + 0.5) / 2 - 0.5)], [0, fy * np.float32(0.5), np.float32((cy + 0.5) / 2 - 0.5)], [0, 0, 1]], np.float32)
    Ki0 = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float32)
    frame = W - 1
    KRKi, Kt = np.zeros((W, 9), np.float32), np.zeros((W, 3), np.float32)
    for h in range(W):
        T = synth.se3_mul(win.world_to_cam[frame], synth.se3_inv(win.world_to_cam[h]))
        KRKi[h] = ((K1 @ T[:, :3].astype(np.float32)) @ Ki0).reshape(-1)
        Kt[h] = K1 @ T[:, 3].astype(np.float32)
    got = cs.c.dist_make_map(frame, KRKi, Kt)
    ref = orc.dist_make_map(w1, h1, frame, win.host, win.u, win.v, win.idepth, KRKi, Kt)
    assert got.shape == (h1, w1) and np.array_equal(got, ref)
    vals = set(np.unique(got).astype(int).tolist())
    print("IMM-COVER distance map %s %dx%d levels present %d of 0..39, 1000: %d px" % (name, w1, h1, len(vals & set(range(40))), (got == 1000).sum()))
    assert {0, 1000}.issubset(vals) and set(range(1, 40)).issubset(vals) and (got == 1000).sum() >= 20
