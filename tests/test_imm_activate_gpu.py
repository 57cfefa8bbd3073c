"""nalo_imm_resident_activate (activatePointsMT's distance map + selection loop + optimizeImmaturePoint, on the device) against the literal model of
tests/activation_model.py: fate, n_sel and sel EXACT, result / idepth_out / res_in bit for bit against nalo_imm_resident_optimize(sel of the model).

  real shapes   K 1224x368 W=8, B 1920x1072 W=8, S 640x480 W=16 of test_imm_large_gpu.py's construction, the resident set shuffled so that hosts
                interleave, traced on the device over the two later frames, activated at currentMinActDist 0 / 0.3 / 1 / 2.5 / 4
  scale         2560x1280, 160 000 resident points over 8 hosts
  planted       hand-built states on a 640x48 level-1 map (selection only): dependency chains, storage order against key order, the corner C whose value
                depends on the history, border pixels, dist == th, currentMinActDist = 0, non-finite projections, empty / hopeless / single-point sets
  fused call    = selection-only call + nalo_imm_resident_optimize(sel); repeatable; the resident state is not modified
  errors        every NALO_ERR_STATE / NALO_ERR_ARG case of the header, and the context stays usable

What the inputs reach is asserted on the MODEL's output, before the device is asked. The counters of nalo_imm_activate_last are printed (-s); no test
asserts a round count (it depends on scheduling), only that the counts which do not (survivors, selected, rejected by an earlier point) are the model's."""
import numpy as np
import pytest

import activation_model as am
import orc
from imm_helpers import host_to_new
from nalo_slam_amd import binding, synth
from test_imm_large_gpu import CASES, Case, eq, fresh_state

pytestmark = pytest.mark.gpu

DISTS = (0.0, 0.3, 1.0, 2.5, 4.0)
FATES = (1, 0, 2, -1, -2, -3, 3)


def level1_maps(win, frame, yaw_deg=0.0):
    """KRKi [W,9], Kt [W,3] host -> frame at level 1, as activatePointsMT builds them (FullSystem.cpp:809-811). yaw_deg turns the newest keyframe: by the time
    points are activated the optimiser has moved the pose the frames were traced with. In the synthetic sequence every point moves outwards from one frame to
    the next, so with the traced poses no point that was traced inside the two later frames can project outside the keyframe before them; with the keyframe
    turned a few pixels, points near one border do (fate -3)."""
    fx, fy, cx, cy = [np.float32(x) for x in win.K]
    K1 = np.array([[fx * np.float32(0.5), 0, np.float32((cx + 0.5) / 2 - 0.5)], [0, fy * np.float32(0.5), np.float32((cy + 0.5) / 2 - 0.5)], [0, 0, 1]], np.float32)
    Ki0 = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float32)
    a = np.deg2rad(yaw_deg)
    Tf = synth.se3_mul(np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0]]), win.world_to_cam[frame])
    KRKi, Kt = np.zeros((win.W, 9), np.float32), np.zeros((win.W, 3), np.float32)
    for h in range(win.W):
        T = synth.se3_mul(Tf, synth.se3_inv(win.world_to_cam[h]))
        KRKi[h] = ((K1 @ T[:, :3].astype(np.float32)) @ Ki0).reshape(-1)
        Kt[h] = K1 @ T[:, 3].astype(np.float32)
    return KRKi, Kt


def check_stats(c, info, sel, tag):
    st = c.imm_activate_last()
    print("IMM-ACT %s survivors %d selected %d rejected by an earlier point %d rounds %d" % ((tag,) + st))
    assert st[:3] == (info["survivors"], len(sel), info["late"]) and (st[3] >= 1 or info["survivors"] == 0)
    return st


# ---------------------------------------------------------------------------------------------------------------- real shapes
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


def traced_resident_set(cs, seed):
    """the case's immature points, shuffled, resident, traced over the two later frames -> arrays + the device's state"""
    W = cs.W
    u, v, host = cs.points(CASES[cs.name]["per_host"], seed=seed, margin=3)
    color, weights, gradH, eth = cs.create(u, v, host)
    p = np.random.RandomState(seed + 7).permutation(len(u))
    u, v, host, color, weights, gradH, eth = [a[p] for a in (u, v, host, color, weights, gradH, eth)]
    assert (np.diff(host) != 0).sum() > len(u) // 2                           # hosts interleave in storage
    n = len(u)
    st = fresh_state(n)
    c = cs.c
    c.imm_resident_set(u.astype(np.float32), v.astype(np.float32), color, weights, gradH, eth, host, st["idmin"], st["idmax"], st["status"], st["quality"])
    for new in (W, W + 1):
        c.imm_resident_trace(int(cs.slot[new]), *host_to_new(cs.win, new, cs.aff, cs.exposure))
    my_type = np.random.RandomState(seed + 8).choice([1.0, 2.0, 4.0], n).astype(np.float32)
    c.imm_resident_set_type(my_type)
    return u.astype(np.float32), v.astype(np.float32), host, my_type, c.imm_resident_get()


@pytest.mark.parametrize("name,min_obs", [("K", 3), ("B", 3), ("S", 6)])
def test_real_shapes_exact(cases, name, min_obs):
    cs = cases(name)
    win, W, c = cs.win, cs.W, cs.c
    frame = W - 1
    u, v, host, my_type, state = traced_resident_set(cs, seed=4)
    idmin, idmax, status, quality, _, interval = state
    assert (host == frame).any()                                              # the newest keyframe hosts immature points too
    cs.set_window(synth.perturbed_poses(win, sigma_t=0.002, sigma_r=0.0002))
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    KRKi, Kt = level1_maps(win, frame, yaw_deg=2.5)
    D0 = orc.dist_make_map(win.w >> 1, win.h >> 1, frame, win.host, win.u, win.v, win.idepth, KRKi, Kt)
    flagged = np.zeros(W, np.int32); flagged[[1, W - 3]] = 1
    seen, shared = set(), 0
    for d in DISTS:
        fate, sel, info = am.select(D0, frame, host, u, v, idmin, idmax, status, quality, interval, my_type, KRKi, Kt, flagged, d)
        seen |= set(fate.tolist())
        shared = max(shared, info["max_per_pixel"])
        print("IMM-ACT %s n=%d minActDist %.1f fates %s survivors %d rejected by an earlier point %d (%.0f %%), most survivors on a pixel %d"
              % (name, len(u), d, {f: int((fate == f).sum()) for f in FATES}, info["survivors"], info["late"], 100.0 * info["late"] / max(info["survivors"], 1),
                 info["max_per_pixel"]))
        if d >= 1:
            assert info["late"] >= 0.05 * info["survivors"] > 0
        g_fate, g_sel, g_opt = c.imm_resident_activate(frame, KRKi, Kt, flagged, d, min_obs)
        assert np.array_equal(g_fate, fate) and np.array_equal(g_sel, sel), (name, d)
        check_stats(c, info, sel, "%s %.1f" % (name, d))
        for a, b in zip(g_opt, c.imm_resident_optimize(sel, min_obs)):
            assert eq(a, b), (name, d)
        assert set(g_opt[0].tolist()) <= {1, 0, -1} and (g_opt[0] == 1).sum() > 0
    assert seen == set(FATES), seen
    assert shared >= 2


# ---------------------------------------------------------------------------------------------------------------- hand-built states
class Planted:
    """a context whose level-1 map is w1 x h1 and whose host -> newest projection is (u, v) -> (u / 2, v / 2): a point at u = 2 U + 2 f, v = 2 V lands on
    pixel (U, V) with fraction f (0 <= f < 0.5). Images are flat: the selection never reads them."""

    def __init__(self, w1, h1, W):
        self.w1, self.h1, self.W = w1, h1, W
        self.c = binding.Context(2 * w1, 2 * h1, (100.0, 100.0, w1 - 0.5, h1 - 0.5), n_slots=W)
        for s in range(W):
            self.c.frame_upload(s, np.full((2 * h1, 2 * w1), 100, np.float32))
        self.KRKi = np.tile(np.array([0.5, 0, 0, 0, 0.5, 0, 0, 0, 1], np.float32), (W, 1))
        self.Kt = np.zeros((W, 3), np.float32)
        self.window()

    def window(self):
        T = np.tile(np.eye(4)[:3], (self.W, 1, 1))
        self.c.ba_set_window(list(range(self.W)), T)

    def seeds(self, px):
        """the window's active points: level-1 pixels [(U, V)], hosted by frame 0"""
        px = np.asarray(px, np.float32).reshape(-1, 2)
        n = len(px)
        self.act = (np.zeros(n, np.int32), 2 * px[:, 0], 2 * px[:, 1], np.ones(n, np.float32))
        self.c.ba_set_points(self.act[0], self.act[1], self.act[2], self.act[3], np.zeros((n, 8), np.float32), np.ones((n, 8), np.float32))
        return orc.dist_make_map(self.w1, self.h1, self.W - 1, *self.act, self.KRKi, self.Kt)

    def run(self, D0, U, V, host=None, my_type=None, dist=1.0, frac=None, status=None, idmin=None, idmax=None, quality=None, flagged=None, KRKi=None, tag=""):
        n = len(U)
        arr = lambda a, d, t: np.full(n, d, t) if a is None else np.asarray(a, t)
        u = 2 * np.asarray(U, np.float32) + 2 * arr(frac, 0, np.float32)
        v = 2 * np.asarray(V, np.float32)
        host, my_type, status = arr(host, 0, np.int32), arr(my_type, 1, np.float32), arr(status, am.GOOD, np.int32)
        idmin, idmax, quality = arr(idmin, 0.5, np.float32), arr(idmax, 1.5, np.float32), arr(quality, 10, np.float32)
        flagged = np.zeros(self.W, np.int32) if flagged is None else np.asarray(flagged, np.int32)
        KRKi = self.KRKi if KRKi is None else KRKi
        z = np.zeros((n, 8), np.float32)
        self.c.imm_resident_set(u, v, z, z, np.zeros((n, 3), np.float32), np.zeros(n, np.float32), host, idmin, idmax, status, quality)
        self.c.imm_resident_set_type(my_type)
        fate, sel, info = am.select(D0, self.W - 1, host, u, v, idmin, idmax, status, quality, np.zeros(n, np.float32), my_type, KRKi, self.Kt, flagged, dist)
        g_fate, g_sel = self.c.imm_resident_activate(self.W - 1, KRKi, self.Kt, flagged, dist)
        assert np.array_equal(g_fate, fate) and np.array_equal(g_sel, sel), (tag, g_fate.tolist(), fate.tolist())
        st = check_stats(self.c, info, sel, "planted " + tag) if n else None
        return fate, sel, info, st


@pytest.fixture(scope="module")
def planted():
    p = Planted(640, 48, 3)
    yield p
    p.c.close()


def test_planted_chains_and_order(planted):
    P = planted
    D0 = P.seeds(np.zeros((0, 2)))
    assert (D0 == 1000).all()
    # threshold 2: a point conflicts with the earlier points on its 8 neighbours. 600 points along a row: each depends on its predecessor alone
    n = 600
    U, V = np.arange(10, 10 + n), np.full(n, 20)
    fate, sel, info, st = P.run(D0, U, V, dist=2.0, tag="chain")
    assert np.array_equal(fate, np.where(np.arange(n) % 2 == 0, 1, 2)) and info["survivors"] == n
    print("IMM-ACT chain of %d: %d rounds (the first batch holds 12)" % (n, st[3]))
    # the same pixels stored in reverse: the loop starts from the other end, the outcome flips (n is even)
    fate_r, _, _, _ = P.run(D0, U[::-1], V, dist=2.0, tag="chain reversed")
    assert np.array_equal(fate_r[::-1], np.where(np.arange(n) % 2 == 1, 1, 2))
    # two hosts interleaved in storage, pairs on the same pixel, threshold 1: all of host 0 is decided before any of host 1
    m = 300
    Up, Vp = np.repeat(np.arange(10, 10 + 2 * m, 2), 2), np.full(2 * m, 30)
    host = np.tile([1, 0], m)
    fate, sel, _, _ = P.run(D0, Up, Vp, host=host, dist=1.0, tag="two hosts")
    assert (fate[host == 0] == 1).all() and (fate[host == 1] == 2).all() and np.array_equal(sel, np.arange(1, 2 * m, 2))
    # both chains at once in two rows three pixels apart (no interaction across rows at threshold 2), hosts alternating along the row:
    # host 0's points are all accepted (they are two apart), host 1's all rejected
    host = (np.arange(n) % 2).astype(np.int32)[::-1].copy()
    fate, _, _, _ = P.run(D0, U, V, host=host, dist=2.0, tag="chain by host")
    assert (fate[host == 0] == 1).all() and (fate[host == 1] == 2).all()


def test_planted_corner_depends_on_history(planted):
    """C = (w1-1, h1-1) is entered only diagonally from I = (w1-2, h1-2), on an odd level: an acceptance that lowers D(I) to an even v leaves v + 1 on C,
    and a later one that lowers D(I) further to an odd value does not take that back (the from-scratch map of the same seeds would)."""
    P = planted
    w1, h1 = P.w1, P.h1
    C, I = (w1 - 1, h1 - 1), (w1 - 2, h1 - 2)
    D0 = P.seeds(np.zeros((0, 2)))
    two, one = (I[0] - 2, I[1]), (I[0] - 1, I[1])                             # delta(., I) = 2 and 1
    typ = [1, 1, 4]                                                           # threshold 1 for the helpers (accepted: nobody is on their pixel), 4 for C

    def on_C(first, second, tag):
        fate, _, info, _ = P.run(D0, [first[0], second[0], C[0]], [first[1], second[1], C[1]], my_type=typ, dist=1.0, tag=tag)
        assert fate[0] == 1 and fate[1] == 1
        return fate[2], info["D"]
    f, D = on_C(two, one, "C: I to 2, then to 1")
    assert f == 2 and D[C[1], C[0]] == 3 and D[I[1], I[0]] == 1                # the literal map keeps the 3 ...
    scratch = orc.dist_make_map(w1, h1, P.W - 1, np.zeros(2, np.int32), 2 * np.float32([two[0], one[0]]), 2 * np.float32([two[1], one[1]]), np.ones(2, np.float32), P.KRKi, P.Kt)
    assert scratch[C[1], C[0]] == 1000                                         # ... which the from-scratch map of the same two seeds does not have
    f, D = on_C(one, two, "C: I to 1, then nothing")
    assert f == 1 and D[I[1], I[0]] == 1
    f, _ = on_C(I, two, "C: I seeded")                                         # I = 0 -> C = 1 < 4
    assert f == 2
    f, _ = on_C((I[0] - 3, I[1]), (I[0] - 3, I[1] - 4), "C: I to 3")            # odd: nothing reaches C
    assert f == 1
    f, _ = on_C((I[0] - 4, I[1]), (I[0] - 9, I[1]), "C: I to 4")                # C = 5 >= 4
    assert f == 1
    # C against an active seed's map: D0(I) = 2 already, an acceptance at distance 2 of I lowers nothing; and two candidates on C itself
    D1 = P.seeds([two])
    assert D1[I[1], I[0]] == 2 and D1[C[1], C[0]] == 3
    fate, _, _, _ = P.run(D1, [I[0], C[0], C[0]], [I[1] - 2, C[1], C[1]], my_type=[1, 2, 1], dist=1.5, tag="C: D0 = 3")
    assert fate.tolist() == [1, 1, 2]                                          # 3 >= 3 selected; the second one on C finds 0


def test_planted_borders_thresholds_and_degenerate_inputs(planted):
    P = planted
    w1, h1 = P.w1, P.h1
    # seeds ON the right and bottom border never expand: the pixels beside them stay at 1000; candidates on border pixels are selected and do not expand either
    D0 = P.seeds([(w1 - 1, 10), (100, h1 - 1), (300, 20)])
    assert D0[10, w1 - 2] == 1000 and D0[h1 - 2, 100] == 1000 and D0[20, 301] == 1
    U = [w1 - 2, w1 - 1, w1 - 1, w1 - 2, w1 - 1, 100, 200, 200, 201, 200, w1 - 3, w1 - 1, w1 - 1]
    V = [10, 10, 30, 30, 31, h1 - 2, h1 - 1, h1 - 2, h1 - 1, h1 - 3, 40, 42, 41]
    fate, _, _, _ = P.run(D0, U, V, dist=3.0, tag="borders")
    # beside a border seed: free; on it: 0; a free border pixel; beside that accepted border point: still free (it did not expand); the border pixel diagonal
    # to that interior acceptance: 1 < 3. The same along the bottom border, and the interior pixel above.
    assert fate[:5].tolist() == [1, 2, 1, 1, 2] and fate[5:10].tolist() == [1, 1, 1, 2, 2]
    # an interior acceptance reaches a border pixel through interior neighbours only: (w1-3, 40) -> (w1-1, 42) takes 3 steps, not 2
    assert fate[10] == 1 and fate[11] == 1 and fate[12] == 2
    # dist == th on both sides of >=, fraction 0: D0 = 2 two pixels from the seed
    assert D0[20, 302] == 2 and D0[20, 303] == 3
    fate, _, _, _ = P.run(D0, [302, 301, 303, 305], [20, 20, 20, 20], my_type=[2, 2, 4, 4], dist=1.0, frac=[0, 0, 0, 0.25], tag="dist == th")
    assert fate.tolist() == [1, 2, 2, 2]                                       # 2 >= 2; 1 < 2; 3 < 4; 5.25 >= 4 on the initial map but 3.25 < 4 once (302, 20) is in
    fate, _, _, _ = P.run(D0, [302, 303, 303], [20, 20, 24], my_type=[4, 4, 4], dist=0.75, frac=[0, 0, 0.25], tag="3 >= 3")
    assert fate[0] == 2 and fate[1] == 1
    # currentMinActDist = 0: everything that projects into the image is selected, on D = 0 too
    fate, sel, _, _ = P.run(D0, [300, 300, 301, w1 - 1, 1, 0, 5], [20, 20, 20, h1 - 1, 1, 5, 0], my_type=[1, 2, 4, 4, 1, 1, 1], dist=0.0, tag="zero")
    assert fate.tolist() == [1, 1, 1, 1, 1, -3, -3] and sel.tolist() == [0, 1, 2, 3, 4]
    # non-finite values: ptp[2] = 0 and a NaN row for the points of host 1 (-3), NaN / inf depth bounds (-1, or not ready: 0 / -2), OUTLIER, and the newest frame
    K2 = P.KRKi.copy(); K2[1, 6:] = 0
    fate, _, _, _ = P.run(D0, [50] * 8, [10] * 8, host=[1, 0, 0, 0, 0, 2, 0, 1], idmax=[1.5, np.nan, np.inf, 1.5, 1.5, 1.5, 1.5, 1.5],
                          idmin=[0.5, 0.5, 0.5, np.nan, -2, 0.5, 0.5, 0.5], status=[0, 0, 0, 0, am.OOB, 0, am.OUTLIER, am.UNINITIALIZED], KRKi=K2, flagged=[0, 1, 0], tag="non-finite")
    assert fate.tolist() == [-3, -1, -1, 0, -2, 3, -1, -2]
    K3 = P.KRKi.copy(); K3[1, 0] = np.nan
    fate, _, _, _ = P.run(D0, [50, 60], [10, 10], host=[1, 0], KRKi=K3, tag="NaN row")
    assert fate.tolist() == [-3, 1]
    # no survivor at all, one point, no point
    fate, sel, info, _ = P.run(D0, [300] * 40, [20] * 40, dist=1.0, tag="no survivor")
    assert (fate == 2).all() and len(sel) == 0 and info["survivors"] == 0
    fate, sel, _, _ = P.run(D0, [310], [20], dist=4.0, my_type=[2], tag="n = 1")
    assert fate.tolist() == [1]
    fate, sel, _, _ = P.run(D0, [], [], tag="empty")
    assert len(fate) == 0 and len(sel) == 0


# ---------------------------------------------------------------------------------------------------------------- scale
def test_scale_exact():
    """1280x640 at level 1, 160 000 resident points over 8 hosts against 8000 active points, random states"""
    w1, h1, W, n, na = 1280, 640, 8, 160000, 8000
    P = Planted(w1, h1, W)
    try:
        rng = np.random.RandomState(12)
        D0 = P.seeds(np.stack([rng.randint(1, w1, na), rng.randint(1, h1, na)], 1))
        U, V = rng.randint(-2, w1 + 2, n), rng.randint(-2, h1 + 2, n)
        host = rng.randint(0, W, n)
        status = rng.choice([am.GOOD, am.GOOD, am.GOOD, am.SKIPPED, am.BADCONDITION, am.OOB, am.OUTLIER, am.UNINITIALIZED], n)
        quality = rng.choice([10.0, 10.0, 10.0, 2.0], n)
        idmax = np.where(rng.rand(n) < 0.03, np.nan, 1.5)
        flagged = np.zeros(W, np.int32); flagged[[2, 5]] = 1
        fate, sel, info, st = P.run(D0, U, V, host=host, my_type=rng.choice([1.0, 2.0, 4.0], n), dist=2.5, frac=rng.choice([0, 0.125, 0.25, 0.4375], n), status=status,
                                    quality=quality, idmax=idmax, flagged=flagged, tag="scale")
        assert set(fate.tolist()) == set(FATES) and info["late"] >= 0.05 * info["survivors"] and info["max_per_pixel"] >= 2
    finally:
        P.c.close()


# ---------------------------------------------------------------------------------------------------------------- the fused call, errors
def test_fused_call_equals_its_parts_and_leaves_no_state(cases):
    cs = cases("K")
    win, W, c = cs.win, cs.W, cs.c
    frame = W - 1
    traced_resident_set(cs, seed=5)
    before = c.imm_resident_get()
    cs.set_window(synth.perturbed_poses(win, sigma_t=0.002, sigma_r=0.0002))
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    KRKi, Kt = level1_maps(win, frame)
    flagged = np.zeros(W, np.int32)
    fate, sel, opt = c.imm_resident_activate(frame, KRKi, Kt, flagged, 1.0, 3)
    st = c.imm_activate_last()
    fate2, sel2 = c.imm_resident_activate(frame, KRKi, Kt, flagged, 1.0)
    assert np.array_equal(fate, fate2) and np.array_equal(sel, sel2) and c.imm_activate_last()[:3] == st[:3] and len(sel) > 100
    for a, b in zip(opt, c.imm_resident_optimize(sel, 3)):
        assert eq(a, b)
    fate3, sel3, opt3 = c.imm_resident_activate(frame, KRKi, Kt, flagged, 1.0, 3)
    assert np.array_equal(fate, fate3) and np.array_equal(sel, sel3) and all(eq(a, b) for a, b in zip(opt, opt3))
    for a, b in zip(before, c.imm_resident_get()):
        assert eq(a, b)


def test_errors_and_the_context_stays_usable(planted):
    P = planted
    c, W = P.c, P.W
    D0 = P.seeds([(300, 20)])
    ok = lambda: P.run(D0, [310, 311], [20, 20], dist=2.0, tag="after an error")[0].tolist() == [1, 2]
    assert ok()
    fl = np.zeros(W, np.int32)

    def fails(code, f):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % code):
            f()
        assert ok()
    STATE, ARG = -4, -1
    fails(ARG, lambda: c.imm_resident_activate(W, P.KRKi, P.Kt, fl, 1.0))                      # frame outside the window
    fails(ARG, lambda: c.imm_resident_activate(-1, P.KRKi, P.Kt, fl, 1.0))
    fails(ARG, lambda: c.imm_resident_activate(W - 1, P.KRKi, P.Kt, fl, -0.5))
    fails(ARG, lambda: c.imm_resident_activate(W - 1, P.KRKi, P.Kt, fl, float("nan")))
    fails(ARG, lambda: c.imm_resident_activate(W - 1, P.KRKi, P.Kt, fl, float("inf")))
    fails(ARG, lambda: c.imm_resident_activate(W - 1, P.KRKi, P.Kt, fl, 16.5))                  # 16.5 * my_type 1 > 16: refused
    L, n = c.L, c._imm_n
    fate, sel, ns = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.int32)
    res = np.zeros(n, np.int32)
    I, F = binding._i, binding._f
    fails(ARG, lambda: c._ck(L.nalo_imm_resident_activate(c.h_, W - 1, None, F(P.Kt), I(fl), 1.0, 1, I(fate), I(ns), I(sel), None, None, None)))
    fails(ARG, lambda: c._ck(L.nalo_imm_resident_activate(c.h_, W - 1, F(P.KRKi), F(P.Kt), I(fl), 1.0, 1, None, I(ns), I(sel), None, None, None)))
    fails(ARG, lambda: c._ck(L.nalo_imm_resident_activate(c.h_, W - 1, F(P.KRKi), F(P.Kt), I(fl), 1.0, 1, I(fate), I(ns), I(sel), I(res), None, None)))   # outputs: all three or none
    fails(ARG, lambda: c.imm_resident_set_type(np.array([1, np.nan], np.float32)))
    # a new resident set has no types until they are given
    z = np.zeros((2, 8), np.float32)
    c.imm_resident_set(np.float32([620, 622]), np.float32([40, 40]), z, z, np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.zeros(2, np.int32),
                       np.float32([0.5, 0.5]), np.float32([1.5, 1.5]), np.zeros(2, np.int32), np.float32([10, 10]))
    fails(STATE, lambda: c.imm_resident_activate(W - 1, P.KRKi, P.Kt, fl, 1.0))
    # a resident host index outside the window
    c.imm_resident_set(np.float32([620, 622]), np.float32([40, 40]), z, z, np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.int32([0, W]),
                       np.float32([0.5, 0.5]), np.float32([1.5, 1.5]), np.zeros(2, np.int32), np.float32([10, 10]))
    c.imm_resident_set_type(np.ones(2, np.float32))
    fails(STATE, lambda: c.imm_resident_activate(W - 1, P.KRKi, P.Kt, fl, 1.0))
    # a sharded window holds only part of the seeds
    c.ba_set_allreduce(lambda ptr, n: None)
    try:
        with pytest.raises(binding.NaloError, match="nalo error -4:"):
            c.imm_resident_activate(W - 1, P.KRKi, P.Kt, fl, 1.0)
    finally:
        c.ba_set_allreduce(None)
    assert ok()
    # no window, no points
    c2 = binding.Context(160, 128, (100.0, 100.0, 79.5, 63.5), n_slots=3)                      # 80x64 at level 1 (a frame without a level 1 is NALO_ERR_ARG)
    try:
        c2.imm_resident_set(np.float32([20]), np.float32([20]), z[:1], z[:1], np.zeros((1, 3), np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32),
                            np.float32([0.5]), np.float32([1.5]), np.zeros(1, np.int32), np.float32([10]))
        c2.imm_resident_set_type(np.ones(1, np.float32))
        k, t = P.KRKi, P.Kt
        with pytest.raises(binding.NaloError, match="nalo error -4:"):
            c2.imm_resident_activate(2, k, t, fl, 1.0)                         # no window
        for s in range(3):
            c2.frame_upload(s, np.full((128, 160), 100, np.float32))
        c2.ba_set_window([0, 1, 2], np.tile(np.eye(4)[:3], (3, 1, 1)))
        with pytest.raises(binding.NaloError, match="nalo error -4:"):
            c2.imm_resident_activate(2, k, t, fl, 1.0)                         # a window without points
        c2.ba_set_points(np.zeros(1, np.int32), np.float32([10]), np.float32([10]), np.ones(1, np.float32), np.zeros((1, 8), np.float32), np.ones((1, 8), np.float32))
        fate, sel = c2.imm_resident_activate(2, k, t, fl, 1.0)
        assert fate.tolist() == [1] and sel.tolist() == [0]
    finally:
        c2.close()
