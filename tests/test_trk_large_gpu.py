"""The tracker's persistent LM kernel and its reference build at full-size point clouds, against the oracle (fp32 and fp64).

trk_lm_kernel (kernels_trk_lm.hip) changes shape with the cloud: NB = min(max_blocks, ceil(maxn / 512)) workgroups of 512 lanes, max_blocks = 64, or 128 once the
largest level holds 8 x 64 x 512 = 262 144 points; a level of n <= NB x 512 points is loaded once and kept in registers (one round), a larger one is walked in
rounds of NB x 512 points, the last one ragged. test_tracker_gpu.py stays at one round on a few workgroups. Each shape here asserts, through
nalo_trk_get_launch_config, the variant it is for, so that a retuned threshold fails the test instead of quietly testing the small path again:

  id  frame      cloud                                       workgroups  rounds per level 0..4   driver
  K1  1224x368   trk_set_ref, 6 k inputs                     < 64        1 1 1 1 (1)             persistent   (a partly filled grid)
  B1  1920x1072  trk_set_pc, level 0 = 32 768 points         64          1 1 1 1 1               persistent   (every lane holds a point)
  B2  1920x1072  level 0 = 32 769 points                     64          2 1 1 1 1               persistent   (the second round holds one point)
  M1  1920x1072  trk_set_ref, 60 k inputs                    128         5 4 2 1 1               persistent   (*)
  W1  1920x1072  level 0 = 262 143 points                    64          8 2 1 1 1               persistent
  W2  1920x1072  level 0 = 262 144 points                    128         4 1 1 1 1               persistent
  X1  1920x1072  trk_set_ref, 900 k inputs (config-5-sized)  128         >= 10, ragged            persistent   (its scatter list: ~67 k residuals)
(trk_set_pc shapes: every level gets a seeded cloud at its resolution, level l of n0 / 4^l points.)
(*) the cloud of test_fullsize_gpu.py::test_track_round_trip_full_size: the dilation grows its 60 k inputs to 279 k level-0 points, so it runs on 128
    workgroups with three streamed levels; B2 and W1 are the streamed 64-workgroup shapes.

The new frame is not a re-rendering of the reference: it is s I + o with s = 1.15, o = -6, exposures (1, 1.1), plus seeded Gaussian noise (sigma 2) and 1 % of
pixels off by +-40 grey levels. The optimum then depends on the Huber weights and on the affine pair, so a weighting or summation error moves the answer.

Per shape, against the fp32 oracle (orc_set_sum_mode(0)) and the all-fp64 oracle on the same float inputs:
  1  ok equals the fp32 oracle's
  2  the evaluations per level (nalo_trk_last_evals) and n_evals equal the fp32 oracle's (no shape needs an allowance)
  3  pose within 1e-5 of the fp32 oracle (BASELINE's bar); 4  no farther from the fp64 oracle than 1.5x the fp32 oracle's distance + 1e-6
  5  affine pair within 1e-3 of the fp32 oracle
  6  lastResiduals of every level run and the flow indicators as close to the fp64 oracle as the fp32 oracle is (1.5x + 4e-6 relative: the GPU and the
     fp32 oracle both scatter 0 to 2.6e-6 from fp64 on these; lastResiduals is the sqrtf of an fp32 ratio, so the oracle sometimes lands on fp64's value)
  7  printed: the final level's energy (lastResiduals[0]) distance to fp64 of the GPU and of the fp32 oracle - the precision of the fp32 partial exchange
Control flow at 128 workgroups (W2): the cutoff-repeat loop with the haveRepeated re-run, minResForAbort stopping at level 1, the affine range check; the
partials buffer reused across launches of another grid size; the host-driven loop (after an injected lost launch). The reference build: point clouds and depth maps of
M1 and X1 bit for bit, and a scatter list longer than the fix pass's LDS copy."""
import functools

import numpy as np
import pytest

import orc
from helpers import pose_dist, tracker_inputs, true_rel_pose
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

SHAPES = {
    "K1": dict(w=1224, h=368, ref=6000, expect=dict(nblocks=lambda nb: nb < 64, rounds=lambda r: max(r) == 1)),
    "B1": dict(pc=32768, expect=dict(nblocks=64, rounds=[1, 1, 1, 1, 1])),
    "B2": dict(pc=32769, expect=dict(nblocks=64, rounds=[2, 1, 1, 1, 1])),
    "M1": dict(ref=60000, expect=dict(nblocks=128, rounds=[5, 4, 2, 1, 1])),
    "W1": dict(pc=262143, expect=dict(nblocks=64, rounds=[8, 2, 1, 1, 1])),
    "W2": dict(pc=262144, expect=dict(nblocks=128, rounds=[4, 1, 1, 1, 1])),
    "X1": dict(ref=900000, expect=dict(nblocks=128, rounds=lambda r: r[0] >= 10)),
}
EXPOSURES = [1.0, 1.1]
POSE_FLOOR, REL_FLOOR = 1e-6, 4e-6
_SHAPES_OPEN = []


@functools.lru_cache(maxsize=None)
def frames(w, h):
    """reference image, new image (s I + o + noise + outliers), depth of the reference, true pose ref -> new"""
    win = synth.make_window(w=w, h=h, W=1, P=16, seed=11, n_extra=1)
    rng = np.random.RandomState(23)
    new = 1.15 * win.images[1] - 6.0 + rng.normal(0, 2.0, win.images[1].shape)
    out = rng.rand(*new.shape) < 0.01
    new[out] += rng.choice([-40.0, 40.0], out.sum())
    return win, new.astype(np.float32)


def pc_clouds(win, dI_ref, levels, n0, seed):
    """a seeded cloud per level at the level's resolution, raster order: level l holds n0 / 4^l points"""
    rng = np.random.RandomState(seed)
    L = orc.lib()
    out = []
    for l in range(levels):
        wl, hl = win.w >> l, win.h >> l
        uu, vv = np.meshgrid(np.arange(2, wl - 3), np.arange(2, hl - 3))
        uu, vv = uu.ravel(), vv.ravel()
        d = win.depth[0][vv << l, uu << l]
        ok = np.isfinite(d) & (d > 0)
        uu, vv, d = uu[ok], vv[ok], d[ok]
        n = min(max(n0 >> (2 * l), 1), len(uu))
        k = np.sort(rng.choice(len(uu), n, replace=False))
        u, v = uu[k], vv[k]
        o = L.orc_pyr_offset(win.w, win.h, l)
        col = dI_ref[o + v * wl + u, 0]
        out.append((u.astype(np.float32), v.astype(np.float32), (1.0 / d[k]).astype(np.float32), col.astype(np.float32)))
    return out


class Shape:
    def __init__(self, name):
        s = SHAPES[name]
        self.name = name
        self.win, self.new = frames(s.get("w", 1920), s.get("h", 1072))
        win = self.win
        self.ctx = binding.Context(win.w, win.h, win.K, n_slots=2)
        _SHAPES_OPEN.append(self)
        self.levels = self.ctx.levels
        self.ctx.frame_upload(0, win.images[0]); self.ctx.frame_upload(1, self.new)
        self.dI_ref, _ = orc.make_images(win.images[0], self.levels)
        self.dI_new, _ = orc.make_images(self.new, self.levels)
        self.Ttrue = true_rel_pose(win, 0, 1)
        self.T0 = orc.se3_exp(orc.se3_log(self.Ttrue) * 0.9)
        self.oracles = {}
        if "ref" in s:
            self.inputs = tracker_inputs(win, n=s["ref"], seed=3)
            self.ctx.trk_set_ref(0, *self.inputs)
        else:
            self.inputs = None
            self.clouds = pc_clouds(win, self.dI_ref, self.levels, s["pc"], seed=5)
            self.set_pc(self.ctx)

    def set_pc(self, c):
        for l, pc in enumerate(self.clouds):
            c.trk_set_pc(0, l, *pc)

    def oracle(self, kind):
        if kind not in self.oracles:
            trk = orc.Tracker(self.win.w, self.win.h, self.levels, self.win.K, kind)
            if self.inputs is not None:
                trk.set_ref(self.dI_ref, *self.inputs)
            else:
                for l, pc in enumerate(self.clouds):
                    trk.set_pc(self.dI_ref, l, *pc)
            self.oracles[kind] = trk
        return self.oracles[kind]

    def track_oracle(self, kind, aff0=(0, 0), ref_aff=(0, 0), min_res=None, new=None):
        orc.lib("f32").orc_set_sum_mode(0)
        trk = self.oracle(kind)
        dI_new = self.dI_new if new is None else orc.make_images(new, self.levels)[0]
        ok, T, aff, lr, lf = trk.track(dI_new, self.T0, aff0, ref_aff, EXPOSURES, self.levels - 1, min_res=min_res)
        ev, rep = trk.last_evals()
        return dict(ok=ok, T=T, aff=aff, lr=lr, lf=lf, ev=ev, nev=int(ev.sum()), rep=rep)

    def track_gpu(self, c=None, aff0=(0, 0), ref_aff=(0, 0), min_res=None):
        c = c or self.ctx
        ok, T, aff, lr, lf, nev = c.trk_track(1, self.T0, aff0, ref_aff, EXPOSURES, self.levels - 1, min_res=min_res)
        ev, n = c.trk_last_evals()
        return dict(ok=ok, T=T, aff=aff, lr=lr, lf=lf, ev=ev, nev=nev, n=n, cfg=c.trk_launch_config())


@functools.lru_cache(maxsize=None)
def shape(name):
    return Shape(name)


@pytest.fixture(scope="module", autouse=True)
def _close_shapes():
    yield
    for s in list(_SHAPES_OPEN):
        s.ctx.close()
    _SHAPES_OPEN.clear()
    shape.cache_clear()


def check_variant(name, cfg, n):
    exp = SHAPES[name]["expect"]
    assert cfg["driver"] == 1 and cfg["lanes"] == 512, cfg
    for k, want in exp.items():
        got = cfg[k] if k != "rounds" else cfg["rounds"][:len(n)]
        if isinstance(want, list):
            want = want[:len(got)]
        assert want(got) if callable(want) else got == want, (name, k, cfg, list(n))
    nb = cfg["nblocks"]
    assert nb == min(128 if max(n) >= 262144 else 64, -(-max(n) // 512)), (cfg, list(n))
    assert cfg["rounds"] == [-(-int(x) // (nb * 512)) if l < len(n) else 0 for l, x in enumerate(list(n) + [0] * (5 - len(n)))], (cfg, list(n))


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b) / np.maximum(np.abs(b), 1e-300)


def compare(g, o32, o64, levels_run, tag=""):
    """checks 1-7 of the header for one track; prints the distances"""
    assert g["ok"] == o32["ok"], (tag, g["ok"], o32["ok"])
    assert list(g["ev"]) == list(o32["ev"]) and g["nev"] == o32["nev"], (tag, list(g["ev"]), list(o32["ev"]), list(o64["ev"]))
    d_g, d_32, d_g64 = pose_dist(g["T"], o32["T"]), pose_dist(o32["T"], o64["T"]), pose_dist(g["T"], o64["T"])
    e_g, e_32 = rel(g["lr"][0], o64["lr"][0]), rel(o32["lr"][0], o64["lr"][0])
    print("%s: evals %s | pose gpu-o32 %.2e, gpu-o64 %.2e, o32-o64 %.2e | lastRes[0] to fp64: gpu %.2e, o32 %.2e | aff %s"
          % (tag, list(g["ev"]), d_g, d_g64, d_32, e_g, e_32, np.asarray(g["aff"]).round(5)))
    assert d_g < 1e-5, (tag, d_g)
    assert d_g64 <= 1.5 * d_32 + POSE_FLOOR, (tag, d_g64, d_32)
    assert np.abs(np.asarray(g["aff"]) - o32["aff"]).max() < 1e-3, (tag, g["aff"], o32["aff"])
    lv = list(levels_run)
    for key, idx in (("lr", lv), ("lf", [0, 1, 2])):
        mine, ref = rel(g[key][idx], o64[key][idx]), rel(o32[key][idx], o64[key][idx])
        assert (mine <= 1.5 * ref + REL_FLOOR).all(), (tag, key, mine, ref)
    for l in range(5):
        if l not in lv:
            assert np.isnan(g["lr"][l]) and np.isnan(o32["lr"][l]), (tag, l)


@pytest.mark.parametrize("name", list(SHAPES))
def test_track_matches_oracles(name):
    s = shape(name)
    g = s.track_gpu()
    check_variant(name, g["cfg"], g["n"][:s.levels])
    o32, o64 = s.track_oracle("f32"), s.track_oracle("f64")
    assert o32["ok"] == 1 and not o32["rep"] and g["cfg"]["have_repeated"] == 0
    compare(g, o32, o64, range(s.levels), name)
    assert pose_dist(g["T"], s.Ttrue) < 5e-3                                    # and the noisy, brightened frame is still tracked


def test_cutoff_repeat_and_rerun_at_128_workgroups():
    """a brightness jump of +45 grey levels the start estimate does not know saturates the coarsest level's residuals: the cutoff-repeat loop runs, then the
    haveRepeated re-run of that level - both oracles and the GPU report the re-run, with the same evaluation counts"""
    s = shape("W2")
    c = s.ctx
    jump = (s.new + 45.0).astype(np.float32)
    c.frame_upload(1, jump)
    try:
        g = s.track_gpu()
    finally:
        c.frame_upload(1, s.new)
    assert g["cfg"]["nblocks"] == 128 and g["cfg"]["have_repeated"] == 1, g["cfg"]
    o32, o64 = s.track_oracle("f32", new=jump), s.track_oracle("f64", new=jump)
    assert o32["rep"] and o64["rep"]
    top = s.levels - 1
    assert o32["ev"][top] >= 6, o32["ev"]                                     # cutoff doubled at least twice on the first run of the level
    compare(g, o32, o64, range(s.levels), "W2 +45")


def test_min_res_abort_at_level_1_at_128_workgroups():
    """minResForAbort that only level 1 fails: ok = 0, pose and affine pair untouched, lastResiduals of levels top..1 as the oracle's, level 0 never run"""
    s = shape("W2")
    ref = s.track_oracle("f32")
    mr = np.full(5, 1e9)
    mr[1] = 0.5 * ref["lr"][1]
    g = s.track_gpu(min_res=mr)
    o32, o64 = s.track_oracle("f32", min_res=mr), s.track_oracle("f64", min_res=mr)
    assert g["ok"] == o32["ok"] == o64["ok"] == 0
    assert np.array_equal(g["T"], np.asarray(s.T0).reshape(3, 4)) and np.array_equal(g["aff"], [0, 0])
    assert list(g["ev"]) == list(o32["ev"]) and g["ev"][0] == 0 and g["nev"] == o32["nev"], (list(g["ev"]), list(o32["ev"]))
    lv = range(1, s.levels)
    mine, r32 = rel(g["lr"][lv], o64["lr"][lv]), rel(o32["lr"][lv], o64["lr"][lv])
    assert (mine <= 1.5 * r32 + REL_FLOOR).all() and np.isnan(g["lr"][0]), (mine, r32, g["lr"])
    print("W2 abort: evals %s, lastRes %s" % (list(g["ev"]), g["lr"]))


def test_affine_range_check_at_128_workgroups():
    """|a| > 1.2: the tracker returns false with the pose written (CoarseTracker.cpp:1243-1245), like the oracle"""
    s = shape("W2")
    aff0 = ref_aff = (1.3, 0.0)
    g = s.track_gpu(aff0=aff0, ref_aff=ref_aff)
    o32, o64 = s.track_oracle("f32", aff0=aff0, ref_aff=ref_aff), s.track_oracle("f64", aff0=aff0, ref_aff=ref_aff)
    assert g["ok"] == o32["ok"] == 0 and abs(g["aff"][0]) > 1.2
    assert not np.array_equal(g["T"], np.asarray(s.T0).reshape(3, 4))         # written
    o32["ok"] = o64["ok"] = g["ok"]
    compare(g, o32, o64, range(s.levels), "W2 range")


def test_repeated_tracks_reuse_the_partials_buffer():
    """one context: three 128-workgroup tracks with a small-cloud track (another grid size, stale tags in the partials buffer) between them - every output
    bit-identical across the three and equal to a fresh context's"""
    s, k = shape("W2"), shape("B1")
    c = binding.Context(s.win.w, s.win.h, s.win.K, n_slots=2)
    c.frame_upload(0, s.win.images[0]); c.frame_upload(1, s.new)
    runs = []
    for _ in range(3):
        s.set_pc(c)
        runs.append(s.track_gpu(c))
        k.set_pc(c)
        small = s.track_gpu(c)
        assert small["cfg"]["nblocks"] == 64 and small["ok"] == 1
    c.close()
    fresh = s.track_gpu()
    for r in runs:
        assert r["cfg"]["nblocks"] == 128
        for key in ("ok", "nev"):
            assert r[key] == fresh[key], key
        for key in ("T", "aff", "lr", "lf", "ev"):
            assert np.array_equal(np.asarray(r[key]), np.asarray(fresh[key]), equal_nan=True), key


def test_host_driven_loop_at_128_workgroups():
    """a context of its own whose first launch is reported lost (nalo_test_inject; the latch must not reach the shared one): the host-driven loop on W2 reaches
    the persistent kernel's pose within 1e-5 with the same evaluation counts"""
    s = shape("W2")
    g = s.track_gpu()
    c = binding.Context(s.win.w, s.win.h, s.win.K, n_slots=2)
    c.frame_upload(0, s.win.images[0]); c.frame_upload(1, s.new)
    s.set_pc(c)
    c.test_inject(binding.INJECT_LM_LOST_BLOCK)
    r = s.track_gpu(c)
    c.close()
    assert r["cfg"]["driver"] == 2 and r["ok"] == g["ok"] == 1
    assert pose_dist(r["T"], g["T"]) < 1e-5 and np.abs(r["aff"] - g["aff"]).max() < 1e-3
    assert r["nev"] == g["nev"] and list(r["ev"]) == list(g["ev"]), (list(r["ev"]), list(g["ev"]))


def assert_ref_build_equal(c, trk, levels, tag):
    for l in range(levels):
        a, b = trk.get_pc(l), c.trk_get_pc(l)
        da, db = trk.get_depth(l), c.trk_get_depth(l)
        print("%s level %d: n %d/%d, pc equal %s, depth equal %s" % (tag, l, len(a[0]), len(b[0]), [np.array_equal(x, y) for x, y in zip(a, b)] if len(a[0]) == len(b[0]) else "-",
                                                                   [np.array_equal(da[0], db[0]), np.array_equal(da[1], db[1])]))
    for l in range(levels):
        a, b = trk.get_pc(l), c.trk_get_pc(l)
        assert len(a[0]) == len(b[0]) > 0, (tag, l)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (tag, l)
        da, db = trk.get_depth(l), c.trk_get_depth(l)
        assert np.array_equal(da[0], db[0]) and np.array_equal(da[1], db[1]), (tag, l)


@pytest.mark.parametrize("name", ["M1", "X1"])
def test_reference_build_bit_exact_full_size(name):
    """makeCoarseDepthL0 at full size: every level's point cloud and depth map equal the oracle's bit for bit, over three builds (X1's 900 k inputs put ~67 k
    residuals on pixels with 3+ hits: the fix pass runs from the global list)"""
    s = shape(name)
    trk = s.oracle("f32")
    for rep in range(3):
        s.ctx.trk_set_ref(0, *s.inputs)
        assert_ref_build_equal(s.ctx, trk, s.levels, "%s build %d" % (name, rep))


def test_scatter_list_longer_than_the_lds_copy():
    """2 000 pixels with 3-5 hits each (~8 000 listed residuals, more than the fix pass's 4 096-entry LDS copy), inverse depths over three decades, random input
    order: level 0's idepth / weightSums and every level's cloud equal the oracle's bit for bit, three builds in a row"""
    win, _ = frames(1920, 1072)
    rng = np.random.RandomState(17)
    Ku, Kv, nid, hdi = tracker_inputs(win, n=20000, seed=4)
    npx = 2000
    pix = rng.choice((win.w - 40) * (win.h - 40), npx, replace=False)
    hot_u, hot_v = 20 + pix % (win.w - 40), 20 + pix // (win.w - 40)
    reps = rng.randint(3, 6, npx)
    eu = np.concatenate([np.full(r, u) + rng.uniform(-0.45, 0.45, r) for u, r in zip(hot_u, reps)]).astype(np.float32)
    ev = np.concatenate([np.full(r, v) + rng.uniform(-0.45, 0.45, r) for v, r in zip(hot_v, reps)]).astype(np.float32)
    en = (10.0 ** rng.uniform(-2.5, 0.5, len(eu))).astype(np.float32)
    eh = (10.0 ** rng.uniform(-7, -2, len(eu))).astype(np.float32)
    perm = rng.permutation(len(Ku) + len(eu))
    Ku, Kv, nid, hdi = [np.concatenate([a, b])[perm] for a, b in ((Ku, eu), (Kv, ev), (nid, en), (hdi, eh))]
    p = (Ku + 0.5).astype(np.int64) + win.w * (Kv + 0.5).astype(np.int64)
    cnt = np.bincount(p, minlength=win.w * win.h)
    assert cnt[cnt >= 3].sum() > 4096 * 1.5
    c = binding.Context(win.w, win.h, win.K, n_slots=1)
    c.frame_upload(0, win.images[0])
    trk = orc.Tracker(win.w, win.h, c.levels, win.K)
    dI_ref, _ = orc.make_images(win.images[0], c.levels)
    trk.set_ref(dI_ref, Ku, Kv, nid, hdi)
    for rep in range(3):
        c.trk_set_ref(0, Ku, Kv, nid, hdi)
        assert_ref_build_equal(c, trk, c.levels, "build %d" % rep)
    c.close()
