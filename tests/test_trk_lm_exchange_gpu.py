"""The exchange of block partials in trk_lm_kernel (kernels_trk_lm.hip) at the edges of its batched loads.

A reader lane of wave group g (8 groups per workgroup) sums the partials of the publishing workgroups g, g + 8, ... < nbl. It loads all of its words back to
back into a fixed array of 8 entries (16 on the 128-workgroup grid), entries past its last block re-reading a clamped index, and only then tests the tags
and adds the payloads, in the order it always did. The clouds here put nbl, the count of publishing workgroups of level 0, on the edges of that loop:

  level-0 points   workgroups   what it exercises
  512              1            no exchange (one workgroup)
  513              2            six wave groups sum nothing (all their entries are clamped re-reads)
  3 585            8            one block per group
  4 097            9            group 0 has two blocks, the others one
  6 249            13           the coarsest level of the headline cloud
  21 381           42           ragged: groups with 6 and with 5 blocks
(test_trk_large_gpu.py covers the 64- and 128-workgroup grids: B1, W2.)

Frames: 1224x368, the brightened noisy pair of test_trk_large_gpu.py (frames()). Clouds through trk_set_pc, seeded, raster order: level l holds
max(n0 / 4^l, min(n0, 384)) points, so that the coarse levels of the small clouds still constrain the pose (level 0 stays the largest: it sets the grid) and
the levels below 0 publish from fewer workgroups than the grid has (21 381: 42, 11, 3, 1 - the same launch runs four different nbl).

Per cloud:
  1  the checks of test_trk_large_gpu.py::compare against the fp32 and the all-fp64 oracle: ok and the evaluations per level equal, pose within 1e-5, affine
     pair within 1e-3, lastResiduals / flow indicators as close to fp64 as the fp32 oracle is (that test's bars, unchanged)
  2  bit for bit what the kernel computed BEFORE the loads were batched: T, aff, lastResiduals, the flow indicators, ok and the evaluations per level equal
     tests/golden/golden_trk_lm_exchange.npz (np.array_equal; equal_nan for the levels never run). The batched pass adds the same values in the same order,
     so nothing may move.
Reuse across grids: three rounds on one context alternating the 9- and the 42-workgroup cloud (stale tags of the other grid size in the partials buffer) -
identical outputs in every round, equal to the fixture.

The fixture: tests/golden/make_golden_trk_lm_exchange.py, run on an MI355X with the library built from the commit before this test was added (the kernel
with one load and one wait per block in the exchange loop); it runs track() below on every cloud and stores the outputs. It holds outputs of this project's
own kernel only. The bounded poll's timeout path cannot be provoked without holding the device; test_trk_large_gpu.py::test_host_driven_loop_at_128_workgroups
covers the host's fallback after an injected lost block."""
import functools
import os

import numpy as np
import pytest

import orc
from helpers import true_rel_pose
from nalo_slam_amd import binding
from test_trk_large_gpu import EXPOSURES, compare, frames

pytestmark = pytest.mark.gpu

W, H = 1224, 368
CLOUDS = {512: 1, 513: 2, 3585: 8, 4097: 9, 6249: 13, 21381: 42}              # level-0 points -> publishing workgroups of level 0 = the grid
LEVEL_FLOOR = 384
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_trk_lm_exchange.npz")
KEYS = ("ok", "T", "aff", "lr", "lf", "ev")
_OPEN = []


def level_sizes(n0, levels):
    return [max(n0 >> (2 * l), min(n0, LEVEL_FLOOR)) for l in range(levels)]


class Scene:
    """the frame pair on one context, the oracles' images and the start estimate (0.9 of the true motion)"""

    def __init__(self):
        self.win, self.new = frames(W, H)
        self.ctx = self.context()
        self.levels = self.ctx.levels
        self.dI_ref, _ = orc.make_images(self.win.images[0], self.levels)
        self.dI_new, _ = orc.make_images(self.new, self.levels)
        self.T0 = orc.se3_exp(orc.se3_log(true_rel_pose(self.win, 0, 1)) * 0.9)

    def context(self):
        c = binding.Context(self.win.w, self.win.h, self.win.K, n_slots=2)
        _OPEN.append(c)
        c.frame_upload(0, self.win.images[0]); c.frame_upload(1, self.new)
        return c

    @functools.lru_cache(maxsize=None)
    def clouds(self, n0):
        """(u, v, idepth, colour) per level: level_sizes(n0) pixels with a depth, drawn with seed n0, in raster order"""
        rng = np.random.RandomState(n0)
        L = orc.lib()
        out = []
        for l, n in enumerate(level_sizes(n0, self.levels)):
            wl, hl = W >> l, H >> l
            uu, vv = np.meshgrid(np.arange(2, wl - 3), np.arange(2, hl - 3))
            uu, vv = uu.ravel(), vv.ravel()
            d = self.win.depth[0][vv << l, uu << l]
            ok = np.isfinite(d) & (d > 0)
            uu, vv, d = uu[ok], vv[ok], d[ok]
            assert len(uu) >= n, (l, n, len(uu))
            k = np.sort(rng.choice(len(uu), n, replace=False))
            col = self.dI_ref[L.orc_pyr_offset(W, H, l) + vv[k] * wl + uu[k], 0]
            out.append(tuple(a.astype(np.float32) for a in (uu[k], vv[k], 1.0 / d[k], col)))
        return out

    def track(self, n0, c=None):
        """set the clouds of n0 on the context and track the new frame: the outputs, the cloud sizes and the launch configuration"""
        c = c or self.ctx
        for l, pc in enumerate(self.clouds(n0)):
            c.trk_set_pc(0, l, *pc)
        ok, T, aff, lr, lf, nev = c.trk_track(1, self.T0, (0, 0), (0, 0), EXPOSURES, self.levels - 1)
        ev, n = c.trk_last_evals()
        return dict(ok=ok, T=T, aff=aff, lr=lr, lf=lf, ev=ev, nev=nev, n=n, cfg=c.trk_launch_config())

    @functools.lru_cache(maxsize=None)
    def oracle(self, n0, kind):
        orc.lib("f32").orc_set_sum_mode(0)
        trk = orc.Tracker(W, H, self.levels, self.win.K, kind)
        for l, pc in enumerate(self.clouds(n0)):
            trk.set_pc(self.dI_ref, l, *pc)
        ok, T, aff, lr, lf = trk.track(self.dI_new, self.T0, (0, 0), (0, 0), EXPOSURES, self.levels - 1)
        ev, rep = trk.last_evals()
        return dict(ok=ok, T=T, aff=aff, lr=lr, lf=lf, ev=ev, nev=int(ev.sum()), rep=rep)


@functools.lru_cache(maxsize=None)
def scene():
    return Scene()


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _OPEN:
        c.close()
    _OPEN.clear()
    scene.cache_clear()


def check_grid(s, n0, g):
    """the launch is the variant the cloud is for: persistent kernel, 512 lanes, CLOUDS[n0] workgroups, one round per level"""
    cfg = g["cfg"]
    assert cfg["driver"] == 1 and cfg["lanes"] == 512 and cfg["nblocks"] == CLOUDS[n0] == -(-n0 // 512), (n0, cfg)
    assert list(g["n"][:s.levels]) == level_sizes(n0, s.levels) and cfg["rounds"][:s.levels] == [1] * s.levels, (n0, cfg, list(g["n"]))


def assert_equals_fixture(n0, g, tag):
    z = golden()
    for key in KEYS:
        want, got = z["%d_%s" % (n0, key)], np.asarray(g[key])
        assert want.dtype == got.dtype and np.array_equal(want, got, equal_nan=True), (tag, key, got, want)


@pytest.mark.parametrize("n0", list(CLOUDS))
def test_track_matches_oracles(n0):
    s = scene()
    g = s.track(n0)
    check_grid(s, n0, g)
    o32, o64 = s.oracle(n0, "f32"), s.oracle(n0, "f64")
    assert o32["ok"] == 1 and not o32["rep"] and g["cfg"]["have_repeated"] == 0
    compare(g, o32, o64, range(s.levels), "n0 = %d" % n0)


@pytest.mark.parametrize("n0", list(CLOUDS))
def test_track_bit_for_bit_as_before_the_batched_loads(n0):
    s = scene()
    g = s.track(n0)
    check_grid(s, n0, g)
    assert_equals_fixture(n0, g, "n0 = %d" % n0)


def test_alternating_grids_reuse_the_partials_buffer():
    """one context of its own, three rounds of the 9-workgroup and the 42-workgroup cloud: every launch finds the other grid's tags in the partials buffer"""
    s = scene()
    c = s.context()
    for rnd in range(3):
        for n0 in (4097, 21381):
            g = s.track(n0, c)
            check_grid(s, n0, g)
            assert_equals_fixture(n0, g, "round %d, n0 = %d" % (rnd, n0))
