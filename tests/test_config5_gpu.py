"""BASELINE.json configs[4] AT ITS OWN SIZE on one GPU: the synthetic 1 M active points / 12-keyframe window (bench.make_inputs("shard1m"):
1920x1072, R = 11 M residual slots). The large-window variants this window runs (sc_bpw 8 point blocks per SC workgroup, the radix select, the
device-built xAd) are compared with the oracle in tests/test_ba_large_gpu.py; the checks here are the size-independent properties of the path:
  determinism    the same pass twice (nalo_ba_snapshot / nalo_ba_restore) gives BIT-IDENTICAL stitched systems, energy, count and threshold: every sum of
                 the path has a fixed order (no float atomics), as the reference's per-thread replicas summed in order (AccumulatedTopHessian.h:144-149)
  linearity      two shards (nalo_shard_points through bench.shard: the partition the 8-GPU run uses) driven through the all-reduce hooks: residual counts
                 add up exactly, energy and the systems to fp32 summation noise, and both ranks install, bit for bit, the energy threshold of the whole
                 window (setNewFrameEnergyTH is an order statistic: both radix histograms are summed across ranks before their search)
  structure      H_A and H_A - H_sc are symmetric positive semi-definite (a Schur complement of a PSD system), b_A - b_sc is finite
  descent        optimize(6) lowers the photometric energy of the perturbed window and moves every frame towards the ground-truth pose"""
import threading

import numpy as np
import pytest
import torch

import bench
from helpers import pose_dist
from nalo_slam_amd import binding
from test_shard_gpu import _Ptr, make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def window():
    win, st6, _ = bench.make_inputs("shard1m")
    assert win.W == 12 and len(win.host) == 1000000 and (win.w, win.h) == (1920, 1072)
    return win, st6


def one_pass(c, W):
    e = c.ba_linearize()
    th = c.ba_get_frames()[0][W - 1].frameEnergyTH
    HA, bA = c.ba_accumulate(0)
    Hs, bs = c.ba_accumulate_sc(True)
    return dict(e=e, th=th, HA=HA, bA=bA, Hs=Hs, bs=bs, n=c.ba_counts()[0])


def test_config5_determinism_structure_descent(window):
    win, st6 = window
    W = win.W
    c = make_ctx(win, st6)
    c.ba_snapshot()
    a = one_pass(c, W)
    c.ba_restore()
    b = one_pass(c, W)
    for k in ("e", "th", "n"):
        assert a[k] == b[k], k
    for k in ("HA", "bA", "Hs", "bs"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n"] > 0.4 * int((win.exists > 0).sum())                      # 0.8 m forward per keyframe over 12 frames: more than half of the 11 M slots project outside
    # structure
    HA, Hs = a["HA"], a["Hs"]
    sc = np.abs(HA).max()
    assert np.abs(HA - HA.T).max() <= 1e-12 * sc and np.abs(Hs - Hs.T).max() <= 1e-6 * np.abs(Hs).max()
    assert np.isfinite(a["bA"]).all() and np.isfinite(a["bs"]).all()
    d = 1.0 / np.sqrt(np.maximum(np.diag(HA), 1e-300))                       # Jacobi scaling (as solveSystemF does) before looking at the spectrum
    for M in (HA, HA - 0.5 * (Hs + Hs.T)):
        ev = np.linalg.eigvalsh(d[:, None] * M * d[None, :])
        print("  Jacobi-scaled spectrum: min %.3e max %.3e" % (ev.min(), ev.max()))
        # the 7 gauge directions are exact null directions of H_A - H_sc; the difference cancels ~100x on fp32 products, so "zero" is 1e-5 of the scale
        assert ev.min() > -2e-5 * ev.max(), (ev.min(), ev.max())
    # descent: FullSystem::optimize on the perturbed window
    c.ba_restore()
    w2c0 = c.ba_get_frames()[1].copy()
    c.ba_optimize(6, never_break=True)
    w2c1 = c.ba_get_frames()[1].copy()
    e1 = c.ba_linearize()
    assert e1 < 0.8 * a["e"], (e1, a["e"])
    # gauge: poses relative to frame 0 (its pose prior holds it), translations up to the monocular scale
    def rel(ws):
        return [bench.synth.se3_mul(ws[i], bench.synth.se3_inv(ws[0])) for i in range(1, W)]
    truth = rel(win.world_to_cam[:W])
    def err(ws):
        r = rel(ws)
        ta, tb = np.array([x[:, 3] for x in truth]), np.array([x[:, 3] for x in r])
        s = (ta * tb).sum() / (tb * tb).sum()
        return max(pose_dist(t, np.c_[x[:, :3], s * x[:, 3]]) for t, x in zip(truth, r))
    assert err(w2c1) < 0.2 * err(w2c0), (err(w2c0), err(w2c1))
    c.close()
    test_config5_determinism_structure_descent.full = a                        # the two-shard test compares against this pass


def test_config5_two_shards_add_up(window):
    win, st6 = window
    W = win.W
    full = getattr(test_config5_determinism_structure_descent, "full", None)
    if full is None:
        c = make_ctx(win, st6); full = one_pass(c, W); c.close()
    world = 2
    bar = threading.Barrier(world)
    bufs, out, err = [None] * world, [None] * world, []

    def rank_job(r):
        try:
            part = bench.shard(win, r, world)
            c = make_ctx(part, st6)
            local = one_pass(c, W)                                   # no hook yet: this rank's own sums
            c.close()
            c = make_ctx(part, st6)

            def hook(ptr, n):                                        # blocking contract: the library drained the producing stream before the call
                t = torch.as_tensor(_Ptr(ptr, n), device="cuda")
                bufs[r] = t.cpu()
                bar.wait()
                tot = bufs[0] + bufs[1]
                bar.wait()
                t.copy_(tot)
                torch.cuda.synchronize()
            c.ba_set_allreduce(hook)
            red = one_pass(c, W)
            c.ba_set_allreduce(None)
            c.close()
            out[r] = dict(local=local, red=red, n_pts=len(part.host))
        except Exception as ex:                                      # never leave the other rank waiting in the barrier
            err.append(ex)
            bar.abort()

    ts = [threading.Thread(target=rank_job, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(900) for t in ts]
    assert not err, err
    a, b = out
    assert a["n_pts"] + b["n_pts"] == len(win.host) and abs(a["n_pts"] - b["n_pts"]) <= W
    # rank-local passes (no exchange): counts add up exactly, energies and systems up to the order of fp32 / fp64 partial sums
    assert a["local"]["n"] + b["local"]["n"] == full["n"]
    assert abs(a["local"]["e"] + b["local"]["e"] - full["e"]) < 1e-6 * full["e"]
    for k in ("HA", "bA", "Hs", "bs"):
        s = a["local"][k] + b["local"][k]
        assert np.abs(s - full[k]).max() < 2e-5 * np.abs(full[k]).max(), k
    # through the hooks both ranks hold the window's sums and, bit for bit, its energy threshold
    assert a["red"]["th"] == b["red"]["th"] == full["th"]
    assert a["red"]["n"] == b["red"]["n"] == full["n"] and a["red"]["e"] == b["red"]["e"]
    assert abs(a["red"]["e"] - full["e"]) < 1e-6 * full["e"]
    for k in ("HA", "bA", "Hs", "bs"):
        assert np.array_equal(a["red"][k], b["red"][k]), k
        assert np.abs(a["red"][k] - full[k]).max() < 2e-5 * np.abs(full[k]).max(), k
    # a rank alone would NOT find that threshold: the cross-rank histogram sum is what makes it the window's
    assert a["local"]["th"] != full["th"] or b["local"]["th"] != full["th"]
