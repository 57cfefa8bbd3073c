"""The window replacement on the device (nalo_tsdf_replace_depth_n, nalo_tsdf_replace_last_n, nalo_tsdf_replace_frames; include/nalo_gpu.h, "The window
replacement"). The yardstick throughout is a twin context that loops the EXISTING nalo_tsdf_replace_depth / nalo_tsdf_replace_frame: equality bit for bit (a NaN
as a NaN) in tsdf, weight and colour, per-pair counts equal to the twin's nalo_tsdf_replace_last after its call k, written_total equal to the voxels whose flags
tests/tsdf_replace_window_model.py sets. Scenes and helpers are tests/test_tsdf_replace_gpu.py's."""
import math
import time

import numpy as np
import pytest
import torch

import tsdf_color_model as cm
import tsdf_mesh_model as mm
import tsdf_replace_model as rm
import tsdf_replace_window_model as wm
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth
from test_tsdf_gpu import FRAME_GRID, GRIDS, H0, K0, POSES, W0, bits_eq, ctx, frame_scene, make, planted
from test_tsdf_replace_gpu import ERR_ARG, ERR_STATE, H1, K1, KN, W1, assert_volume, cmake, dev, moved_pose, rand_bgr, sides, six_planes

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ("removed", "reset", "added", "written")


def arrays(c, colour):
    t, w = c.tsdf_get()
    return [t, w] + ([c.tsdf_color_get()] if colour else [])


def same_volume(a, b, colour):
    """two contexts' volumes bit for bit, a NaN as a NaN"""
    return all(mm.same_floats(x, y) for x, y in zip(arrays(a, colour), arrays(b, colour)))


def dev_pairs(pairs):
    return [dict(remove=None if p.get("remove") is None else p["remove"][0], add=None if p.get("add") is None else p["add"][0], box=p.get("box")) for p in pairs]


def model_pairs(pairs):
    return [dict(remove=None if p.get("remove") is None else p["remove"][1], add=None if p.get("add") is None else p["add"][1], box=p.get("box")) for p in pairs]


def chain_against_twin(c, twin, vol, pairs, colour, tag=""):
    """ONE nalo_tsdf_replace_depth_n on c against the twin's loop of nalo_tsdf_replace_depth, and against the model when vol is given. pairs: dict(remove=, add=,
    box=) of sides() pairs. Returns (total, rows, model result or None)"""
    c.tsdf_replace_depth_n(dev_pairs(pairs))
    total, rows = c.tsdf_replace_last_n()
    last = c.tsdf_last()
    print("replace_n", tag, len(pairs), {k: total[k] for k in ("visited",) + KEYS}, rows)
    assert len(rows) == len(pairs)
    for k, p in enumerate(dev_pairs(pairs)):
        twin.tsdf_replace_depth(p["remove"], p["add"], p["box"])
        st = twin.tsdf_replace_last()
        assert rows[k] == {q: st[q] for q in KEYS}, (tag, k, rows[k], st)
    assert same_volume(c, twin, colour), tag
    assert all(total[q] == sum(r[q] for r in rows) for q in ("removed", "reset", "added")) and total == c.tsdf_replace_last()
    assert (last["lo"], last["hi"], last["visited"], last["updated"]) == (total["lo"], total["hi"], total["visited"], total["written"])
    assert max(r["written"] for r in rows) <= total["written"] <= sum(r["written"] for r in rows)
    r = None
    if vol is not None:
        lo, hi, visited = wm.hull_n(vol, model_pairs(pairs))
        r = wm.replace_n(vol, model_pairs(pairs))
        assert (total["lo"], total["hi"], total["visited"]) == (lo, hi, visited), (tag, total, lo, hi)
        assert rows == r["pairs"] and total["written"] == r["written_total"], (tag, rows, r["pairs"], r["written_total"])
        assert_volume(c, vol, tag)
    return total, rows, r


def fused_pair(g, colour):
    """c, twin and the model with tests/test_tsdf_gpu.py's six planes fused"""
    c, twin = ctx(), ctx()
    vol = (cmake if colour else make)(c, g)
    (cmake if colour else make)(twin, g)
    planes = [sides(d, K0, c2w, 1.0, 0.5, 3.5, b if colour else None) for d, c2w, b in six_planes(GRIDS.index(g))]
    for sd in planes:
        for x in (c, twin):
            x.tsdf_replace_depth(add=sd[0])
        rm.replace(vol, add=sd[1])
    return c, twin, vol, planes


# ------------------------------------------------------------------------------------------------ 1. n = 1 is nalo_tsdf_replace_depth
@pytest.mark.parametrize("gi", [0, 1])
def test_one_pair_is_the_single_replacement(gi):
    g = GRIDS[gi]
    c, twin = ctx(), ctx()
    cmake(c, g)
    cmake(twin, g)
    a, b = (binding.tsdf_side(dev(wavy_depth(W0, H0, 3 + q)), K0, POSES[q], 1.0 + 0.02 * q, 0.5, 3.5, colour=dev(rand_bgr(W0, H0, q))) for q in range(2))
    box = ((3, 2, 1), (21, 11, 3))
    for q, kw in enumerate((dict(add=a), dict(remove=a, add=b), dict(remove=b, box=box), dict(remove=a, add=a), dict(remove=a))):
        c.tsdf_replace_depth_n([kw])
        twin.tsdf_replace_depth(**kw)
        total, rows = c.tsdf_replace_last_n()
        st = twin.tsdf_replace_last()
        assert c.tsdf_last() == twin.tsdf_last() and c.tsdf_replace_last() == st == total and rows == [{k: st[k] for k in KEYS}], (q, total, st)
        assert same_volume(c, twin, True), q
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
            twin.tsdf_replace_last_n()                                          # the twin's last operation was no window replacement
    assert total["removed"] > 300
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 2. chains on the six-times-fused volumes
@pytest.mark.parametrize("n,colour", [(2, True), (3, False), (7, True), (16, True)])
def test_chains_on_the_fused_volumes(n, colour):
    """removals and adds at s = 0.5, 1, 1.25 and 2; pairs with only a remove side, with only an add side, with both; a plane that one pair adds is what a later
    pair removes (one plane serving several pairs), and the six fused planes go out along the way"""
    g = GRIDS[n % 2]
    c, twin, vol, planes = fused_pair(g, colour)
    scales = (0.5, 1.0, 1.25, 2.0)
    new = []
    for q in range(n):
        s = scales[q % 4]
        w, h, K = ((W0, H0, K0), (W1, H1, K1))[q % 2]
        new.append(sides(wavy_depth(w, h, 100 + q) / F(s), K, POSES[q % 3], s, 0.5 / s, 3.5 / s, rand_bgr(w, h, 100 + q) if colour else None))
    pairs = []
    for k in range(n):
        kind = k % 4
        if kind == 0:
            pairs.append(dict(add=new[k]))
        elif kind == 1:
            pairs.append(dict(remove=planes[k % 6], add=new[k]))
        elif kind == 2:
            pairs.append(dict(remove=new[k - 2]))                               # what pair k - 2 added
        else:
            pairs.append(dict(remove=new[k - 2], add=new[k - 2]))               # one plane on both sides: out and in again
    total, rows, r = chain_against_twin(c, twin, vol, pairs, colour, tag=("chain", n, colour))
    assert total["removed"] > 300 and total["added"] > 300 and total["written"] < sum(x["written"] for x in rows)      # overlapping frusta: strict
    assert all(x["written"] > 0 for x in rows)
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 3. the order is part of the definition
def test_the_planted_order_case_in_both_orders():
    g, fused, spec = wm.order_case()
    out = []
    for order in (spec, spec[::-1]):
        c, twin = ctx(), ctx()
        vol = cmake(c, g)
        cmake(twin, g)
        for sd in fused:
            both = sides(*sd)
            for x in (c, twin):
                x.tsdf_replace_depth(add=both[0])
            rm.replace(vol, add=both[1])
        pairs = [dict(remove=None if p["remove"] is None else sides(*p["remove"]), add=None if p["add"] is None else sides(*p["add"])) for p in order]
        chain_against_twin(c, twin, vol, pairs, True, tag="order")
        out.append(arrays(c, True))
        c.close()
        twin.close()
    assert all(not mm.same_floats(x, y) for x, y in zip(out[0], out[1]))          # tsdf, weight and colour all differ between the two orders


# ------------------------------------------------------------------------------------------------ 4. boxes
def test_per_pair_boxes_at_every_phase_and_the_voxels_beyond_their_faces():
    g = dict(origin=(-1.5, -1.5, 0.0), vs=0.1, dims=(30, 30, 36), trunc=0.2, mw=8.0)      # tests/test_tsdf_gpu.py's interior-box grid
    c, twin = ctx(), ctx()
    vol = cmake(c, g)
    cmake(twin, g)
    rng = np.random.RandomState(5)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["weight"][:] = rng.randint(2, 6, vol["weight"].shape)
    vol["colour"][:] = rng.uniform(0, 255, vol["colour"].shape)
    for x in (c, twin):
        x.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
        x.tsdf_color_set((0, 0, 0), vol["colour"])
    wide = sides(np.full((H0, W0), 1.9, F), K0, pose(0.05, -0.04, 0.3, (0.1, -0.05, 0.55)), 1.0, 0.5, 2.0, rand_bgr(W0, H0, 3))
    takes = rm.sample(vol, wide[1])[0]
    before = {k: vol[k].copy() for k in ("tsdf", "weight", "colour")}
    # four removals of the same plane, each inside its own box: x ranges that start at every phase of a group of four, different per pair, in slabs of z
    # that do not meet
    boxes = [((12, 9, 14), (8, 8, 3)), ((13, 10, 17), (8, 6, 3)), ((14, 9, 20), (5, 8, 2)), ((15, 11, 22), (2, 5, 2))]
    assert sorted(b[0][0] % 4 for b in boxes) == [0, 1, 2, 3]
    total, rows, r = chain_against_twin(c, twin, vol, [dict(remove=wide, box=b) for b in boxes], True, tag="boxes")
    union = np.zeros(takes.shape, bool)
    for k, (lo, sz) in enumerate(boxes):
        inb = np.zeros(takes.shape, bool)
        inb[lo[2]:lo[2] + sz[2], lo[1]:lo[1] + sz[1], lo[0]:lo[0] + sz[0]] = True
        assert rows[k]["removed"] == rows[k]["written"] == int((takes & inb).sum()) > 0
        union |= inb
        # the side takes voxels beyond each of the box's six faces
        for a in range(3):
            for far in (False, True):
                face = np.zeros(takes.shape, bool)
                sl = [slice(None)] * 3
                sl[2 - a] = slice(lo[a] + sz[a], None) if far else slice(0, lo[a])
                face[tuple(sl)] = True
                assert (takes & face).any(), (k, a, far)
    beyond = takes & ~union
    t, w = c.tsdf_get()
    col = c.tsdf_color_get()
    assert beyond.sum() > 300 and bits_eq(t[beyond], before["tsdf"][beyond]) and bits_eq(w[beyond], before["weight"][beyond]) and bits_eq(col[:, beyond], before["colour"][:, beyond])
    assert total["written"] == sum(x["written"] for x in rows) == int((takes & union).sum())      # the boxes do not meet: every voxel fired once
    c.close()
    twin.close()


def test_frusta_that_do_not_meet_and_narrow_hulls():
    g = GRIDS[1]                                                                # 33 voxels a row: rows begin at every phase of a group of four
    c, twin, vol, planes = fused_pair(g, True)
    side_at = lambda tx, seed: sides(wavy_depth(W0, H0, seed), KN, pose(0, 0, 0, (tx, 0.0, 0.0)), 1.0, 0.5, 3.5, rand_bgr(W0, H0, seed))
    left, right = side_at(-0.6, 40), side_at(0.99, 41)
    bl, br = (rm.frustum_box_est(vol, W0, H0, KN, sd[1]["c2w"], 1.0, 3.5) for sd in (left, right))
    assert bl[1][0] < br[0][0]                                                  # columns of the hull in neither box
    total, rows, r = chain_against_twin(c, twin, vol, [dict(add=left), dict(add=right)], True, tag="frusta that do not meet")
    assert rows[0]["added"] > 0 and rows[1]["added"] > 0 and total["written"] == rows[0]["written"] + rows[1]["written"]
    assert (total["lo"][0], total["hi"][0]) == (bl[0][0], br[1][0]) and total["visited"] > sum(rm.hull(vol, add=sd[1])[2] for sd in (left, right))
    total, rows, r = chain_against_twin(c, twin, vol, [dict(remove=left, add=right), dict(remove=right, add=left)], True, tag="swapped")
    assert rows[0]["removed"] > 0 and rows[1]["removed"] > 0
    # hull x ranges of 1, 3, 4, 5 and 33 voxels, at starts of every phase: the scalar ends, a single partial group, and whole rows
    for x0, sx in ((14, 1), (13, 3), (12, 4), (15, 5), (17, 4), (18, 3), (0, 33)):
        box = ((x0, 0, 0), (sx, 17, 5))
        total, rows, r = chain_against_twin(c, twin, vol, [dict(remove=planes[q], box=box) for q in (0, 3, 1)], True, tag=("narrow", x0, sx))
        assert total["hi"][0] - total["lo"][0] == sx and total["lo"][0] == x0 and total["removed"] > 0
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 5. weights and colour
def test_max_weight_reached_in_the_middle_of_the_chain():
    g = GRIDS[0]
    c, twin = ctx(), ctx()
    vol = cmake(c, g)                                                           # max_weight = 4
    cmake(twin, g)
    p = [sides(wavy_depth(W0, H0, 200 + q, base=2.0 + 0.01 * q), K0, POSES[0], 1.0, 0.5, 3.5, rand_bgr(W0, H0, 200 + q)) for q in range(6)]
    pairs = [dict(add=p[q]) for q in range(6)] + [dict(remove=p[q]) for q in (0, 1, 2)]
    total, rows, r = chain_against_twin(c, twin, vol, pairs, True, tag="saturating")
    # six adds of nearly the same voxels saturate at 4 behind the fourth; three removals take the weight to 1, which a faithful count would leave at 3
    mid = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    wm.replace_n(mid, model_pairs(pairs[:6]))
    assert mid["weight"].max() == 4.0 and (mid["weight"] == 4.0).sum() > 300
    assert (vol["weight"] == 1.0).sum() > 300 and rows[5]["added"] > 300 and rows[8]["removed"] > 300
    c.close()
    twin.close()


def test_planted_weights_and_a_nan_tsdf_through_a_chain():
    g, K, depth = planted(EYE)
    c, twin = ctx(32, 16, K), ctx(32, 16, K)
    vol = cmake(c, g)
    cmake(twin, g)
    rng = np.random.RandomState(9)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["weight"][:] = rng.randint(2, 4, vol["weight"].shape)
    vol["colour"][:] = rng.uniform(0, 255, vol["colour"].shape)
    up = np.nextafter(F(1.0), F(2.0))
    for i, w0 in zip(range(12, 19), (0.0, 1.0, up, 0.5, np.nan, np.inf, 3.0)):   # the row (j = 4, k = 6) reads the constant 1.5 left of i = 20: d = 1
        vol["weight"][6, 4, i] = w0
    vol["tsdf"][6, 4, 18] = np.nan
    for x in (c, twin):
        x.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
        x.tsdf_color_set((0, 0, 0), vol["colour"])
    sd = sides(depth, K, EYE, 1.0, 0.5, 2.0, rand_bgr(32, 16, 1))
    plain = sides(depth, K, EYE, 1.0, 0.5, 2.0)
    total, rows, r = chain_against_twin(c, twin, vol, [dict(remove=sd), dict(add=sd), dict(remove=plain, add=sd), dict(remove=sd)], True, tag="planted")
    T, Wt = vol["tsdf"], vol["weight"]
    # w0 = 0, 1, 0.5, NaN: reset by pair 0, 1 behind pair 1, reset and added by pair 2, reset by pair 3. +inf and the NaN tsdf stay NaN in tsdf
    for i in (12, 13, 15, 16):
        assert (T[6, 4, i], Wt[6, 4, i]) == (1.0, 0.0), i
    assert np.isnan(T[6, 4, 17]) and np.isnan(T[6, 4, 18]) and rows[0]["reset"] >= 4
    c.close()
    twin.close()


def test_views_channel_orders_and_uncoloured_sides_on_different_pairs():
    """tests/test_tsdf_replace_gpu.py's views, one per pair: a pitched RGB view on pair 0's remove side with an uncoloured add, a planar x-strided view on pair
    1's add side, an uncoloured removal as pair 2. Elements outside the views (depth 1.3, colour 77) would change a result"""
    g = GRIDS[0]
    c, twin = ctx(), ctx()
    vol = cmake(c, g)
    cmake(twin, g)
    da, db, ba, bb = wavy_depth(W0, H0, 7), wavy_depth(W1, H1, 8), rand_bgr(W0, H0, 70), rand_bgr(W1, H1, 71)
    first = sides(da, K0, POSES[0], 1.0, 0.5, 3.5, ba)
    for x in (c, twin):
        x.tsdf_replace_depth(add=first[0])
    rm.replace(vol, add=first[1])
    bigd = torch.full((H0 + 6, W0 + 10), 1.3, device="cuda")
    bigd[3:3 + H0, 5:5 + W0] = dev(da)
    bigc = torch.full((H0 + 6, W0 + 10, 3), 77, dtype=torch.uint8, device="cuda")
    bigc[3:3 + H0, 5:5 + W0] = dev(ba[:, :, ::-1])                               # the tensor holds R, G, B
    rem = binding.tsdf_side(bigd[3:3 + H0, 5:5 + W0], K0, POSES[0], 1.0, 0.5, 3.5, colour=binding.dev_plane(bigc[3:3 + H0, 5:5 + W0], "hwc"), colour_is_rgb=True)
    wided = torch.full((H1, 3 * W1), 1.3, device="cuda")
    wided[:, 1::3] = dev(db)
    planar = torch.full((3, H1 + 4, W1 + 6), 77, dtype=torch.uint8, device="cuda")
    planar[:, 2:2 + H1, 3:3 + W1] = dev(bb.transpose(2, 0, 1))
    add = binding.tsdf_side(wided[:, 1::3], K1, POSES[2], 1.1, 0.5, 3.5, colour=binding.dev_plane(planar[:, 2:2 + H1, 3:3 + W1], "chw"))
    unc = sides(wavy_depth(W0, H0, 9), K0, POSES[1], 1.0, 0.5, 3.5)
    pairs = [dict(remove=(rem, rm.side(da, K0, POSES[0], 1.0, 0.5, 3.5, ba)), add=unc), dict(add=(add, rm.side(db, K1, POSES[2], 1.1, 0.5, 3.5, bb))), dict(remove=unc)]
    col = vol["colour"].copy()
    total, rows, r = chain_against_twin(c, twin, vol, pairs, True, tag="views")
    assert all(x["written"] > 300 for x in rows)
    # a voxel only the uncoloured sides touched keeps its colour words
    only_unc = rm.sample(vol, unc[1])[0] & ~rm.sample(vol, pairs[0]["remove"][1])[0] & ~rm.sample(vol, pairs[1]["add"][1])[0]
    assert only_unc.sum() > 20 and bits_eq(vol["colour"][:, only_unc], col[:, only_unc])
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 6. streams
def test_two_producer_streams_in_one_list_without_a_host_wait():
    """pair 0's planes are written on one producer stream and pair 1's on another, each behind queued matmuls (0.2 s in all); the call returns while they are
    still queued, the kernel reads the planes only behind both, and nalo_tsdf_release makes each producer's next write wait for the kernel"""
    g = GRIDS[0]
    c = ctx()
    vol = make(c, g)
    d0, d1, d2 = wavy_depth(W0, H0, 50), wavy_depth(W0, H0, 51, base=2.1), wavy_depth(W0, H0, 52, base=1.9)
    c.tsdf_replace_depth_n([dict(add=binding.tsdf_side(dev(d0), K0, POSES[0], 1.0, 0.5, 3.5))])      # warm-up: the table, the events
    rm.replace(vol, add=rm.side(d0, K0, POSES[0], 1.0, 0.5, 3.5))
    assert_volume(c, vol, "warm-up")
    ta, tb, tc = (torch.full((H0, W0), 1.3, device="cuda") for _ in range(3))
    s0, s1, s2 = dev(d0), dev(d1), dev(d2)
    a = torch.randn(4096, 4096, device="cuda")
    outs = [torch.empty_like(a), torch.empty_like(a)]
    S = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(S[0]):
            torch.mm(a, a, out=outs[0])
            S[0].synchronize()
            t0 = time.perf_counter()
            torch.mm(a, a, out=outs[0])
            S[0].synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
        reps = min(int(math.ceil(0.2 / one)) + 1, 20000)
        behind = []
        for q, job in enumerate((((ta, s0), (tb, s1)), ((tc, s2),))):
            with torch.cuda.stream(S[q]):
                for _ in range(reps):
                    torch.mm(a, a, out=outs[q])
                for t, s in job:
                    t.copy_(s)
                ev = torch.cuda.Event()
                ev.record(S[q])
                behind.append(ev)
        pairs = [dict(remove=binding.tsdf_side(ta, K0, POSES[0], 1.0, 0.5, 3.5), add=binding.tsdf_side(tb, K0, POSES[1], 1.0, 0.5, 3.5), stream=S[0].cuda_stream),
                 dict(add=binding.tsdf_side(tc, K0, POSES[2], 1.0, 0.5, 3.5), stream=S[1].cuda_stream)]
        c.tsdf_replace_depth_n(pairs, release=True)
        assert not behind[0].query() and not behind[1].query(), "the call waited for a producer stream"
        for q, ts in enumerate(((ta, tb), (tc,))):
            with torch.cuda.stream(S[q]):
                for t in ts:
                    t.fill_(1.3)                                                # behind nalo_tsdf_release: must not reach the kernel
        wm.replace_n(vol, [dict(remove=rm.side(d0, K0, POSES[0], 1.0, 0.5, 3.5), add=rm.side(d1, K0, POSES[1], 1.0, 0.5, 3.5)), dict(add=rm.side(d2, K0, POSES[2], 1.0, 0.5, 3.5))])
        total, rows = c.tsdf_replace_last_n()
        assert rows[0]["removed"] > 300 and rows[1]["added"] > 300
        assert_volume(c, vol, "behind both producers")
    finally:
        for s in S:
            s.synchronize()
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. two runs; queued calls; an untouched twin
def run_once():
    g = GRIDS[1]
    c, idle = ctx(), ctx()
    cmake(c, g)
    cmake(idle, g)
    initial = [x.copy() for x in arrays(idle, True)]
    p = [binding.tsdf_side(dev(wavy_depth(W0, H0, 300 + q)), K0, POSES[q % 3], 1.0 + 0.01 * q, 0.5, 3.5, colour=dev(rand_bgr(W0, H0, 300 + q))) for q in range(8)]
    out = []
    # six calls back to back with no wait between them: more than the staging slots, so a slot comes round while its first table may still be queued
    for r in range(6):
        c.tsdf_replace_depth_n([dict(add=p[(r + q) % 8]) if r < 2 else dict(remove=p[(r + q) % 8], add=p[(r + q + 3) % 8]) for q in range(5)], release=False)
    out.append([x.tobytes() for x in arrays(c, True)] + [repr(c.tsdf_replace_last_n()), repr(c.tsdf_last())])
    assert all(bits_eq(x, y) for x, y in zip(arrays(idle, True), initial))        # a context that is never touched stays untouched
    c.close()
    idle.close()
    return out


def test_two_runs_give_the_same_bytes_and_queued_calls_keep_their_tables():
    a, b = run_once(), run_once()
    assert a == b
    # the same six calls with a wait behind each: what the queued ones must have computed
    g = GRIDS[1]
    c = ctx()
    cmake(c, g)
    p = [binding.tsdf_side(dev(wavy_depth(W0, H0, 300 + q)), K0, POSES[q % 3], 1.0 + 0.01 * q, 0.5, 3.5, colour=dev(rand_bgr(W0, H0, 300 + q))) for q in range(8)]
    for r in range(6):
        c.tsdf_replace_depth_n([dict(add=p[(r + q) % 8]) if r < 2 else dict(remove=p[(r + q) % 8], add=p[(r + q + 3) % 8]) for q in range(5)])
        c.tsdf_replace_last_n()
    assert [x.tobytes() for x in arrays(c, True)] == a[0][:3]
    c.close()


# ------------------------------------------------------------------------------------------------ 8. frames and the log
def frames_context(w, h):
    """tests/test_tsdf_replace_gpu.py's two frames A and B with a dense list each"""
    import test_dense_map_gpu as tdm
    sa, sb = frame_scene(w, h), frame_scene(w, h, shift=0.4)
    c = tdm.context(sa)
    assert min(fill_frames(c, sa, sb, w)) > 1000
    return c, sa, sb, tdm


def fill_frames(c, sa, sb, w, short_b=False):
    """the two dense lists (short_b: B's from the points of one wall only); the points each call appended"""
    import plane_model as pm
    import test_dense_map_gpu as tdm
    keep = np.ones(len(sb["u"]), bool)
    if short_b:
        keep = sb["mask"][sb["v"].astype(np.int32), sb["u"].astype(np.int32)] == 3.0
        assert 10 < keep.sum() < len(keep)
    na, nb = len(sa["u"]), int(keep.sum())
    cat = lambda k: np.concatenate([sa[k], sb[k][keep]])
    c.ba_set_points(np.concatenate([np.zeros(na, np.int32), np.ones(nb, np.int32)]), cat("u"), cat("v"), cat("idp"), np.full((na + nb, 8), 100, F), np.ones((na + nb, 8), F))
    return [c.dense_update_map(hf, pm.make_draws(w + hf), tdm.C2W)[2] for hf in (0, 1)]


def frames_both(c, twin, ids, poses, K, mn, mx, s=1.0, skip=False, colour=True, tag=""):
    """ONE nalo_tsdf_replace_frames on c against the twin's loop of nalo_tsdf_replace_frame: volume, colour and log"""
    ss = list(s) if np.ndim(s) else [s] * len(ids)
    n_skipped = c.tsdf_replace_frames(ids, poses, K, mn, mx, s=s, skip_unchanged=skip)
    for k, fid in enumerate(ids):
        twin.tsdf_replace_frame(fid, None if poses is None else poses[k], K, mn, mx, s=ss[k])
    assert rm.log_equal(c.tsdf_log_get(), twin.tsdf_log_get()), (tag, c.tsdf_log_get(), twin.tsdf_log_get())
    assert same_volume(c, twin, colour), tag
    return n_skipped


@pytest.mark.parametrize("w,h", [(80, 48), (320, 240)])
def test_replace_frames_against_the_loop_of_replace_frame(w, h):
    import plane_model as pm
    c, sa, sb, tdm = frames_context(w, h)
    twin = frames_context(w, h)[0]
    K, A, B = sa["K"], tdm.FID, tdm.FID + 1
    for x in (c, twin):
        cmake(x, FRAME_GRID)
        x.tsdf_log_enable()
        x.tsdf_integrate_frame(A, tdm.C2W, K, 0.5, 8.0)
    pa, pb, pc = tdm.C2W, moved_pose(tdm.C2W, (0.05, -0.03, 0.04)), moved_pose(tdm.C2W, (-0.04, 0.02, 0.06))
    # ---- a frame with an entry and a frame without one
    assert frames_both(c, twin, [A, B], [pb, pa], K, 0.6, 7.5, s=[1.02, 1.0], tag="entry and none") == 0
    total, rows = c.tsdf_replace_last_n()
    assert len(rows) == 2 and rows[0]["removed"] > 300 and rows[0]["added"] > 300 and rows[1]["removed"] == 0 < rows[1]["added"]
    assert [e["frame_id"] for e in c.tsdf_log_get()] == [A, B]
    # ---- A's list grows: the first n_records records on its remove side, the whole list on its add side; B's plane serves both its sides
    sc2 = frame_scene(w, h, shift=0.2)
    P = len(sc2["u"])
    for x in (c, twin):
        x.ba_set_points(np.zeros(P, np.int32), sc2["u"], sc2["v"], sc2["idp"], np.full((P, 8), 100, F), np.ones((P, 8), F))
        assert x.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] > 1000
    n_before = c.tsdf_log_get()[0]["n_records"]
    assert len(c.map_dense_get(A)) > n_before
    assert frames_both(c, twin, [B, A], [pc, pc], K, 0.5, 8.0, tag="a list that has grown") == 0
    assert c.tsdf_log_get()[0]["n_records"] == len(c.map_dense_get(A)) and [e["frame_id"] for e in c.tsdf_log_get()] == [A, B]
    # ---- resident boxes behind a shift: each entry's box cuts its own pair's removal
    for x in (c, twin):
        x.tsdf_shift((6, 0, -4))
    dims = FRAME_GRID["dims"]
    assert all(e["size"] == (dims[0] - 6, dims[1], dims[2] - 4) for e in c.tsdf_log_get())
    d, b = wavy_depth(w, h, 3, base=2.4), rand_bgr(w, h, 3)
    for x in (c, twin):                                                         # something in the fresh voxels that a removal without the box would disturb
        x.tsdf_integrate_depth(dev(d), K, tdm.C2W, 0.5, 8.0, colour=dev(b))
    assert frames_both(c, twin, [A, B], [pa, pb], K, 0.5, 8.0, s=[1.0, 1.03], tag="resident boxes") == 0
    assert all(e["size"] == tuple(dims) for e in c.tsdf_log_get())
    # ---- skip_unchanged: none, some, all
    last, log = repr(c.tsdf_last()), c.tsdf_log_get()
    assert frames_both(c, twin, [A, B], [pb, pa], K, 0.5, 8.0, skip=True, tag="none unchanged") == 0
    assert c.tsdf_replace_frames([A, B], [pb, pc], K, 0.5, 8.0, skip_unchanged=True) == 1        # A is where the call before put it
    twin.tsdf_replace_frame(B, pc, K, 0.5, 8.0)
    assert rm.log_equal(c.tsdf_log_get(), twin.tsdf_log_get()) and same_volume(c, twin, True) and len(c.tsdf_replace_last_n()[1]) == 1
    last, vb = repr(c.tsdf_last()), [x.copy() for x in arrays(c, True)]
    c.profile_enable(True)
    c.profile_reset()
    assert c.tsdf_replace_frames([B, A], [pc, pb], K, 0.5, 8.0, skip_unchanged=True) == 2        # all unchanged: nothing is launched
    assert c.profile_get("tsdf_replace_n")[1] == 0 and c.profile_get("tsdf_replace")[1] == 0
    c.profile_enable(False)
    assert repr(c.tsdf_last()) == last and rm.log_equal(c.tsdf_log_get(), twin.tsdf_log_get()) and all(bits_eq(x, y) for x, y in zip(arrays(c, True), vb))
    assert c.tsdf_replace_frames([B, A], [pc, pb], K, 0.5, 8.0, s=[1.0, 1.0 + 2.0 ** -52], skip_unchanged=True) == 1      # one ulp in s is a change
    twin.tsdf_replace_frame(A, pb, K, 0.5, 8.0, s=1.0 + 2.0 ** -52)
    assert rm.log_equal(c.tsdf_log_get(), twin.tsdf_log_get()) and same_volume(c, twin, True)
    # ---- a frame removed only, beside one that is replaced; then every frame removed only
    assert frames_both(c, twin, [A, B], [None, pa], K, 0.5, 8.0, tag="A removed only") == 0
    assert [e["frame_id"] for e in c.tsdf_log_get()] == [B]
    assert frames_both(c, twin, [B], None, K, 0.5, 8.0, tag="all removed only") == 0
    assert c.tsdf_log_get() == []
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_of_the_plane_level_call():
    g = GRIDS[0]
    c = ctx()
    d, b = dev(wavy_depth(W0, H0, 1)), dev(rand_bgr(W0, H0, 1))
    good = binding.tsdf_side(d, K0, POSES[1], 1.0, 0.5, 3.5, colour=b)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_depth_n([dict(add=good)])                               # no volume
    vol = cmake(c, g)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_last_n()                                                 # nothing has happened to this volume
    c.tsdf_replace_depth(add=good)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_last_n()                                                 # the last operation was the single replacement
    c.tsdf_log_enable()
    snap = lambda: ([x.tobytes() for x in arrays(c, True)], repr(c.tsdf_last()), repr(c.tsdf_replace_last()), repr(c.tsdf_log_get()))
    before = snap()
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_replace_depth_n([])                                              # n = 0 (and a NULL list)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_replace_depth_n([dict(add=good)] * 17)
    side = lambda **kw: binding.tsdf_side(kw.get("depth", d), kw.get("K", K0), kw.get("c2w", EYE), kw.get("s", 1.0), kw.get("mn", 0.5), kw.get("mx", 3.5), colour=kw.get("colour", b))
    bad_sides = [side(K=(np.nan, 68.0, 31.5, 23.5)), side(c2w=np.full((3, 4), np.inf)), side(s=0.0), side(s=np.nan), side(mn=3.0, mx=1.0),
                 side(depth=torch.zeros((H0, W0), dtype=torch.int32, device="cuda")), side(colour=dev(rand_bgr(W0 + 1, H0, 2)))]
    for n, at in ((3, 0), (5, 2), (16, 15), (1, 0)):                            # a bad pair first, in the middle and last
        for q, sd in enumerate(bad_sides):
            for kw in (dict(remove=sd), dict(add=sd), dict(remove=good, add=sd), dict()):      # the last: both sides NULL
                pairs = [dict(remove=good, add=good) for _ in range(n)]
                pairs[at] = kw
                with pytest.raises(binding.NaloError, match=r"nalo error %d: .*pair %d\b" % (ERR_ARG, at)):
                    c.tsdf_replace_depth_n(pairs)
        pairs = [dict(remove=good) for _ in range(n)]
        pairs[at] = dict(remove=good, box=((30, 0, 0), (3, 4, 4)))              # a box that leaves the grid
        with pytest.raises(binding.NaloError, match=r"nalo error %d: .*pair %d\b" % (ERR_ARG, at)):
            c.tsdf_replace_depth_n(pairs)
    c.tsdf_color_disable()
    with pytest.raises(binding.NaloError, match=r"nalo error %d: .*pair 1\b" % ERR_STATE):
        c.tsdf_replace_depth_n([dict(add=binding.tsdf_side(d, K0, POSES[1], 1.0, 0.5, 3.5)), dict(add=good)])      # a colour plane on an uncoloured volume
    c.tsdf_color_enable()
    c.tsdf_color_set((0, 0, 0), np.frombuffer(before[0][2], F).reshape((3,) + vol["tsdf"].shape))
    assert snap() == before
    c.tsdf_replace_depth_n([dict(remove=good, add=binding.tsdf_side(d, K0, POSES[2], 1.1, 0.5, 3.5, colour=b)), dict(remove=good)])      # the next legal call
    total, rows = c.tsdf_replace_last_n()
    assert rows[0]["removed"] > 300 and rows[0]["reset"] == rows[0]["removed"] and rows[0]["added"] > 300 and rows[1]["removed"] > 0
    c.close()


def test_refusals_of_the_frame_level_call():
    w, h = 80, 48
    c, sa, sb, tdm = frames_context(w, h)
    K, A, B = sa["K"], tdm.FID, tdm.FID + 1
    pa, pb, pc = tdm.C2W, moved_pose(tdm.C2W, (0.05, -0.03, 0.04)), moved_pose(tdm.C2W, (-0.04, 0.02, 0.06))
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_frames([A], [pa], K, 0.5, 8.0)                           # no volume
    cmake(c, FRAME_GRID)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_frames([A], [pa], K, 0.5, 8.0)                           # the log is off
    c.tsdf_log_enable()
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)
    c.tsdf_integrate_frame(B, pa, K, 0.5, 8.0)
    c.tsdf_replace_frames([A, B], [pb, pb], K, 0.5, 8.0)
    snap = lambda: ([x.tobytes() for x in arrays(c, True)], repr(c.tsdf_last()), repr(c.tsdf_replace_last()), repr(c.tsdf_replace_last_n()), repr(c.tsdf_log_get()))
    before = snap()

    def refused(code, *a, **kw):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % code):
            c.tsdf_replace_frames(*a, **kw)
        assert snap() == before

    refused(ERR_ARG, [], [], K, 0.5, 8.0)
    refused(ERR_ARG, list(range(17)), [pa] * 17, K, 0.5, 8.0)
    refused(ERR_ARG, [A, B, A], [pc, pc, pa], K, 0.5, 8.0)                      # a frame twice
    refused(ERR_ARG, [A, B, A + 7], [pc, pc, pc], K, 0.5, 8.0)                  # a frame the archive has never seen, last
    refused(ERR_ARG, [A, A + 7], [pc, None], K, 0.5, 8.0)
    for bad in (dict(K=(np.nan, 1.0, 1.0, 1.0)), dict(s=[1.0, 0.0]), dict(s=[1.0, np.nan]), dict(mn=3.0, mx=1.0), dict(poses=[pc, np.full((3, 4), np.inf)])):
        a = dict(poses=[pc, pc], K=K, mn=0.5, mx=8.0, s=1.0)
        a.update(bad)
        refused(ERR_ARG, [A, B], a["poses"], a["K"], a["mn"], a["mx"], s=a["s"])
    c.tsdf_replace_frames([B], None, K, 0.5, 8.0)                               # B has no entry now
    before = snap()
    refused(ERR_ARG, [A, B], [pc, None], K, 0.5, 8.0)                           # nothing to remove and nothing to add, last
    c.map_dense_enable(False)
    refused(ERR_STATE, [A, B], [pc, pc], K, 0.5, 8.0)                           # no dense archive
    c.map_dense_enable(True)
    c.ba_set_allreduce(lambda ptr, n: None)
    refused(ERR_STATE, [A, B], [pc, pc], K, 0.5, 8.0)                           # a sharded window
    c.ba_set_allreduce(None)
    c.tsdf_replace_frames([A, B], [pc, pc], K, 0.5, 8.0)                        # the next legal call works; B has an entry again
    assert c.tsdf_replace_last_n()[1][0]["removed"] > 300 and [e["frame_id"] for e in c.tsdf_log_get()] == [A, B]
    # ---- a list shorter than n_records for the LAST frame of the list: nothing was enqueued for the frames before it
    n_b = c.tsdf_log_get()[1]["n_records"]
    c.map_reset()
    fill_frames(c, sa, sb, w, short_b=True)
    assert len(c.map_dense_get(A)) >= c.tsdf_log_get()[0]["n_records"] and 0 < len(c.map_dense_get(B)) < n_b
    before = snap()
    refused(ERR_STATE, [A, B], [pa, pa], K, 0.5, 8.0)
    c.tsdf_replace_frames([A], [pa], K, 0.5, 8.0)                               # A alone is legal
    assert c.tsdf_replace_last_n()[1][0]["added"] > 300 and snap() != before
    c.close()


# ------------------------------------------------------------------------------------------------ 10. the device chain
def chain_window(one_call):
    """tests/test_tsdf_replace_gpu.py's chain (1224x368, W = 8, three keyframes, each fused into a coloured 256x64x256 volume when it is made) with the log on;
    after EACH keyframe all logged frames are replaced at perturbed poses and s = 1.02, in one nalo_tsdf_replace_frames (one_call) or in the loop of
    nalo_tsdf_replace_frame"""
    import lifecycle_model as lm
    import lifecycle_scenes as lsc
    import plane_cases as pc
    import plane_model as pm
    from nalo_slam_amd import synth
    WW, KF, w, h, s = 8, 3, 1224, 368, 3e-4
    win = synth.make_window(w=w, h=h, W=WW, P=8000, seed=lsc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    nF = WW + KF
    srng = np.random.RandomState(lsc.SEED + 3)
    st6 = np.zeros((nF, 6))
    st6[1:, :3] = 0.004 * srng.randn(nF - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * srng.randn(nF - 1, 3)
    mask = pc.block_mask(w, h, 2, 1, [2.0, 0.0])
    mask[2 * h // 3:, :w // 2] = 6.0
    mask[2 * h // 3:, w // 2:] = 8.0
    bgr = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    c = binding.Context(w, h, win.K, n_slots=nF)
    fids = [200 + i for i in range(WW)]
    for i in range(nF):
        c.frame_upload(i, win.images[i], mask=mask, bgr=bgr)
    c.ba_set_prior_carry(True)
    c.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=st6[:WW], frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(win.exists)
    ng0, lt0, ls0 = lm.default_history(win.exists)
    ls0[win.host == WW - 1, 0] = lm.IN
    c.ba_set_point_history(ng0, lt0, ls0)
    c.map_enable()
    c.map_dense_enable(True, 65536)
    c.tsdf_log_enable()
    cur, fused, stats = list(fids), [], []
    for kf in range(KF):
        if kf:
            c.ba_marginalize_frame(0)
            c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            cur = cur[1:] + [200 + WW - 1 + kf]
        c.ba_linearize(False)
        c.ba_linearize(True)
        hf, slot = WW - 3, WW - 3 + kf
        T = np.asarray(synth.se3_inv(win.world_to_cam[slot]), np.float64).reshape(-1)[:12].reshape(3, 4)
        assert c.dense_update_map(hf, pm.make_draws(60 + kf), T)[2] > 0
        if kf == 0:
            pts = c.map_dense_get(cur[hf])
            xyz = c.map_dense_world_points(cur[hf], T)
            ok = np.isfinite(xyz).all(1)
            lo, hi = np.percentile(xyz[ok], 2, axis=0), np.percentile(xyz[ok], 98, axis=0)
            vs = float(max((hi - lo) / np.array([256, 64, 256])) * 1.05)
            origin = 0.5 * (lo + hi) - 0.5 * vs * np.array([256, 64, 256])
            dep = 1.0 / pts["idepth"].astype(np.float64)
            dep = dep[np.isfinite(dep) & (dep > 0)]
            mn, mx = float(np.percentile(dep, 2)) * 0.5, float(np.percentile(dep, 98)) * 2.0
            c.tsdf_create(origin, vs, (256, 64, 256), 4 * vs, 16.0)
            c.tsdf_color_enable()
        c.tsdf_integrate_frame(cur[hf], T, win.K, mn, mx)
        fused.append([cur[hf], T])
        # the window has moved: every logged frame goes to a perturbed pose at s = 1.02
        for q, ft in enumerate(fused):
            ft[1] = moved_pose(ft[1], vs * np.array([0.8, -0.5, 1.1]) * (1 + q + kf))
        if one_call:
            c.tsdf_replace_frames([f for f, _ in fused], [t for _, t in fused], win.K, mn, mx, s=1.02)
            stats.append(c.tsdf_replace_last_n())
        else:
            rows = []
            for f, t in fused:
                c.tsdf_replace_frame(f, t, win.K, mn, mx, s=1.02)
                st = c.tsdf_replace_last()
                rows.append({k: st[k] for k in KEYS})
            stats.append(rows)
        ff = np.zeros(WW, np.uint8)
        ff[0] = 1
        c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
    out = [x.tobytes() for x in arrays(c, True)], c.tsdf_log_get()
    c.close()
    return out, stats


def test_three_keyframes_of_the_device_chain_with_the_window_replaced_in_one_call():
    (a, la), sa = chain_window(True)
    (b, lb), sb = chain_window(False)
    print("TSDF chain 1224x368 into 256x64x256, the window replaced in one call per keyframe:", sa)
    assert [len(rows) for _, rows in sa] == [1, 2, 3] and [rows for _, rows in sa] == sb
    assert all(r["removed"] > 0 and r["added"] > 0 for _, rows in sa for r in rows) and sum(r["removed"] for _, rows in sa for r in rows) > 1000
    assert all(max(r["written"] for r in rows) <= total["written"] <= sum(r["written"] for r in rows) for total, rows in sa)
    assert a == b and rm.log_equal(la, lb) and [e["s"] for e in la] == [1.02] * 3      # the one call per keyframe IS the loop
    (a2, la2), sa2 = chain_window(True)
    assert a2 == a and rm.log_equal(la2, la) and sa2 == sa                       # a second run gives the same bytes
