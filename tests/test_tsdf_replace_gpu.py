"""The replacement in the TSDF volume on the device (nalo_tsdf_replace_*, nalo_tsdf_log_*; include/nalo_gpu.h, "The replacement") against
tests/tsdf_replace_model.py, against the existing integration at s == 1 and against a twin context that removes and adds in two calls. Every comparison is bit
for bit in tsdf, weight and colour through the get calls and exact in the counts; against the numpy model a NaN equals a NaN whatever its payload (IEEE 754
leaves the sign of a NaN that inf / inf makes to the machine), between two device contexts not even that. The model evaluates EVERY voxel, the device only the
hull of the two culling boxes: equality is what shows the boxes to be conservative."""
import math
import time

import numpy as np
import pytest
import torch

import tsdf_color_model as cm
import tsdf_mesh_model as mm
import tsdf_model as tm
import tsdf_replace_model as rm
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth
from test_tsdf_gpu import FRAME_GRID, GRIDS, H0, K0, POSES, W0, bits_eq, ctx, frame_scene, make, planted

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4
W1, H1, K1 = 70, 33, (75.0, 73.0, 34.5, 16.0)                                  # the second plane size, with its own K
KN = (200.0, 200.0, 31.5, 23.5)                                                 # tests/test_tsdf_gpu.py's narrow camera: its box starts and ends inside a row


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rand_bgr(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def cmake(c, g, mw=None):
    c.tsdf_create(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"] if mw is None else mw)
    c.tsdf_color_enable()
    return cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"] if mw is None else mw)


def sides(depth, K, c2w, s, mn, mx, bgr=None):
    """one side for the device (fresh contiguous tensors) and for the model"""
    return binding.tsdf_side(dev(depth), K, c2w, s, mn, mx, colour=None if bgr is None else dev(bgr)), rm.side(depth, K, c2w, s, mn, mx, bgr)


def volume_bytes(c, colour):
    t, w = c.tsdf_get()
    return t.tobytes() + w.tobytes() + (c.tsdf_color_get().tobytes() if colour else b"")


def assert_volume(c, vol, tag=""):
    t, w = c.tsdf_get()
    assert mm.same_floats(t, vol["tsdf"]) and mm.same_floats(w, vol["weight"]), tag
    if "colour" in vol:
        assert mm.same_floats(c.tsdf_color_get(), vol["colour"]), tag


def replace_both(c, vol, remove=None, add=None, box=None, tag=""):
    """one replacement on the device and in the model: hull, visited, the four counts and every array must agree. remove / add: pairs from sides()"""
    c.tsdf_replace_depth(None if remove is None else remove[0], None if add is None else add[0], box)
    mr, ma = None if remove is None else remove[1], None if add is None else add[1]
    lo, hi, visited = rm.hull(vol, mr, ma, box)
    n = rm.replace(vol, mr, ma, box)
    st, last = c.tsdf_replace_last(), c.tsdf_last()
    print("replace", tag, {k: st[k] for k in ("visited", "removed", "reset", "added", "written")})
    assert (st["lo"], st["hi"], st["visited"]) == (lo, hi, visited), (tag, st, lo, hi)
    assert all(st[k] == n[k] for k in ("removed", "reset", "added", "written")), (tag, st, {k: n[k] for k in ("removed", "reset", "added", "written")})
    assert (last["lo"], last["hi"], last["visited"], last["updated"]) == (lo, hi, visited, n["written"]), (tag, last)
    for m in (n["rem"], n["add"]):                                              # the model's voxels lie in the hull
        k, j, i = np.nonzero(m)
        assert len(i) == 0 or (lo[0] <= i.min() and i.max() < hi[0] and lo[1] <= j.min() and j.max() < hi[1] and lo[2] <= k.min() and k.max() < hi[2]), tag
    assert_volume(c, vol, tag)
    return n, st


# ------------------------------------------------------------------------------------------------ 1. add only
@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("colour", [False, True])
def test_add_at_scale_one_is_the_integration_of_a_twin(gi, colour):
    g = GRIDS[gi]
    c, twin = ctx(), ctx()
    for x in (c, twin):
        (cmake if colour else make)(x, g)
    for q, (w, h, K) in enumerate(((W0, H0, K0), (W1, H1, K1), (W0, H0, K0), (W0, H0, KN))):
        depth, bgr, c2w = wavy_depth(w, h, 20 + q), rand_bgr(w, h, q) if colour else None, POSES[q % 3]
        c.tsdf_replace_depth(add=binding.tsdf_side(dev(depth), K, c2w, 1.0, 0.5, 3.5, colour=None if bgr is None else dev(bgr)))
        twin.tsdf_integrate_depth(dev(depth), K, c2w, 0.5, 3.5, colour=None if bgr is None else dev(bgr))
        assert c.tsdf_last() == twin.tsdf_last() and c.tsdf_last()["updated"] > 100, q
        st = c.tsdf_replace_last()
        assert st["added"] == st["written"] == c.tsdf_last()["updated"] and st["removed"] == st["reset"] == 0
        assert volume_bytes(c, colour) == volume_bytes(twin, colour), q
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
            twin.tsdf_replace_last()                                            # the twin's last operation was an integration
    c.close()
    twin.close()


@pytest.mark.parametrize("gi", [0, 1])
def test_add_at_a_scale_equals_the_model(gi):
    g = GRIDS[gi]
    c = ctx()
    vol = cmake(c, g)
    total = 0
    for q, s in enumerate((0.5, 1.25, 2.0, 1.25)):
        w, h, K = ((W0, H0, K0), (W1, H1, K1))[q % 2]
        # the plane's depths over s: the estimate puts its points at s times their depth, so the surfaces stay inside the grid at every scale
        n, _ = replace_both(c, vol, add=sides(wavy_depth(w, h, 30 + q) / F(s), K, POSES[q % 3], s, 0.5 / s, 3.5 / s, rand_bgr(w, h, 40 + q)), tag=("add", gi, s))
        assert n["added"] > 100
        total += n["added"]
    assert total > 1000 and vol["weight"].max() >= 3
    c.close()


# ------------------------------------------------------------------------------------------------ 2. remove only
def six_planes(gi):
    """the six integrations of tests/test_tsdf_gpu.py's `fused` fixture, with a colour image each"""
    return [(wavy_depth(W0, H0, 10 * gi + pi, base=2.0 + 0.02 * rnd), POSES[pi], rand_bgr(W0, H0, 60 + 3 * rnd + pi)) for rnd in range(2) for pi in range(3)]


@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("order", ["same", "reversed"])
def test_every_plane_removed_from_the_saturated_volume(gi, order):
    g = GRIDS[gi]
    c = ctx()
    vol = cmake(c, g)
    planes = [sides(d, K0, c2w, 1.0, 0.5, 3.5, b) for d, c2w, b in six_planes(gi)]
    for sd in planes:
        c.tsdf_replace_depth(add=sd[0])
        rm.replace(vol, add=sd[1])
    assert_volume(c, vol, "fused")
    assert vol["weight"].max() == 4.0 and (vol["weight"] == 4.0).sum() > 50      # weights saturated at max_weight = 4
    removed = reset = 0
    for q, sd in enumerate(planes if order == "same" else planes[::-1]):
        n, _ = replace_both(c, vol, remove=sd, tag=("remove", gi, order, q))
        removed, reset = removed + n["removed"], reset + n["reset"]
    assert removed > 2000 and 0 < reset < removed
    c.close()


def test_planted_weights_and_depths_through_the_removal():
    g, K, depth = planted(EYE)
    c = ctx(32, 16, K)
    vol = cmake(c, g)
    rng = np.random.RandomState(9)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["weight"][:] = rng.randint(2, 4, vol["weight"].shape)
    vol["colour"][:] = rng.uniform(0, 255, vol["colour"].shape)
    # the row (j = 4, k = 6) lies at y = 0, z = 1 and reads the constant 1.5 left of i = 20: d = 1 there
    up = np.nextafter(F(1.0), F(2.0))
    for i, w0 in zip(range(12, 19), (0.0, 1.0, up, 0.5, np.nan, np.inf, 3.0)):
        vol["weight"][6, 4, i] = w0
    vol["tsdf"][6, 4, 18] = np.nan
    vol["weight"][6, 4, 24] = vol["weight"][6, 4, 25] = 2.0
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    c.tsdf_color_set((0, 0, 0), vol["colour"])
    before = {k: vol[k].copy() for k in ("tsdf", "weight", "colour")}
    n, st = replace_both(c, vol, remove=sides(depth, K, EYE, 1.0, 0.5, 2.0, rand_bgr(32, 16, 1)), tag="planted")
    T, Wt, Cv = vol["tsdf"], vol["weight"], vol["colour"]
    for i in (12, 13, 15, 16):                                                  # w0 = 0, 1, 0.5, NaN: the initial values, colour too
        assert (T[6, 4, i], Wt[6, 4, i]) == (1.0, 0.0) and (Cv[:, 6, 4, i] == 0).all(), i
    assert Wt[6, 4, 14] == F(2.0 ** -23) and T[6, 4, 14] == (before["tsdf"][6, 4, 14] * up - F(1.0)) / F(2.0 ** -23)      # one ulp above 1: the quotient
    assert Wt[6, 4, 17] == np.inf and np.isnan(T[6, 4, 17]) and np.isnan(T[6, 4, 18]) and Wt[6, 4, 18] == 2.0           # +inf; t0 NaN
    # depths exactly at the range's ends are removed (d = -1 at sdf == -trunc; d = fminf(1, 2)), one ulp outside either end and 0, < 0, NaN, inf are left alone
    assert n["rem"][6, 4, 24] and T[6, 4, 24] == (before["tsdf"][6, 4, 24] * F(2.0) + F(1.0)) / F(1.0) and n["rem"][6, 4, 25] and T[6, 4, 25] == before["tsdf"][6, 4, 25] * F(2.0) - F(1.0)
    for i in (20, 21, 22, 23, 26, 27):
        assert not n["rem"][6, 4, i] and T[6, 4, i] == before["tsdf"][6, 4, i] and Wt[6, 4, i] == before["weight"][6, 4, i]
    assert not n["rem"][7, 3, 20] and n["rem"][7, 4, 19]                        # sdf just below -trunc is left alone
    assert n["reset"] >= 4 and st["lo"][0] == 0 and st["hi"][0] == 40
    c.close()


def test_one_add_and_its_removal_and_the_round_trip_with_room_in_the_weight():
    g = GRIDS[0]
    c = ctx()
    cmake(c, g, mw=64.0)
    initial = volume_bytes(c, True)
    planes = [binding.tsdf_side(dev(d), K0, c2w, 1.0, 0.5, 3.5, colour=dev(b)) for d, c2w, b in six_planes(0)]
    c.tsdf_replace_depth(add=planes[0])
    added = c.tsdf_replace_last()["added"]
    assert added > 300 and volume_bytes(c, True) != initial
    c.tsdf_replace_depth(remove=planes[0])
    st = c.tsdf_replace_last()
    assert st["removed"] == st["reset"] == st["written"] == added and volume_bytes(c, True) == initial      # colour included
    for order in (planes, planes[::-1]):
        for sd in planes:
            c.tsdf_replace_depth(add=sd)
        assert c.tsdf_get()[1].max() == 6.0
        resets = 0
        for sd in order:
            c.tsdf_replace_depth(remove=sd)
            resets += c.tsdf_replace_last()["reset"]
        assert resets > 2000 and volume_bytes(c, True) == initial
    c.close()


# ------------------------------------------------------------------------------------------------ 3. fused against remove, then add
def fused_against_twin(c, twin, vol, remove, add, box=None, tag=""):
    """the fused launch on c (and in the model) against the twin's two calls: every array bit for bit, the four counts equal"""
    n, st = replace_both(c, vol, remove, add, box, tag)
    twin.tsdf_replace_depth(remove=remove[0], box=box)
    a = twin.tsdf_replace_last()
    twin.tsdf_replace_depth(add=add[0])
    b = twin.tsdf_replace_last()
    assert (st["removed"], st["reset"], st["added"]) == (a["removed"], a["reset"], b["added"]) and max(a["written"], b["written"]) <= st["written"] <= a["written"] + b["written"], (tag, st, a, b)
    assert volume_bytes(c, "colour" in vol) == volume_bytes(twin, "colour" in vol), tag
    return n, st


@pytest.mark.parametrize("gi", [0, 1])
def test_fused_replacement_equals_remove_then_add(gi):
    g = GRIDS[gi]
    c, twin = ctx(), ctx()
    vol = cmake(c, g)
    cmake(twin, g)
    d0, d1, b0, b1 = wavy_depth(W0, H0, 80 + gi), wavy_depth(W1, H1, 82 + gi), rand_bgr(W0, H0, 5), rand_bgr(W1, H1, 6)
    first = sides(d0, K0, POSES[1], 1.0, 0.5, 3.5, b0)
    for q in range(3):                                                          # something to remove from, not saturated
        sd = sides(wavy_depth(W0, H0, 70 + q), K0, POSES[q], 1.0, 0.5, 3.5, rand_bgr(W0, H0, q))
        for x in (c, twin):
            x.tsdf_replace_depth(add=sd[0])
        rm.replace(vol, add=sd[1])
    for x in (c, twin):
        x.tsdf_replace_depth(add=first[0])
    rm.replace(vol, add=first[1])
    # a pose moved by less than a voxel, and a scale: nearly every voxel has both sides
    moved = np.concatenate([POSES[1][:, :3], POSES[1][:, 3:] + 0.4 * g["vs"]], 1)
    second = sides(d0, K0, moved, 1.01, 0.5, 3.5, b0)
    n, _ = fused_against_twin(c, twin, vol, first, second, tag="moved by less than a voxel")
    assert (n["rem"] & n["add"]).sum() > 0.8 * n["rem"].sum() > 200
    # two different planes of different sizes, each with its own K
    third = sides(d1 / F(0.9), K1, POSES[2], 0.9, 0.5, 4.0, b1)
    n, _ = fused_against_twin(c, twin, vol, second, third, tag="two planes, two sizes")
    print("two planes:", n["removed"], n["added"], int((n["rem"] ^ n["add"]).sum()))
    assert n["removed"] > 200 and n["added"] > 100 and (n["rem"] ^ n["add"]).sum() > 50
    c.close()
    twin.close()


def test_fused_replacement_of_frusta_that_do_not_meet_and_of_boxes_at_every_phase():
    g = GRIDS[1]                                                                # 33 voxels a row: rows begin at every phase of a group of four
    c, twin = ctx(), ctx()
    vol = cmake(c, g)
    cmake(twin, g)
    side_at = lambda tx, seed: sides(wavy_depth(W0, H0, seed), KN, pose(0, 0, 0, (tx, 0.0, 0.0)), 1.0, 0.5, 3.5, rand_bgr(W0, H0, seed))
    left = side_at(-0.6, 40)
    for x in (c, twin):
        x.tsdf_replace_depth(add=left[0])
    rm.replace(vol, add=left[1])
    # the two frusta do not meet: the hull holds columns of voxels that belong to neither box
    right = side_at(0.99, 41)
    br, ba = (rm.frustum_box_est(vol, W0, H0, KN, sd[1]["c2w"], 1.0, 3.5) for sd in (left, right))
    assert br[1][0] < ba[0][0]
    n, st = fused_against_twin(c, twin, vol, left, right, tag="frusta that do not meet")
    assert n["removed"] > 0 and n["added"] > 0 and not (n["rem"] & n["add"]).any() and st["lo"][0] == br[0][0] and st["hi"][0] == ba[1][0]
    # tests/test_tsdf_gpu.py's eight camera offsets on the ADD side only, the remove side being the add of the step before: the two boxes start at different
    # phases of a group of four, and lanes at either end have one side alone
    seen, prev = set(), right
    for k, tx in enumerate((0.9, 0.93, 0.96, 0.99, 1.02, 1.05, -0.6, -0.63)):
        nxt = side_at(tx, 42 + k)
        n, st = fused_against_twin(c, twin, vol, prev, nxt, tag=("offset", tx))
        br, ba = (rm.frustum_box_est(vol, W0, H0, KN, sd[1]["c2w"], 1.0, 3.5) for sd in (prev, nxt))
        seen.add((br[0][0] % 4, ba[0][0] % 4))
        assert n["removed"] > 0 and n["added"] > 0 and (n["rem"] ^ n["add"]).any()
        prev = nxt
    assert len({a for a, _ in seen} | {b for _, b in seen}) >= 3 and any(a != b for a, b in seen), seen
    c.close()
    twin.close()


def test_a_callers_box_at_every_phase_and_the_voxels_beyond_its_faces():
    g = dict(origin=(-1.5, -1.5, 0.0), vs=0.1, dims=(30, 30, 36), trunc=0.2, mw=8.0)      # tests/test_tsdf_gpu.py's interior-box grid
    c, twin = ctx(), ctx()
    vol = cmake(c, g)
    cmake(twin, g)
    rng = np.random.RandomState(5)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["weight"][:] = rng.randint(1, 4, vol["weight"].shape)
    vol["colour"][:] = rng.uniform(0, 255, vol["colour"].shape)
    for x in (c, twin):
        x.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
        x.tsdf_color_set((0, 0, 0), vol["colour"])
    wide = sides(np.full((H0, W0), 1.9, F), K0, pose(0.05, -0.04, 0.3, (0.1, -0.05, 0.55)), 1.0, 0.5, 2.0, rand_bgr(W0, H0, 3))
    other = sides(wavy_depth(W0, H0, 4, base=1.7), K0, pose(-0.05, 0.02, 0.1, (0.0, 0.05, 0.5)), 1.0, 0.5, 2.0, rand_bgr(W0, H0, 4))
    takes = rm.sample(vol, wide[1])[0]
    for q, (x0, sx) in enumerate(((12, 8), (13, 8), (14, 8), (15, 8), (16, 5), (17, 2), (20, 1))):      # x ranges that start and end at every phase mod 4
        box = ((x0, 9, 14), (sx, 8, 10))                                        # inside the frustum: the side takes voxels beyond each of its six faces
        before = {k: vol[k].copy() for k in ("tsdf", "weight", "colour")}
        inb = np.zeros(takes.shape, bool)
        inb[14:24, 9:17, x0:x0 + sx] = True
        if q % 2:
            n, _ = fused_against_twin(c, twin, vol, wide, other, box, tag=("box, fused", box))
        else:
            n, _ = replace_both(c, vol, remove=wide, box=box, tag=("box, remove only", box))
            twin.tsdf_replace_depth(remove=wide[0], box=box)
            assert volume_bytes(c, True) == volume_bytes(twin, True)
        # the side takes voxels beyond every face of the box, and they survive (an add, where there is one, apart)
        assert np.array_equal(n["rem"], takes & inb) and n["rem"].any()
        beyond = takes & ~inb & ~n["add"]
        for lo_, hi_ in (((0, 0, 0), (x0, 30, 36)), ((x0 + sx, 0, 0), (30, 30, 36)), ((0, 0, 0), (30, 9, 36)), ((0, 17, 0), (30, 30, 36)), ((0, 0, 0), (30, 30, 14)), ((0, 0, 24), (30, 30, 36))):
            face = np.zeros(takes.shape, bool)
            face[lo_[2]:hi_[2], lo_[1]:hi_[1], lo_[0]:hi_[0]] = True
            assert (beyond & face).any(), (box, lo_, hi_)
        t, w = c.tsdf_get()
        col = c.tsdf_color_get()
        assert bits_eq(t[beyond], before["tsdf"][beyond]) and bits_eq(w[beyond], before["weight"][beyond]) and bits_eq(col[:, beyond], before["colour"][:, beyond])
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 4. strided views, channel orders, an uncoloured side
def test_strided_views_on_both_sides_and_one_uncoloured_side():
    """pitched and x-strided views for depth and colour on both sides inside tensors whose other elements (depth 1.3, colour 77) WOULD change a result if one
    were read; interleaved B, G, R, interleaved R, G, B and planar colour; a coloured volume with one uncoloured side"""
    g = GRIDS[0]
    c = ctx()
    vol = cmake(c, g)
    da, db, ba, bb = wavy_depth(W0, H0, 7), wavy_depth(W1, H1, 8), rand_bgr(W0, H0, 70), rand_bgr(W1, H1, 71)
    for q in range(2):
        replace_both(c, vol, add=sides(wavy_depth(W0, H0, 90 + q), K0, POSES[q], 1.0, 0.5, 3.5, rand_bgr(W0, H0, 90 + q)))
    replace_both(c, vol, add=sides(da, K0, POSES[0], 1.0, 0.5, 3.5, ba), tag="the plane that is removed below")
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
    assert not bigd[3:3 + H0, 5:5 + W0].is_contiguous() and wided[:, 1::3].stride() == (3 * W1, 3)
    n, _ = replace_both(c, vol, (rem, rm.side(da, K0, POSES[0], 1.0, 0.5, 3.5, ba)), (add, rm.side(db, K1, POSES[2], 1.1, 0.5, 3.5, bb)), tag="strided, rgb, planar")
    assert n["removed"] > 300 and n["added"] > 300
    # the control: a reader that ignored the strides, or the channel order, would have made another volume
    a, b, d = (cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"]) for _ in range(3))
    for v, dd, cc in ((a, da, ba), (b, bigd.cpu().numpy().reshape(-1)[:H0 * W0].reshape(H0, W0), ba), (d, da, ba[:, :, ::-1])):
        rm.replace(v, add=rm.side(dd, K0, POSES[0], 1.0, 0.5, 3.5, cc))
    assert not bits_eq(a["tsdf"], b["tsdf"]) and not bits_eq(a["colour"], d["colour"])
    # one uncoloured side on the coloured volume: its voxels keep their colour words
    col = vol["colour"].copy()
    n, _ = replace_both(c, vol, remove=(add, rm.side(db, K1, POSES[2], 1.1, 0.5, 3.5, bb)), add=sides(da, K0, POSES[1], 1.0, 0.5, 3.5), tag="an uncoloured add")
    only_add = n["add"] & ~n["rem"]
    assert only_add.sum() > 50 and bits_eq(vol["colour"][:, only_add], col[:, only_add]) and not bits_eq(vol["colour"][:, n["rem"]], col[:, n["rem"]])
    col = vol["colour"].copy()
    n, _ = replace_both(c, vol, remove=sides(da, K0, POSES[1], 1.0, 0.5, 3.5), tag="an uncoloured removal")
    assert n["reset"] > 0 and (col[:, n["rem"]] != 0).any() and bits_eq(vol["colour"], col)      # an uncoloured removal, its resets too, leaves every colour word alone
    c.close()


# ------------------------------------------------------------------------------------------------ 5. stream order
def test_stream_order_without_a_host_wait():
    """the planes of both sides are written on a producer stream behind 0.2 s of matmuls; the call returns while they are still queued, reads the planes only
    behind them, and nalo_tsdf_release makes the producer's next write wait for the kernel"""
    g = GRIDS[0]
    c = ctx()
    vol = make(c, g)
    d0, d1 = wavy_depth(W0, H0, 50), wavy_depth(W0, H0, 51, base=2.1)
    replace_both(c, vol, add=sides(d0, K0, POSES[0], 1.0, 0.5, 3.5), tag="warm-up")
    ta, tb = torch.full((H0, W0), 1.3, device="cuda"), torch.full((H0, W0), 1.3, device="cuda")
    s0, s1 = dev(d0), dev(d1)
    a = torch.randn(4096, 4096, device="cuda")
    out = torch.empty_like(a)
    S = torch.cuda.Stream()
    try:
        with torch.cuda.stream(S):
            torch.mm(a, a, out=out)
            S.synchronize()
            t0 = time.perf_counter()
            torch.mm(a, a, out=out)
            S.synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
            for _ in range(min(int(math.ceil(0.25 / one)) + 1, 20000)):
                torch.mm(a, a, out=out)
            ta.copy_(s0)
            tb.copy_(s1)
            behind = torch.cuda.Event()
            behind.record(S)
            c.tsdf_replace_depth(remove=binding.tsdf_side(ta, K0, POSES[0], 1.0, 0.5, 3.5), add=binding.tsdf_side(tb, K0, POSES[1], 1.0, 0.5, 3.5), stream=S.cuda_stream, release=True)
            assert not behind.query(), "the call waited for the producer stream"
            ta.fill_(1.3)                                                        # behind nalo_tsdf_release: must not reach the kernel
            tb.fill_(1.3)
        rm.replace(vol, remove=rm.side(d0, K0, POSES[0], 1.0, 0.5, 3.5), add=rm.side(d1, K0, POSES[1], 1.0, 0.5, 3.5))
        assert c.tsdf_replace_last()["removed"] > 300
        assert_volume(c, vol, "behind the producer")
    finally:
        S.synchronize()
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. the log and nalo_tsdf_replace_frame
def moved_pose(c2w, d):
    return np.concatenate([c2w[:, :3], c2w[:, 3:] + np.asarray(d, np.float64).reshape(3, 1)], 1)


def frame_sides(pts, n_records, w, h, K, c2w, s, mn, mx):
    """the side the model and a twin take for the first n_records records of a frame's dense list (None: all of them)"""
    p = pts if n_records is None else pts[:n_records]
    with np.errstate(all="ignore"):
        D, Cp = tm.frame_plane(p, w, h), cm.frame_color_plane(p, w, h)
    return sides(D, K, c2w, s, mn, mx, Cp)


@pytest.mark.parametrize("w,h", [(80, 48), (320, 240)])
def test_the_log_and_replace_frame(w, h):
    import plane_model as pm
    import test_dense_map_gpu as tdm
    sa, sb = frame_scene(w, h), frame_scene(w, h, shift=0.4)
    K, g, dims = sa["K"], FRAME_GRID, FRAME_GRID["dims"]
    c = tdm.context(sa)
    na, nb = len(sa["u"]), len(sb["u"])
    cat = lambda k: np.concatenate([sa[k], sb[k]])
    c.ba_set_points(np.concatenate([np.zeros(na, np.int32), np.ones(nb, np.int32)]), cat("u"), cat("v"), cat("idp"), np.full((na + nb, 8), 100, F), np.ones((na + nb, 8), F))
    for hf in (0, 1):
        assert c.dense_update_map(hf, pm.make_draws(w + hf), tdm.C2W)[2] > 1000
    A, B = tdm.FID, tdm.FID + 1
    twin = binding.Context(w, h, K, n_slots=1)
    vol = cmake(c, g)
    cmake(twin, g)
    log = []
    pa, pb, pc = tdm.C2W, moved_pose(tdm.C2W, (0.05, -0.03, 0.04)), moved_pose(tdm.C2W, (-0.04, 0.02, 0.06))
    # off by default: an integrate_frame leaves no entry, and replace_frame is refused
    assert c.tsdf_log_get() == []
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_frame(A, pb, K, 0.5, 8.0)
    c.tsdf_log_enable()
    # ---- the entries after nalo_tsdf_integrate_frame
    ptsA = c.map_dense_get(A)
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)
    sA = frame_sides(ptsA, None, w, h, K, pa, 1.0, 0.5, 8.0)
    twin.tsdf_replace_depth(add=sA[0])
    rm.replace(vol, add=sA[1])
    rm.log_put(log, dims, A, len(ptsA), pa, 1.0, K, 0.5, 8.0)
    assert rm.log_equal(c.tsdf_log_get(), log) and c.tsdf_log_get()[0]["n_records"] == len(ptsA) > 1000
    assert volume_bytes(c, True) == volume_bytes(twin, True)
    assert_volume(c, vol, "integrate_frame with the log on")
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)                              # the frame has an entry: use the replacement
    assert rm.log_equal(c.tsdf_log_get(), log) and volume_bytes(c, True) == volume_bytes(twin, True)
    # ---- nalo_tsdf_replace_frame against the twin's nalo_tsdf_replace_depth on the model's planes: the one plane serves both sides
    c.tsdf_replace_frame(A, pb, K, 0.6, 7.5, s=1.02)
    sA2 = frame_sides(ptsA, None, w, h, K, pb, 1.02, 0.6, 7.5)
    twin.tsdf_replace_depth(remove=sA[0], add=sA2[0])
    n = rm.replace(vol, remove=sA[1], add=sA2[1])
    rm.log_put(log, dims, A, len(ptsA), pb, 1.02, K, 0.6, 7.5)
    st = c.tsdf_replace_last()
    assert st == twin.tsdf_replace_last() and (st["removed"], st["reset"], st["added"], st["written"]) == (n["removed"], n["reset"], n["added"], n["written"]) and n["removed"] > 300 and n["added"] > 300
    assert rm.log_equal(c.tsdf_log_get(), log) and volume_bytes(c, True) == volume_bytes(twin, True)
    assert_volume(c, vol, "replace_frame")
    # ---- a second nalo_dense_update_map of the frame: the first n_records records on the remove side, the whole list on the add side
    sc2 = frame_scene(w, h, shift=0.2)
    P = len(sc2["u"])
    c.ba_set_points(np.zeros(P, np.int32), sc2["u"], sc2["v"], sc2["idp"], np.full((P, 8), 100, F), np.ones((P, 8), F))
    assert c.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] > 1000
    ptsA2 = c.map_dense_get(A)
    assert len(ptsA2) > len(ptsA) and ptsA2[:len(ptsA)].tobytes() == ptsA.tobytes()
    c.tsdf_replace_frame(A, pc, K, 0.5, 8.0)
    sA3 = frame_sides(ptsA2, None, w, h, K, pc, 1.0, 0.5, 8.0)
    assert not bits_eq(sA3[1]["depth"], sA2[1]["depth"])
    twin.tsdf_replace_depth(remove=sA2[0], add=sA3[0])
    rm.replace(vol, remove=sA2[1], add=sA3[1])
    rm.log_put(log, dims, A, len(ptsA2), pc, 1.0, K, 0.5, 8.0)
    assert c.tsdf_replace_last() == twin.tsdf_replace_last() and rm.log_equal(c.tsdf_log_get(), log) and volume_bytes(c, True) == volume_bytes(twin, True)
    assert_volume(c, vol, "replace_frame of a list that has grown")
    # ---- a shift that brings in fresh voxels, a second frame fused over them, then the first frame replaced: the resident box keeps the removal off them
    shift = (6, 0, -4)
    for x in (c, twin):
        x.tsdf_shift(shift)
    rm.log_shift(log, dims, shift)
    assert rm.log_equal(c.tsdf_log_get(), log) and log[0]["lo"] == (0, 0, 4) and log[0]["size"] == (dims[0] - 6, dims[1], dims[2] - 4)
    geo = c.tsdf_geometry()
    shifted = cm.volume(geo["origin"], g["vs"], dims, g["trunc"], g["mw"])
    assert shifted["origin"].tobytes() == geo["origin"].tobytes()
    t, wgt = c.tsdf_get()
    shifted["tsdf"][:], shifted["weight"][:], shifted["colour"][:] = t, wgt, c.tsdf_color_get()
    fresh = np.ones(t.shape, bool)
    fresh[4:, :, :dims[0] - 6] = False
    assert (wgt[fresh] == 0).all() and (wgt[~fresh] > 0).sum() > 300            # what the shift brought in is initial
    vol = shifted
    ptsB = c.map_dense_get(B)
    c.tsdf_integrate_frame(B, pa, K, 0.5, 8.0)
    sB = frame_sides(ptsB, None, w, h, K, pa, 1.0, 0.5, 8.0)
    twin.tsdf_replace_depth(add=sB[0])
    nB = rm.replace(vol, add=sB[1])
    rm.log_put(log, dims, B, len(ptsB), pa, 1.0, K, 0.5, 8.0)
    assert (nB["add"] & fresh).sum() > 50 and rm.log_equal(c.tsdf_log_get(), log) and [e["frame_id"] for e in log] == [A, B]
    box = (log[0]["lo"], log[0]["size"])
    without = dict(vol, tsdf=vol["tsdf"].copy(), weight=vol["weight"].copy(), colour=vol["colour"].copy())
    c.tsdf_replace_frame(A, pa, K, 0.5, 8.0)
    sA4 = frame_sides(ptsA2, None, w, h, K, pa, 1.0, 0.5, 8.0)
    twin.tsdf_replace_depth(remove=sA3[0], add=sA4[0], box=box)
    n = rm.replace(vol, remove=sA3[1], add=sA4[1], box=box)
    rm.replace(without, remove=sA3[1], add=sA4[1])
    rm.log_put(log, dims, A, len(ptsA2), pa, 1.0, K, 0.5, 8.0)
    assert c.tsdf_replace_last() == twin.tsdf_replace_last() and volume_bytes(c, True) == volume_bytes(twin, True)
    assert_volume(c, vol, "replace_frame behind a shift: the model WITH the resident box")
    assert not mm.same_floats(c.tsdf_get()[1], without["weight"])              # and not the model without it: the clip is exercised
    assert rm.log_equal(c.tsdf_log_get(), log) and log[0]["size"] == tuple(dims)
    # ---- remove only: the entry is dropped; NULL with no entry is refused; a frame without an entry gets one
    c.tsdf_replace_frame(B, None, K, 0.5, 8.0)
    twin.tsdf_replace_depth(remove=sB[0], box=((0, 0, 0), dims))
    rm.log_drop(log, B)
    assert rm.log_equal(c.tsdf_log_get(), log) and volume_bytes(c, True) == volume_bytes(twin, True)
    before = volume_bytes(c, True), repr(c.tsdf_last()), repr(c.tsdf_replace_last())
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_replace_frame(B, None, K, 0.5, 8.0)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_replace_frame(A + 7, pa, K, 0.5, 8.0)                            # a frame the archive has never seen
    for bad in (dict(K=(np.nan, 1.0, 1.0, 1.0)), dict(s=0.0), dict(s=np.nan), dict(mn=3.0, mx=1.0), dict(c2w=np.full((3, 4), np.inf))):
        a = dict(c2w=pa, K=K, mn=0.5, mx=8.0, s=1.0)
        a.update(bad)
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_replace_frame(A, a["c2w"], a["K"], a["mn"], a["mx"], s=a["s"])
    assert (volume_bytes(c, True), repr(c.tsdf_last()), repr(c.tsdf_replace_last())) == before and rm.log_equal(c.tsdf_log_get(), log)
    c.tsdf_replace_frame(B, pb, K, 0.5, 8.0)
    twin.tsdf_replace_depth(add=frame_sides(ptsB, None, w, h, K, pb, 1.0, 0.5, 8.0)[0])
    rm.log_put(log, dims, B, len(ptsB), pb, 1.0, K, 0.5, 8.0)
    assert rm.log_equal(c.tsdf_log_get(), log) and volume_bytes(c, True) == volume_bytes(twin, True)
    # ---- nalo_tsdf_follow moves the boxes as nalo_tsdf_shift does; an entry is dropped when its box empties
    c.tsdf_shift((0, 3, 0))
    rm.log_shift(log, dims, (0, 3, 0))
    c.tsdf_archive_enable()
    geo = c.tsdf_geometry()
    centre = geo["origin"].astype(np.float64) + (np.asarray(dims) // 2 + np.array([2, 0, -1]) + 0.5) * float(geo["voxel_size"])
    r = c.tsdf_follow(centre, (0, 0, 0), 1.0)
    assert tuple(r["shift"]) == (2, 0, -1)
    rm.log_shift(log, dims, (2, 0, -1))
    assert rm.log_equal(c.tsdf_log_get(), log) and [e["lo"] for e in log] == [(0, 0, 1)] * 2 and log[0]["size"] == (dims[0] - 2, dims[1] - 3, dims[2] - 1)
    c.tsdf_replace_frame(A, pb, K, 0.5, 8.0)                                    # A is whole again, B keeps its box
    rm.log_put(log, dims, A, len(ptsA2), pb, 1.0, K, 0.5, 8.0)
    c.tsdf_shift((0, dims[1] - 3, 0))
    rm.log_shift(log, dims, (0, dims[1] - 3, 0))
    assert rm.log_equal(c.tsdf_log_get(), log) and [e["frame_id"] for e in log] == [A]
    # ---- cleared by reset, create and disable; the switch outlives the volume
    c.tsdf_reset()
    assert c.tsdf_log_get() == []
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)
    assert len(c.tsdf_log_get()) == 1
    c.tsdf_create(g["origin"], g["vs"], dims, g["trunc"], g["mw"])
    assert c.tsdf_log_get() == []
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)
    assert len(c.tsdf_log_get()) == 1
    c.tsdf_log_enable(False)
    assert c.tsdf_log_get() == []
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)                                  # off: a second fusion of the frame is the caller's business again
    assert c.tsdf_log_get() == []
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 7. the log changes no byte; two runs
def run_once(log_on):
    import plane_model as pm
    import test_dense_map_gpu as tdm
    w, h = 80, 48
    sc = frame_scene(w, h)
    c = tdm.context(sc)
    assert c.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] > 1000
    cmake(c, FRAME_GRID)
    if log_on is not None:
        c.tsdf_log_enable(log_on)
    out = []
    c.tsdf_integrate_frame(tdm.FID, tdm.C2W, sc["K"], 0.5, 8.0)
    out.append((volume_bytes(c, True), repr(c.tsdf_last())))
    c.tsdf_shift((3, -2, 1))
    d, b = dev(wavy_depth(w, h, 3, base=2.4)), dev(rand_bgr(w, h, 3))
    c.tsdf_integrate_depth(d, sc["K"], tdm.C2W, 0.5, 8.0, colour=b)
    out.append((volume_bytes(c, True), repr(c.tsdf_last())))
    c.tsdf_replace_depth(remove=binding.tsdf_side(d, sc["K"], tdm.C2W, 1.0, 0.5, 8.0, colour=b), add=binding.tsdf_side(d, sc["K"], moved_pose(tdm.C2W, (0.03, 0.0, 0.02)), 1.03, 0.5, 8.0, colour=b))
    out.append((volume_bytes(c, True), repr(c.tsdf_last()), repr(c.tsdf_replace_last())))
    c.close()
    return out


def test_the_log_changes_no_byte_and_two_runs_agree():
    never, off, on, again = run_once(None), run_once(False), run_once(True), run_once(True)
    assert never == off == on == again


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_volume_colour_log_and_last_as_they_were():
    g = GRIDS[0]
    c = ctx()
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_depth(add=binding.tsdf_side(dev(wavy_depth(W0, H0, 1)), K0, EYE, 1.0, 0.5, 3.5))       # no volume
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_last()
    vol = make(c, g)
    d, b = dev(wavy_depth(W0, H0, 1)), dev(rand_bgr(W0, H0, 1))
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_last()                                                   # nothing has happened to this volume
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_depth(add=binding.tsdf_side(d, K0, EYE, 1.0, 0.5, 3.5, colour=b))                    # a colour plane on an uncoloured volume
    c.tsdf_color_enable()
    vol["colour"] = np.zeros((3,) + vol["tsdf"].shape, F)
    good = sides(wavy_depth(W0, H0, 1), K0, POSES[1], 1.0, 0.5, 3.5, rand_bgr(W0, H0, 1))
    replace_both(c, vol, add=good, tag="before the refusals")
    c.tsdf_log_enable()
    before = volume_bytes(c, True), repr(c.tsdf_last()), repr(c.tsdf_replace_last()), repr(c.tsdf_log_get())
    side = lambda **kw: binding.tsdf_side(kw.get("depth", d), kw.get("K", K0), kw.get("c2w", EYE), kw.get("s", 1.0), kw.get("mn", 0.5), kw.get("mx", 3.5), colour=kw.get("colour", b))
    host = binding.DevPlane()
    host.ptr, host.dtype, host.w, host.h, host.channels, host.stride_y, host.stride_x = np.zeros((H0, W0), F).ctypes.data, binding.DT_F32, W0, H0, 1, 4 * W0, 4
    bad_sides = [side(K=(np.nan, 68.0, 31.5, 23.5)), side(K=(70.0, np.inf, 31.5, 23.5)), side(c2w=pose(0, 0, 0, (np.nan, 0, 0))), side(c2w=np.full((3, 4), np.inf)),
                 side(s=0.0), side(s=-1.0), side(s=np.nan), side(s=np.inf), side(mn=np.nan), side(mx=np.inf), side(mn=3.0, mx=1.0),
                 side(depth=torch.zeros((H0, W0), dtype=torch.int32, device="cuda")), side(depth=binding.dev_plane(dev(rand_bgr(W0, H0, 2)), "hwc")), side(depth=host),
                 side(colour=dev(rand_bgr(W0 + 1, H0, 2))), side(colour=binding.dev_plane(torch.zeros((H0, W0, 3), device="cuda"), "hwc"))]
    for q, sd in enumerate(bad_sides):
        for kw in (dict(remove=sd), dict(add=sd), dict(remove=good[0], add=sd), dict(remove=sd, add=good[0])):
            with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
                c.tsdf_replace_depth(**kw)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_replace_depth()                                                  # both sides NULL
    for box in (((0, 0, 0), (0, 4, 4)), ((-1, 0, 0), (4, 4, 4)), ((30, 0, 0), (3, 4, 4)), ((0, 0, 0), (32, 24, 41)), ((0, 24, 0), (1, 1, 1))):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_replace_depth(remove=good[0], box=box)                       # a box that is empty or leaves the grid
    assert (volume_bytes(c, True), repr(c.tsdf_last()), repr(c.tsdf_replace_last()), repr(c.tsdf_log_get())) == before
    n, _ = replace_both(c, vol, remove=good, add=sides(wavy_depth(W0, H0, 2), K0, POSES[2], 1.1, 0.5, 3.5, rand_bgr(W0, H0, 2)), tag="the next legal call")
    assert n["removed"] > 300 and n["reset"] == n["removed"] and n["added"] > 300
    c.close()


# ------------------------------------------------------------------------------------------------ 9. the device chain
def chain_with_replacement(with_model):
    """tests/test_tsdf_gpu.py's chain (1224x368, W = 8, three keyframes, each fused into a 256x64x256 volume when it is made) on a coloured volume with the log
    on; after the third keyframe all three are replaced at perturbed poses, one of them at s = 1.02. with_model: tests/tsdf_replace_model.py alongside"""
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
    cur, fused, vol, stats = list(fids), [], None, []
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
        pts = c.map_dense_get(cur[hf])
        if kf == 0:
            # the volume is laid around the first keyframe's dense points (their 2nd .. 98th percentiles), the depth range around their depths
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
            if with_model:
                vol = cm.volume(origin, vs, (256, 64, 256), 4 * vs, 16.0)
        c.tsdf_integrate_frame(cur[hf], T, win.K, mn, mx)
        fused.append((cur[hf], T, pts))
        if with_model:
            rm.replace(vol, add=frame_sides(pts, None, w, h, win.K, T, 1.0, mn, mx)[1])
        ff = np.zeros(WW, np.uint8)
        ff[0] = 1
        c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
    assert [e["frame_id"] for e in c.tsdf_log_get()] == [f for f, _, _ in fused] and len(set(f for f, _, _ in fused)) == 3
    for q, (fid, T, pts) in enumerate(fused):
        Tn, sc = moved_pose(T, vs * np.array([0.8, -0.5, 1.1]) * (1 + q)), 1.02 if q == 1 else 1.0
        c.tsdf_replace_frame(fid, Tn, win.K, mn, mx, s=sc)
        stats.append(c.tsdf_replace_last())
        if with_model:
            n = rm.replace(vol, remove=frame_sides(pts, None, w, h, win.K, T, 1.0, mn, mx)[1], add=frame_sides(pts, None, w, h, win.K, Tn, sc, mn, mx)[1])
            assert all(stats[-1][k] == n[k] for k in ("removed", "reset", "added", "written")), (q, stats[-1])
    if with_model:
        assert_volume(c, vol, "the chain, replaced")
    out = volume_bytes(c, True)
    c.close()
    return out, stats


def test_three_keyframes_of_the_device_chain_replaced_at_perturbed_poses():
    a, stats = chain_with_replacement(True)
    print("TSDF chain 1224x368 into 256x64x256, replaced:", stats)
    assert all(st["removed"] > 0 and st["added"] > 0 and st["visited"] >= st["written"] for st in stats) and sum(st["removed"] for st in stats) > 1000
    b, stats2 = chain_with_replacement(False)
    assert a == b and stats == stats2                                           # two runs give the same bytes


# ------------------------------------------------------------------------------------------------ the scaled threshold, planted
def test_planted_scaled_sdf_at_the_truncation_edge():
    """s = 2 at the identity on tests/test_tsdf_gpu.py's planted grid: M = I / 2 is exact, the voxels (i, j = 4, k = 6) at z = 1 have zc = 0.5 and still read
    pixel (16 + 2 (i - 20), 8). sdf = (D - zc) * 2 exactly -trunc is taken (d = -1), one step below it is skipped - unscaled, -0.25 would pass either way -
    and exactly +trunc gives d = 1"""
    g, K, _ = planted(EYE)
    c = ctx(32, 16, K)
    vol = cmake(c, g)
    rng = np.random.RandomState(4)
    vol["tsdf"][:] = rng.uniform(-1, 1, vol["tsdf"].shape)
    vol["weight"][:] = 2.0
    vol["colour"][:] = rng.uniform(0, 255, vol["colour"].shape)
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    c.tsdf_color_set((0, 0, 0), vol["colour"])
    depth = np.full((16, 32), 9.0, F)                                           # beyond max_depth: only the planted pixels hold a usable depth
    below = F(0.25) - F(2.0 ** -25)
    assert (below - F(0.5)) * F(2.0) == F(-0.5) - F(2.0 ** -24) and below > F(0.2)
    for i, dv in ((20, 0.25), (21, below), (22, 0.75), (23, 0.5)):
        depth[8, 16 + 2 * (i - 20)] = dv
    before = vol["tsdf"].copy()
    sd = sides(depth, K, EYE, 2.0, 0.2, 2.0, rand_bgr(32, 16, 2))
    n, _ = replace_both(c, vol, remove=sd, tag="planted, s = 2: removal")
    T = vol["tsdf"]
    assert n["rem"][6, 4, 20] and T[6, 4, 20] == before[6, 4, 20] * F(2.0) + F(1.0)          # sdf * s == -trunc: d = -1
    assert not n["rem"][6, 4, 21] and T[6, 4, 21] == before[6, 4, 21] and vol["weight"][6, 4, 21] == 2.0      # just below: left alone
    assert n["rem"][6, 4, 22] and T[6, 4, 22] == before[6, 4, 22] * F(2.0) - F(1.0)          # sdf * s == trunc: d = 1
    assert n["rem"][6, 4, 23] and T[6, 4, 23] == before[6, 4, 23] * F(2.0)                   # sdf == 0
    m, _ = replace_both(c, vol, add=sd, tag="planted, s = 2: add")
    assert np.array_equal(m["add"], n["rem"]) and m["add"][6, 4, 20] and not m["add"][6, 4, 21]
    c.close()


# ------------------------------------------------------------------------------------------------ nalo_tsdf_replace_frame: colour that came later, and its refusals
def frame_context(w=80, h=48):
    import plane_model as pm
    import test_dense_map_gpu as tdm
    sc = frame_scene(w, h)
    c = tdm.context(sc)
    assert c.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] > 1000
    return c, sc, tdm


def test_a_frame_fused_before_colour_was_enabled():
    """the entry says whether the fusion moved colour: a frame fused into the uncoloured volume is taken out of tsdf and weight only, and the colour words, which
    never held it, take the add alone"""
    w, h = 80, 48
    c, sc, tdm = frame_context(w, h)
    K, A = sc["K"], tdm.FID
    twin = binding.Context(w, h, K, n_slots=1)
    for x in (c, twin):
        make(x, FRAME_GRID)
    c.tsdf_log_enable()
    pts = c.map_dense_get(A)
    pa, pb = tdm.C2W, moved_pose(tdm.C2W, (0.05, -0.03, 0.04))
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)
    plain, _ = frame_sides(pts, None, w, h, K, pa, 1.0, 0.5, 8.0)
    twin.tsdf_replace_depth(add=binding.tsdf_side(plain.keep[0], K, pa, 1.0, 0.5, 8.0))
    assert [e["coloured"] for e in c.tsdf_log_get()] == [False]
    for x in (c, twin):
        x.tsdf_color_enable()
    c.tsdf_replace_frame(A, pb, K, 0.5, 8.0)
    twin.tsdf_replace_depth(remove=binding.tsdf_side(plain.keep[0], K, pa, 1.0, 0.5, 8.0), add=frame_sides(pts, None, w, h, K, pb, 1.0, 0.5, 8.0)[0])
    assert c.tsdf_replace_last() == twin.tsdf_replace_last() and volume_bytes(c, True) == volume_bytes(twin, True)
    col = c.tsdf_color_get()
    assert (col >= 0).all() and (col > 0).sum() > 300 and [e["coloured"] for e in c.tsdf_log_get()] == [True]
    # now the entry's fusion did move colour: the next replacement takes it out of the colour words too
    c.tsdf_replace_frame(A, None, K, 0.5, 8.0)
    twin.tsdf_replace_depth(remove=frame_sides(pts, None, w, h, K, pb, 1.0, 0.5, 8.0)[0])
    assert volume_bytes(c, True) == volume_bytes(twin, True) and not c.tsdf_color_get().any() and c.tsdf_log_get() == []
    # nalo_tsdf_color_disable clears the flag: colour enabled again holds nothing of the frame
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)
    assert [e["coloured"] for e in c.tsdf_log_get()] == [True]
    c.tsdf_color_disable()
    assert [e["coloured"] for e in c.tsdf_log_get()] == [False]
    c.close()
    twin.close()


def test_replace_frame_refusals_leave_volume_colour_log_and_last_as_they_were():
    """nalo_tsdf_replace_frame's refusals of state: without a volume, without the dense archive, on a sharded window, with a list shorter than n_records. Each
    with its return code, with volume, colour, log, nalo_tsdf_last and nalo_tsdf_replace_last byte for byte as before, and with the next legal call working"""
    import plane_model as pm
    w, h = 80, 48
    c, sc, tdm = frame_context(w, h)
    K, A = sc["K"], tdm.FID
    pa, pb, pc = tdm.C2W, moved_pose(tdm.C2W, (0.05, -0.03, 0.04)), moved_pose(tdm.C2W, (-0.04, 0.02, 0.06))
    c.tsdf_log_enable()
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_frame(A, pa, K, 0.5, 8.0)                                # no volume
    assert c.tsdf_log_get() == []
    cmake(c, FRAME_GRID)
    c.tsdf_integrate_frame(A, pa, K, 0.5, 8.0)
    c.tsdf_replace_frame(A, pb, K, 0.5, 8.0)
    snap = lambda: (volume_bytes(c, True), repr(c.tsdf_last()), repr(c.tsdf_replace_last()), repr(c.tsdf_log_get()))

    def refused(code, *args):
        before = snap()
        for a in ((A, pc, K, 0.5, 8.0), (A, None, K, 0.5, 8.0)) + args:          # a replacement and a removal alike
            with pytest.raises(binding.NaloError, match="nalo error %d:" % code):
                c.tsdf_replace_frame(*a)
        assert snap() == before

    def legal(pose_):
        before = snap()
        c.tsdf_replace_frame(A, pose_, K, 0.5, 8.0)
        st = c.tsdf_replace_last()
        assert st["removed"] > 300 and st["added"] > 300 and snap() != before and c.tsdf_log_get()[0]["cam_to_world"].tobytes() == np.asarray(pose_, np.float64).tobytes()

    # ---- without the dense archive
    c.map_dense_enable(False)
    refused(ERR_STATE)
    c.map_dense_enable(True)
    legal(pc)
    # ---- on a sharded window
    c.ba_set_allreduce(lambda ptr, n: None)
    refused(ERR_STATE)
    c.ba_set_allreduce(None)
    legal(pa)
    # ---- a list shorter than n_records: the archives are reset and the frame comes back with the points of one wall only, while the entry survives
    n_records = c.tsdf_log_get()[0]["n_records"]
    on_wall = sc["mask"][sc["v"].astype(np.int32), sc["u"].astype(np.int32)] == 3.0
    assert 10 < on_wall.sum() < len(on_wall)
    c.map_reset()
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_replace_frame(A, pc, K, 0.5, 8.0)                                # the reset archive has never seen the frame
    P = int(on_wall.sum())
    c.ba_set_points(np.zeros(P, np.int32), sc["u"][on_wall], sc["v"][on_wall], sc["idp"][on_wall], np.full((P, 8), 100, F), np.ones((P, 8), F))
    assert 0 < c.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] < n_records
    assert 0 < len(c.map_dense_get(A)) < n_records and c.tsdf_log_get()[0]["n_records"] == n_records
    refused(ERR_STATE)
    # the list grows past n_records again: legal, and the entry takes the new length
    P = len(sc["u"])
    c.ba_set_points(np.zeros(P, np.int32), sc["u"], sc["v"], sc["idp"], np.full((P, 8), 100, F), np.ones((P, 8), F))
    assert c.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] >= n_records
    legal(pb)
    assert c.tsdf_log_get()[0]["n_records"] == len(c.map_dense_get(A)) > n_records
    # ---- without a volume again: the log went with it
    c.tsdf_destroy()
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_replace_frame(A, pa, K, 0.5, 8.0)
    assert c.tsdf_log_get() == []
    c.close()
