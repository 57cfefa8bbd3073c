"""Colour in the TSDF volume and on the mesh (include/nalo_gpu.h, "Colour") on the device against tests/tsdf_color_model.py. Every comparison is bit for bit, a
NaN as a NaN: the definitions contain only correctly rounded float operations and integer rules. Words the definition does not touch are compared by their bits,
NaN payloads included. The shapes are the smallest ones tests/test_tsdf_gpu.py and tests/test_tsdf_mesh_gpu.py use: the kernels' edges are the same."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import tsdf_color_model as cm
import tsdf_mesh_model as mm
import tsdf_model as tm
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth
from test_tsdf_gpu import FRAME_GRID, GRIDS, H0, K0, POSES, W0, bits_eq, ctx, frame_scene, make, state
from test_tsdf_mesh_gpu import grid, random_field

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4


def cmake(c, g):
    """a volume with colour on the device and in the model"""
    c.tsdf_create(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    c.tsdf_color_enable()
    return cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])


def rand_bgr(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_all(c, vol, tag="", untouched=None):
    """tsdf and weight by their bits; colour by its bits where no NaN is involved, and wholly by its bits on `untouched` (a mask over the voxels)"""
    t, w = c.tsdf_get()
    col = c.tsdf_color_get()
    assert bits_eq(t, vol["tsdf"]) and bits_eq(w, vol["weight"]), tag
    assert mm.same_floats(col, vol["colour"]), tag
    if untouched is not None:
        assert bits_eq(col[:, untouched], vol["colour"][:, untouched]), tag
    return col


def integrate_both(c, vol, depth, bgr, K, c2w, mn, mx, tag="", d_dev=None, c_dev=None, rgb=False, untouched=None):
    c.tsdf_integrate_depth(dev(depth) if d_dev is None else d_dev, K, c2w, mn, mx, colour=dev(bgr) if c_dev is None else c_dev, colour_is_rgb=rgb)
    r = cm.integrate(vol, depth, bgr, K, c2w, mn, mx)
    st = c.tsdf_last()
    h, w = depth.shape
    lo, hi = tm.frustum_box(vol, w, h, K, c2w, mx)
    assert (st["lo"], st["hi"]) == (lo, hi) and st["updated"] == r["updated"], (tag, st, lo, hi, r["updated"])
    assert_all(c, vol, tag, untouched)
    return r, st


# ------------------------------------------------------------------------------------------------ 1. integration against the model
@pytest.mark.parametrize("gi", [0, 1])
def test_integration_equals_the_model_and_an_uncoloured_twin(gi):
    g = GRIDS[gi]
    c, twin = ctx(), ctx()
    vol = cmake(c, g)
    make(twin, g)
    lit = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"]) if gi == 1 else None
    assert not c.tsdf_color_get().any()                                          # the planes start at 0.0f
    n = 0
    for pi, c2w in enumerate(POSES):                                            # w0 = 0, 1, 2 where the views overlap
        depth, bgr = wavy_depth(W0, H0, 10 * gi + pi), rand_bgr(W0, H0, 100 + 10 * gi + pi)
        r, st = integrate_both(c, vol, depth, bgr, K0, c2w, 0.5, 3.5, tag=(gi, pi))
        twin.tsdf_integrate_depth(dev(depth), K0, c2w, 0.5, 3.5)
        tt, tw = twin.tsdf_get()
        assert twin.tsdf_last() == st and bits_eq(tt, vol["tsdf"]) and bits_eq(tw, vol["weight"]), (gi, pi)
        n += r["updated"]
        if lit is not None:
            cm.integrate_literal(lit, depth, bgr, K0, c2w, 0.5, 3.5)
            assert bits_eq(lit["colour"], vol["colour"])
    assert n > 1000 and vol["weight"].max() == 3.0 and (vol["colour"] > 0).sum() > 1000
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 2. box phases and untouched voxels
def test_box_phases_scalar_ends_and_untouched_voxels_keep_their_bits():
    """tests/test_tsdf_gpu.py's boxes whose x start lies at every phase of a lane's four, on 33 voxels a row. The colour is planted: every other word a NaN with a
    payload of its own, the rest distinct finite values. Whatever the model never updates, inside a box or outside, keeps its bits."""
    g = GRIDS[1]
    c = ctx()
    vol = cmake(c, g)
    n3 = vol["colour"].size
    planted = np.random.RandomState(2).uniform(0, 255, n3).astype(F)
    planted.view(np.uint32)[::2] = 0x7FC00000 | (np.arange(n3, dtype=np.uint32)[::2] + 1)
    vol["colour"][:] = planted.reshape(vol["colour"].shape)
    c.tsdf_color_set((0, 0, 0), vol["colour"])
    assert bits_eq(c.tsdf_color_get(), vol["colour"]) and np.isnan(vol["colour"]).sum() == (n3 + 1) // 2
    never = np.ones(vol["tsdf"].shape, bool)
    seen, partial = set(), set()
    for k, tx in enumerate((0.9, 0.93, 0.96, 0.99, 1.02, 1.05, -0.6, -0.63)):
        c2w = pose(0, 0, 0, (tx, 0.0, 0.0))
        depth, bgr = wavy_depth(W0, H0, 40 + k), rand_bgr(W0, H0, 140 + k)
        w_before = vol["weight"].copy()
        # the model first, to know what stays untouched by THIS call; then device and model together
        probe = dict(vol, tsdf=vol["tsdf"].copy(), weight=vol["weight"].copy())
        up = tm.integrate(probe, depth, (200.0, 200.0, 31.5, 23.5), c2w, 0.5, 3.5)["code"] == tm.UPDATED
        never &= ~up
        r, st = integrate_both(c, vol, depth, bgr, (200.0, 200.0, 31.5, 23.5), c2w, 0.5, 3.5, tag=tx, untouched=never)
        assert np.array_equal(r["code"] == tm.UPDATED, up) and np.array_equal(vol["weight"][~up], w_before[~up])
        seen.add(st["lo"][0] % 4)
        # lanes (aligned groups of four consecutive words) with one, two or three updated voxels
        flat = np.concatenate([up.reshape(-1), np.zeros((-up.size) % 4, bool)]).reshape(-1, 4).sum(1)
        partial |= set(flat.tolist())
        inside = np.zeros(up.shape, bool)
        inside[st["lo"][2]:st["hi"][2], st["lo"][1]:st["hi"][1], st["lo"][0]:st["hi"][0]] = True
        assert r["updated"] > 0 and (inside & ~up).any() and (~inside).any()
    assert len(seen) >= 3 and seen & {1, 3} and {1, 2, 3, 4} <= partial, (seen, partial)
    assert never.any() and not never.all()
    c.close()


# ------------------------------------------------------------------------------------------------ 3. non-integer weights
def test_a_non_integer_w0_and_saturation():
    g = dict(GRIDS[1], mw=2.5)
    c = ctx()
    vol = cmake(c, g)
    depth = wavy_depth(W0, H0, 1)
    for it in range(5):                                                          # w0 = 0, 1, 2, 2.5, 2.5
        integrate_both(c, vol, depth, rand_bgr(W0, H0, 60 + it), K0, POSES[0], 0.5, 3.5, tag=it)
    assert vol["weight"].max() == 2.5 and (vol["weight"] == 2.5).sum() > 100
    c.close()


# ------------------------------------------------------------------------------------------------ 4. strided views
def test_strided_colour_views_and_a_pair_of_another_size():
    """colour views over larger tensors whose other bytes (77) WOULD change the result if one were read: interleaved and pitched, planar, planar and pitched,
    x-strided, channel 0 as B and as R; then a depth / colour pair of 40 x 30 in a context of 64 x 48"""
    g = GRIDS[0]
    c = ctx()
    vol = cmake(c, g)
    depth = wavy_depth(W0, H0, 7)
    bgr = [rand_bgr(W0, H0, 70 + k) for k in range(6)]
    big = torch.full((H0 + 6, W0 + 10, 3), 77, dtype=torch.uint8, device="cuda")
    big[3:3 + H0, 5:5 + W0] = dev(bgr[0])
    view = big[3:3 + H0, 5:5 + W0]
    assert not view.is_contiguous()
    integrate_both(c, vol, depth, bgr[0], K0, POSES[0], 0.5, 3.5, c_dev=binding.dev_plane(view, "hwc"), tag="hwc, pitched")
    chw = dev(bgr[1].transpose(2, 0, 1))
    integrate_both(c, vol, depth, bgr[1], K0, POSES[1], 0.5, 3.5, c_dev=binding.dev_plane(chw, "chw"), tag="chw")
    bigc = torch.full((3, H0 + 4, W0 + 6), 77, dtype=torch.uint8, device="cuda")
    bigc[:, 2:2 + H0, 3:3 + W0] = dev(bgr[2][:, :, ::-1].transpose(2, 0, 1))     # the tensor holds R, G, B planes
    integrate_both(c, vol, depth, bgr[2], K0, POSES[2], 0.5, 3.5, c_dev=binding.dev_plane(bigc[:, 2:2 + H0, 3:3 + W0], "chw"), rgb=True, tag="chw, pitched, rgb")
    wide = torch.full((H0, 3 * W0, 3), 77, dtype=torch.uint8, device="cuda")
    wide[:, 1::3] = dev(bgr[3])
    xs = wide[:, 1::3]
    assert xs.stride() == (9 * W0, 9, 1)
    integrate_both(c, vol, depth, bgr[3], K0, POSES[0], 0.5, 3.5, c_dev=binding.dev_plane(xs, "hwc"), tag="x-strided")
    rgb = dev(bgr[4][:, :, ::-1])
    integrate_both(c, vol, depth, bgr[4], K0, POSES[1], 0.5, 3.5, c_dev=rgb, rgb=True, tag="hwc, rgb")
    # both planes strided at once
    bigd = torch.full((H0 + 6, W0 + 10), 1.3, device="cuda")
    bigd[3:3 + H0, 5:5 + W0] = dev(depth)
    integrate_both(c, vol, depth, bgr[0], K0, POSES[2], 0.5, 3.5, d_dev=bigd[3:3 + H0, 5:5 + W0], c_dev=binding.dev_plane(view, "hwc"), tag="both pitched")
    small, sbgr = wavy_depth(40, 30, 8), rand_bgr(40, 30, 75)
    integrate_both(c, vol, small, sbgr, (44.0, 42.0, 19.5, 14.5), POSES[0], 0.5, 3.5, tag="another size")
    # the control: the surroundings do matter to a reader that ignores the strides, and so does the channel order
    a, b, d = (cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"]) for _ in range(3))
    cm.integrate(a, depth, bgr[0], K0, POSES[0], 0.5, 3.5)
    cm.integrate(b, depth, big.cpu().numpy().reshape(-1)[:H0 * W0 * 3].reshape(H0, W0, 3), K0, POSES[0], 0.5, 3.5)
    cm.integrate(d, depth, bgr[0][:, :, ::-1], K0, POSES[0], 0.5, 3.5)
    assert not bits_eq(a["colour"], b["colour"]) and not bits_eq(a["colour"], d["colour"])
    c.close()


# ------------------------------------------------------------------------------------------------ 5. nalo_tsdf_integrate_frame on a coloured volume
def planted_start(c, g):
    """weight 1 and colour 50 everywhere: an update with (0, 0, 0) then shows (it gives 25), which it would not over the initial 0.0f"""
    vol = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    vol["weight"][:] = 1.0
    vol["colour"][:] = 50.0
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    c.tsdf_color_set((0, 0, 0), vol["colour"])
    return vol


def frame_against_depth_color(c, fid, K, w, h, c2w):
    """nalo_tsdf_integrate_frame on a coloured volume against nalo_tsdf_integrate_depth_color of the two planes the model builds from nalo_map_dense_get, and
    against the model itself; min_depth = 0, so that a pixel without a record (D = 0) is usable"""
    pts = c.map_dense_get(fid)
    with np.errstate(all="ignore"):
        D = tm.frame_plane(pts, w, h)
    Cp = cm.frame_color_plane(pts, w, h)
    planted_start(c, FRAME_GRID)
    c.tsdf_integrate_frame(fid, c2w, K, 0.0, 8.0)
    st_f, (t_f, w_f), col_f = c.tsdf_last(), c.tsdf_get(), c.tsdf_color_get()
    vol = planted_start(c, FRAME_GRID)
    r, st_d = integrate_both(c, vol, D, Cp, K, c2w, 0.0, 8.0, tag=("frame", fid))
    assert st_f == st_d and bits_eq(t_f, vol["tsdf"]) and bits_eq(w_f, vol["weight"]) and bits_eq(col_f, vol["colour"])
    up = r["code"] == tm.UPDATED
    pu, pv = r["uf"][up].astype(np.int32), r["vf"][up].astype(np.int32)
    return D, Cp, int(up.sum()), int((D[pv, pu] == 0).sum())


@pytest.mark.parametrize("w,h", [(80, 48), (320, 240)])
def test_integrate_frame_on_a_coloured_volume(w, h):
    import plane_model as pm
    import test_dense_map_gpu as tdm
    sc = frame_scene(w, h)
    c = tdm.context(sc)
    make(c, FRAME_GRID)
    c.tsdf_color_enable()
    recs, runs, napp = c.dense_update_map(0, pm.make_draws(w), tdm.C2W)
    assert napp > 1000
    # the camera as the archive saw it, and a wide-angle one that stands inside the grid: voxels closer than trunc then read pixels without a record (the pose
    # and K of an integration are the call's own)
    near, K_near = np.concatenate([tdm.C2W[:, :3], np.array([[0.5], [0.1], [4.0]])], 1), (sc["K"][0] / 4, sc["K"][1] / 4, sc["K"][2], sc["K"][3])
    D1, C1, n1, _ = frame_against_depth_color(c, tdm.FID, sc["K"], w, h, tdm.C2W)
    assert n1 > 300 and (D1 > 0).sum() > 900 and np.array_equal(C1[D1 > 0], sc["bgr"][D1 > 0]) and not C1[D1 == 0].any()
    _, _, n_near, n_black = frame_against_depth_color(c, tdm.FID, K_near, w, h, near)
    assert n_black > 50 and n_near > n_black                                    # (0, 0, 0) was integrated, and so were colours of records
    # another colour image under the same pyramid, then a second nalo_dense_update_map of the frame, moved back: the LAST record's colour is the new image's
    bgr2 = (255 - sc["bgr"]).astype(np.uint8)                                    # differs from the first in every byte
    c.undist_set(w, h)
    for slot in (0, 1):
        c.frame_attach(slot, bgr_org=bgr2)
    sc2 = frame_scene(w, h, shift=0.4)
    P = len(sc2["u"])
    c.ba_set_points(np.zeros(P, np.int32), sc2["u"], sc2["v"], sc2["idp"], np.full((P, 8), 100, F), np.ones((P, 8), F))
    recs, runs, napp2 = c.dense_update_map(0, pm.make_draws(w), tdm.C2W)
    assert napp2 == napp and c.map_dense_counts(tdm.FID) == (2 * napp, 6)
    D2, C2, n2, _ = frame_against_depth_color(c, tdm.FID, sc["K"], w, h, tdm.C2W)
    both = (D1 > 0) & (D2 > 0)
    assert both.sum() > 900 and (D2[both] > D1[both] + F(0.3)).all() and np.array_equal(C2[both], bgr2[both]) and (C2[both] != C1[both]).all()
    frame_against_depth_color(c, tdm.FID, K_near, w, h, near)
    c.close()


# ------------------------------------------------------------------------------------------------ 6. colourless calls
def test_colourless_calls_on_a_coloured_volume():
    g = GRIDS[1]
    c, twin = ctx(), ctx()
    vol = cmake(c, g)
    make(twin, g)
    integrate_both(c, vol, wavy_depth(W0, H0, 1), rand_bgr(W0, H0, 80), K0, POSES[0], 0.5, 3.5)
    twin.tsdf_integrate_depth(dev(wavy_depth(W0, H0, 1)), K0, POSES[0], 0.5, 3.5)
    c.tsdf_color_enable()                                                        # a second enable changes nothing
    assert_all(c, vol, "enable twice")
    # a colourless integration: tsdf and weight move like the twin's, the colour keeps its bits
    d2 = wavy_depth(W0, H0, 2)
    for k in (c, twin):
        k.tsdf_integrate_depth(dev(d2), K0, POSES[1], 0.5, 3.5)
    assert tm.integrate(vol, d2, K0, POSES[1], 0.5, 3.5)["updated"] > 100
    assert c.tsdf_last() == twin.tsdf_last()
    col = assert_all(c, vol, "colourless integration")
    assert bits_eq(col, vol["colour"]) and all(bits_eq(a, b) for a, b in zip(c.tsdf_get(), twin.tsdf_get()))
    # the next coloured one divides by the weight that is there
    integrate_both(c, vol, wavy_depth(W0, H0, 3), rand_bgr(W0, H0, 81), K0, POSES[2], 0.5, 3.5)
    c.tsdf_reset()
    vol = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    assert_all(c, vol, "reset")
    assert not c.tsdf_color_get().any()
    integrate_both(c, vol, wavy_depth(W0, H0, 4), rand_bgr(W0, H0, 82), K0, POSES[0], 0.5, 3.5)
    # disable and enable again: zeros under the weight that is there
    c.tsdf_color_disable()
    c.tsdf_color_disable()
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_color_get()
    c.tsdf_color_enable()
    vol["colour"][:] = 0.0
    assert_all(c, vol, "enabled again")
    integrate_both(c, vol, wavy_depth(W0, H0, 5), rand_bgr(W0, H0, 83), K0, POSES[0], 0.5, 3.5)
    # create replaces the volume without colour
    make(c, GRIDS[0])
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_color_view()
    c.tsdf_integrate_depth(dev(d2), K0, POSES[1], 0.5, 3.5)
    c.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 7. transfers and views
def test_color_get_set_round_trips_and_the_view():
    g = GRIDS[1]
    nx, ny, nz = g["dims"]
    c = ctx()
    vol = cmake(c, g)
    rng = np.random.RandomState(11)
    for lo, size in (((0, 0, 0), (3, 2, 2)), ((nx - 5, ny - 3, nz - 1), (5, 3, 1)), ((0, ny - 1, 0), (nx, 1, nz)), ((nx - 1, 0, nz - 2), (1, ny, 2)), ((7, 3, 1), (9, 5, 3)), ((0, 0, 0), (1, 1, 1)),
                     ((nx - 1, ny - 1, nz - 1), (1, 1, 1))):
        blk = rng.randint(0, 2 ** 32, (3,) + size[::-1], dtype=np.uint64).astype(np.uint32).view(F)      # every bit pattern, NaN payloads among them
        blk.view(np.uint32).reshape(-1)[:2] = (0x7FC12345, 0xFFA00001)
        blk.view(np.uint32).reshape(-1)[-1] = 0x7F800001
        c.tsdf_color_set(lo, blk)
        sl = (slice(None),) + tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
        vol["colour"][sl] = blk
        assert bits_eq(c.tsdf_color_get(lo, size), blk) and bits_eq(c.tsdf_color_get(), vol["colour"]), (lo, size)
    t, w = c.tsdf_get()
    assert bits_eq(t, vol["tsdf"]) and bits_eq(w, vol["weight"])                # the other two arrays were not touched
    v = c.tsdf_color_view()
    assert v.shape == (3, nz, ny, nx) and v.stream == c.L.nalo_stream(c.h_)
    c.sync()
    tv = torch.as_tensor(v, device="cuda")
    assert tv.shape == (3, nz, ny, nx) and tv.data_ptr() == v.ptr and bits_eq(tv.cpu().numpy(), vol["colour"])
    tv[2, 0, 0, 0] = 0.125                                                       # zero-copy: a write through the tensor is the volume's
    torch.cuda.synchronize()
    assert c.tsdf_color_get((0, 0, 0), (1, 1, 1))[2, 0, 0, 0] == 0.125
    for lo, size in (((-1, 0, 0), (1, 1, 1)), ((nx, 0, 0), (1, 1, 1)), ((0, 0, 0), (nx + 1, 1, 1)), ((0, 0, 0), (1, 0, 1)), ((0, 0, nz - 1), (1, 1, 2))):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            c.tsdf_color_get(lo, size)
    c.close()


def test_stream_order_without_a_host_wait():
    """depth and colour are produced behind at least 0.2 s of matmuls on a torch stream: the call returns while they run, integrates the right data, and with the
    release both tensors are overwritten on that stream right after"""
    g = GRIDS[1]
    c = ctx()
    vol = cmake(c, g)
    right, wrong = wavy_depth(W0, H0, 21), (wavy_depth(W0, H0, 21) + F(0.7)).astype(F)
    cr, cw = rand_bgr(W0, H0, 90), rand_bgr(W0, H0, 91)
    d_right, d_wrong, c_right, c_wrong = dev(right), dev(wrong), dev(cr), dev(cw)
    t, tc = torch.empty_like(d_right), torch.empty_like(c_right)
    integrate_both(c, vol, wrong, cw, K0, POSES[0], 0.5, 3.5)                    # steady state: the events exist
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
            reps = min(int(math.ceil(0.25 / one)) + 1, 20000)
            for release in (False, True):
                t.copy_(d_wrong)
                tc.copy_(c_wrong)
                for _ in range(reps):
                    torch.mm(a, a, out=out)
                t.copy_(d_right)
                tc.copy_(c_right)
                behind = torch.cuda.Event()
                behind.record(S)
                c.tsdf_integrate_depth(t, K0, POSES[1], 0.5, 3.5, release=release, colour=tc)      # stream=None: torch's current stream, S
                returned_early = not behind.query()
                if not release:
                    c.tsdf_release(S.cuda_stream)
                t.fill_(1.9)                                                     # a usable depth and another colour, on S, directly after
                tc.fill_(200)
                assert returned_early, "nalo_tsdf_integrate_depth_color waited for the producer stream (release=%s, %d matmuls of %.2e s)" % (release, reps, one)
                r = cm.integrate(vol, right, cr, K0, POSES[1], 0.5, 3.5)
                assert c.tsdf_last()["updated"] == r["updated"]
                assert_all(c, vol, ("stream order", release))
                S.synchronize()
    finally:
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. mesh colours
def random_colour(vol, seed):
    rng = np.random.RandomState(seed)
    col = rng.uniform(-60, 320, vol["colour"].shape).astype(F)                   # below 0 and above 255 among them
    flat = col.reshape(-1)
    for value, step in ((np.nan, 31), (np.inf, 59), (-np.inf, 61), (254.5, 37), (0.49, 67)):
        flat[rng.randint(0, step)::step] = value
    vol["colour"][:] = col
    return vol


def cplant(c, vol):
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    c.tsdf_color_set((0, 0, 0), vol["colour"])


def mesh_color_both(c, vol, mw, lo=None, size=None, literal=False, tag=""):
    """the coloured mesh against the model, and its geometry against a plain nalo_tsdf_mesh of the same volume"""
    xyz, tri, rgba = c.tsdf_mesh(mw, lo, size, colour=True)
    counts = c.tsdf_mesh_counts
    want = cm.mesh_colours_literal(vol, mw, lo, size) if literal else cm.mesh_colours(vol, mw, lo, size)
    assert rgba.dtype == np.uint8 and rgba.shape == want.shape == (len(xyz), 4) and np.array_equal(rgba, want), tag
    px, pt = c.tsdf_mesh(mw, lo, size)
    assert c.tsdf_mesh_counts == counts == (len(xyz), len(tri)) and xyz.tobytes() == px.tobytes() and np.array_equal(tri, pt), tag
    wx, wt = mm.mesh(vol, mw, lo, size)
    assert mm.same_floats(xyz, wx) and np.array_equal(tri, wt), tag
    return xyz, tri, rgba


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (5, 3, 2), (33, 17, 5)])
def test_mesh_colours_on_a_random_field(dims):
    c = ctx()
    g = grid(dims)
    vol = random_colour(random_field(cmake(c, g), sum(dims)), 7 + sum(dims))
    cplant(c, vol)
    for mw in (1.0, 0.5):
        xyz, tri, rgba = mesh_color_both(c, vol, mw, literal=mw == 1.0, tag=(dims, mw))
        if min(dims) >= 3:
            assert len(tri) > 100 and np.isnan(xyz).any() and (rgba[:, 3] == 255).all()
            assert (rgba[:, :3] == 0).any() and (rgba[:, :3] == 255).any() and len(np.unique(rgba[:, :3])) > 100
    c.close()


def test_mesh_colours_of_sub_boxes_at_every_phase():
    c = ctx()
    g = grid((23, 11, 9))
    vol = random_colour(random_field(cmake(c, g), 5, p_invalid=0.05), 6)
    cplant(c, vol)
    for phase in range(4):
        for lo, size in (((4 + phase, 2, 1), (9, 5, 4)), ((phase, 0, 0), (7, 11, 9)), ((8 + phase, 3, 2), (11, 7, 6)), ((12 + phase, 10, 8), (2, 1, 1))):
            assert lo[0] % 4 == phase
            mesh_color_both(c, vol, 1.0, lo, size, literal=True, tag=(lo, size))
    c.close()


def test_mesh_colours_of_a_fused_volume():
    """integrated, not planted: the colours of a fused surface are the averages of the images' bytes, so every vertex colour lies within their range"""
    g = GRIDS[0]
    c = ctx()
    vol = cmake(c, g)
    for pi, c2w in enumerate(POSES):
        bgr = rand_bgr(W0, H0, 100 + pi)
        bgr[:, :, 0] = np.clip(bgr[:, :, 0], 200, 255)                            # B high, R low
        bgr[:, :, 2] = np.clip(bgr[:, :, 2], 0, 55)
        integrate_both(c, vol, wavy_depth(W0, H0, pi), bgr, K0, c2w, 0.5, 3.5, tag=pi)
    xyz, tri, rgba = mesh_color_both(c, vol, 1.0)
    assert len(tri) > 200 and (rgba[:, 2] >= 200).all() and (rgba[:, 0] <= 55).all()                  # R, G, B order on the way out
    c.close()


# ------------------------------------------------------------------------------------------------ 9. buffer growth and views
def test_growing_buffers_the_colour_view_and_repeatability():
    c = ctx()
    g = grid((32, 24, 40))
    vol = random_colour(random_field(cmake(c, g), 21), 22)
    cplant(c, vol)
    big = mm.mesh(vol, 1.0)
    small_box = ((3, 2, 1), (6, 5, 4))
    assert len(big[0]) > (1 << 14) and len(big[1]) > (1 << 15)                  # beyond the first capacity of the buffers
    first = mesh_color_both(c, vol, 1.0, tag="larger than the first capacity")
    mesh_color_both(c, vol, 1.0, *small_box, literal=True, tag="a smaller one")
    again = mesh_color_both(c, vol, 1.0, tag="the larger again")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))        # two runs give the same bytes
    # mesh_color_both ends on a plain mesh: the colour view is gone, the mesh view is not
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_mesh_color_view()
    assert c.tsdf_mesh_view()[0].shape == (len(big[0]), 3)
    # download=False, then the views' tensors against the downloaded twin
    assert c.tsdf_mesh(1.0, download=False, colour=True) == (len(big[0]), len(big[1]))
    vc = c.tsdf_mesh_color_view()
    vx, vt = c.tsdf_mesh_view()
    assert vc.shape == (len(big[0]), 4) and vc.stream == c.L.nalo_stream(c.h_) and vx.shape == (len(big[0]), 3)
    c.sync()
    tc, tx, tt = (torch.as_tensor(v, device="cuda") for v in (vc, vx, vt))
    assert tc.data_ptr() == vc.ptr and tc.dtype == torch.uint8
    assert np.array_equal(tc.cpu().numpy(), first[2]) and mm.same_floats(tx.cpu().numpy(), first[0]) and np.array_equal(tt.cpu().numpy(), first[1])
    # the view follows the next coloured mesh: the small one's count, in the same buffer
    nvs = len(mm.mesh(vol, 1.0, *small_box)[0])
    assert c.tsdf_mesh(1.0, *small_box, download=False, colour=True)[0] == nvs
    sc = c.tsdf_mesh_color_view()
    assert sc.ptr == vc.ptr and sc.shape == (nvs, 4)
    # a fresh context whose FIRST mesh is the large coloured one; and one whose buffers a plain mesh grew before colour came
    for plain_first in (False, True):
        c2 = ctx()
        cmake(c2, g)
        cplant(c2, vol)
        if plain_first:
            assert c2.tsdf_mesh(1.0, download=False) == (len(big[0]), len(big[1]))
        assert c2.tsdf_mesh(1.0, download=False, colour=True) == (len(big[0]), len(big[1]))
        c2.sync()
        assert np.array_equal(torch.as_tensor(c2.tsdf_mesh_color_view(), device="cuda").cpu().numpy(), first[2])
        ux, ut = (torch.as_tensor(v, device="cuda").cpu().numpy() for v in c2.tsdf_mesh_view())
        assert mm.same_floats(ux, first[0]) and np.array_equal(ut, first[1])
        c2.close()
    c.close()


# ------------------------------------------------------------------------------------------------ 10. refusals
def mesh_color_once(c, mw, capv, capt, capc, lo=None, size=None, fill=9):
    """ONE nalo_tsdf_mesh_color call with sentinel-filled host arrays of the given caps (None: no array): (rc, xyz, tri, rgba, n_vertices, n_triangles)"""
    a, cc = binding.TsdfMeshArgs(), binding.TsdfMeshColorArgs()
    if lo is not None:
        a.use_box = 1
        a.lo[:] = [int(v) for v in lo]
        a.size[:] = [int(v) for v in size]
    a.min_weight = mw
    xyz = None if capv is None else np.full((max(capv, 1), 3), fill, F)
    tri = None if capt is None else np.full((max(capt, 1), 3), fill, np.int32)
    rgba = None if capc is None else np.full((max(capc, 1), 4), fill, np.uint8)
    a.cap_vertices, a.cap_triangles, cc.cap = capv or 0, capt or 0, capc or 0
    a.xyz = None if xyz is None else xyz.ctypes.data_as(binding.c_fp)
    a.tri = None if tri is None else tri.ctypes.data_as(binding.c_ip)
    cc.rgba = None if rgba is None else rgba.ctypes.data_as(binding.c_u8p)
    rc = c.L.nalo_tsdf_mesh_color(c.h_, C.byref(a), C.byref(cc))
    return rc, xyz, tri, rgba, int(a.n_vertices), int(a.n_triangles)


def colour_rc(c, depth_plane, colour_plane, rgb=0):
    a = binding.TsdfIntegrateArgs()
    a.depth = depth_plane
    a.K[:] = K0
    a.camToWorld[:] = [float(v) for v in np.asarray(EYE, np.float64).reshape(-1)]
    a.min_depth, a.max_depth = 0.5, 3.5
    return c.L.nalo_tsdf_integrate_depth_color(c.h_, C.byref(a), None if colour_plane is None else C.byref(colour_plane), rgb)


def test_refusals_leave_volume_colour_context_and_the_previous_mesh():
    c = ctx()
    d, col = dev(wavy_depth(W0, H0, 30)), dev(rand_bgr(W0, H0, 31))
    good_d, good_c = binding.dev_plane(d), binding.dev_plane(col, "hwc")
    one3, lo_a, sz_a = np.zeros((3, 1, 1, 1), F), np.zeros(3, np.int32), np.ones(3, np.int32)
    ip, fp = binding.c_ip, binding.c_fp
    cv, mv, ma, mc = binding.TsdfColorVolumeView(), binding.TsdfMeshColorDev(), binding.TsdfMeshArgs(), binding.TsdfMeshColorArgs()
    ma.min_weight = 1.0

    def every_new_call():
        return [c.L.nalo_tsdf_color_get(c.h_, lo_a.ctypes.data_as(ip), sz_a.ctypes.data_as(ip), one3.ctypes.data_as(fp)),
                c.L.nalo_tsdf_color_set(c.h_, lo_a.ctypes.data_as(ip), sz_a.ctypes.data_as(ip), one3.ctypes.data_as(fp)), c.L.nalo_tsdf_color_view(c.h_, C.byref(cv)),
                colour_rc(c, good_d, good_c), c.L.nalo_tsdf_mesh_color(c.h_, C.byref(ma), C.byref(mc)), c.L.nalo_tsdf_mesh_color_view(c.h_, C.byref(mv))]

    # no volume
    assert every_new_call() == [ERR_STATE] * 6 and c.L.nalo_tsdf_color_enable(c.h_) == ERR_STATE and c.L.nalo_tsdf_color_disable(c.h_) == ERR_STATE
    g = GRIDS[1]
    vol = make(c, g)
    d0 = wavy_depth(W0, H0, 30)
    c.tsdf_integrate_depth(dev(d0), K0, POSES[0], 0.5, 3.5)
    tm.integrate(vol, d0, K0, POSES[0], 0.5, 3.5)
    xyz0, tri0 = c.tsdf_mesh(1.0)
    nv, nt = len(xyz0), len(tri0)
    assert nv > 50 and nt > 50
    # a volume without colour: the volume and its mesh stay
    before = state(c)
    assert every_new_call() == [ERR_STATE] * 6 and c.L.nalo_tsdf_color_disable(c.h_) == 0
    assert state(c) == before and c.tsdf_mesh_view()[0].shape == (nv, 3)
    # colour on, one coloured integration, one coloured mesh
    c.tsdf_color_enable()
    vol["colour"] = np.zeros((3,) + vol["tsdf"].shape, F)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_mesh_color_view()                                                # before any coloured mesh (a plain one exists)
    integrate_both(c, vol, wavy_depth(W0, H0, 32), rand_bgr(W0, H0, 33), K0, POSES[1], 0.5, 3.5)
    xyz, tri, rgba = mesh_color_both(c, vol, 1.0, literal=True)
    nv, nt = len(xyz), len(tri)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_mesh_color_view()                                                # after a plain mesh (mesh_color_both ends on one)
    c.tsdf_mesh(1.0, download=False, colour=True)

    def cstate():
        return state(c) + (c.tsdf_color_get().tobytes(),)

    def device_mesh():
        c.sync()
        return tuple(torch.as_tensor(t, device="cuda").cpu().numpy().tobytes() for t in c.tsdf_mesh_view() + (c.tsdf_mesh_color_view(),))

    before, mesh_before = cstate(), device_mesh()
    assert mesh_before[2] == rgba.tobytes()
    # colour planes that are refused: on the host, of the wrong size, of the wrong dtype, with one channel, NULL; and a refused depth plane next to a good colour
    host = np.zeros((H0, W0, 3), np.uint8)
    small = torch.zeros((H0 - 1, W0, 3), dtype=torch.uint8, device="cuda")
    f32 = torch.zeros((H0, W0, 3), device="cuda")
    u16 = torch.zeros((H0, W0, 3), dtype=torch.int16, device="cuda").view(torch.int16)
    mono = torch.zeros((H0, W0), dtype=torch.uint8, device="cuda")
    bad_planes = [binding.DevPlane(host.ctypes.data, binding.DT_U8, W0, H0, 3, 3 * W0, 3, 1), binding.dev_plane(small, "hwc"), binding.dev_plane(f32, "hwc"),
                  binding.DevPlane(u16.data_ptr(), binding.DT_U16, W0, H0, 3, 6 * W0, 6, 2), binding.dev_plane(mono), binding.DevPlane(None, binding.DT_U8, W0, H0, 3, 3 * W0, 3, 1),
                  binding.DevPlane(col.data_ptr(), binding.DT_U8, W0, H0, 3, 3 * W0, 1, 1), None]
    for k, p in enumerate(bad_planes):
        assert colour_rc(c, good_d, p) == ERR_ARG, k
    assert colour_rc(c, binding.dev_plane(mono), good_c) == ERR_ARG and c.L.nalo_tsdf_integrate_depth_color(c.h_, None, C.byref(good_c), 0) == ERR_ARG
    assert cstate() == before and device_mesh() == mesh_before
    # get / set: blocks that leave the grid, no array
    nx, ny, nz = g["dims"]
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_color_set((nx, 0, 0), one3)
    assert c.L.nalo_tsdf_color_set(c.h_, lo_a.ctypes.data_as(ip), sz_a.ctypes.data_as(ip), None) == ERR_ARG
    assert c.L.nalo_tsdf_color_get(c.h_, lo_a.ctypes.data_as(ip), sz_a.ctypes.data_as(ip), None) == ERR_ARG and c.L.nalo_tsdf_color_view(c.h_, None) == ERR_ARG
    # the mesh: refused before anything is queued - both counts 0, every host array untouched
    for kw in (dict(mw=np.nan), dict(lo=(nx, 0, 0), size=(1, 1, 1)), dict(lo=(0, 0, 0), size=(nx + 1, 1, 1)), dict(capc=-1)):
        rc, x, t, r, n1, n2 = mesh_color_once(c, kw.get("mw", 1.0), nv, nt, kw.get("capc", nv), kw.get("lo"), kw.get("size"))
        assert rc == ERR_ARG and (n1, n2) == (0, 0) and (x == 9).all() and (t == 9).all() and (r == 9).all(), kw
    mc2 = binding.TsdfMeshColorArgs()
    mc2.cap = 5                                                                  # a cap without an array
    assert c.L.nalo_tsdf_mesh_color(c.h_, C.byref(ma), C.byref(mc2)) == ERR_ARG and c.L.nalo_tsdf_mesh_color(c.h_, C.byref(ma), None) == ERR_ARG
    assert c.L.nalo_tsdf_mesh_color(c.h_, None, C.byref(mc)) == ERR_ARG and c.L.nalo_tsdf_mesh_color_view(c.h_, None) == ERR_ARG
    assert cstate() == before and device_mesh() == mesh_before
    # caps one below the count: refused behind the scans with both counts reported, the sentinel-filled arrays intact, the same device mesh
    for capv, capt, capc in ((nv, nt, nv - 1), (nv - 1, nt, nv), (nv, nt - 1, nv), (nv, nt, 0), (None, None, nv - 1)):
        rc, x, t, r, n1, n2 = mesh_color_once(c, 1.0, capv, capt, capc)
        assert rc == ERR_ARG and (n1, n2) == (nv, nt) and (r == 9).all() and (x is None or ((x == 9).all() and (t == 9).all())), (capv, capt, capc)
        assert cstate() == before and device_mesh() == mesh_before
    # exactly enough is taken; colours alone too
    rc, x, t, r, n1, n2 = mesh_color_once(c, 1.0, nv, nt, nv)
    assert rc == 0 and mm.same_floats(x, xyz) and np.array_equal(t, tri) and np.array_equal(r, rgba)
    rc, x, t, r, n1, n2 = mesh_color_once(c, 1.0, None, None, nv + 3)
    assert rc == 0 and (n1, n2) == (nv, nt) and np.array_equal(r[:nv], rgba) and (r[nv:] == 9).all()
    assert cstate() == before and device_mesh() == mesh_before
    # the next legal calls are correct
    integrate_both(c, vol, wavy_depth(W0, H0, 34), rand_bgr(W0, H0, 35), K0, POSES[2], 0.5, 3.5)
    mesh_color_both(c, vol, 1.0, literal=True)
    c.close()
