"""nalo_tsdf_shift, nalo_tsdf_geometry and the two host helpers on the device (include/nalo_gpu.h, "A volume that follows the camera") against
tests/tsdf_shift_model.py. The shift copies words: every comparison is bit for bit through nalo_tsdf_get / nalo_tsdf_color_get, on volumes filled through
nalo_tsdf_set / nalo_tsdf_color_set with seeded random words, NaN payloads, infinities, -0.0f and denormals among them."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import tsdf_color_model as cm
import tsdf_model as tm
import tsdf_shift_model as sm
from nalo_slam_amd import binding
from test_tsdf_cpu import wavy_depth
from test_tsdf_gpu import FRAME_GRID, GRIDS, H0, K0, POSES, W0, bits_eq, ctx, frame_scene

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
ERR_ARG, ERR_STATE = -1, -4
SMALL = dict(origin=(-1.0, 0.5, 2.0), vs=0.125, trunc=0.25, mw=4.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def create(c, g, colour):
    c.tsdf_create(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    if colour:
        c.tsdf_color_enable()
    return (cm.volume if colour else tm.volume)(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])


def plant_words(c, vol, rng):
    """seeded words of every kind into every array, on the device and in the model; the first and the last voxel of each array hold planted words"""
    shape = vol["tsdf"].shape
    arrs = [sm.random_words(rng, shape) for _ in range(5 if vol.get("colour") is not None else 2)]
    for k, a in enumerate(arrs):
        a.reshape(-1)[0], a.reshape(-1)[-1] = 0x7FC10000 + k, 0xFFA00001 + k
    vol["tsdf"], vol["weight"] = arrs[0].view(F), arrs[1].view(F)
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    if len(arrs) == 5:
        vol["colour"] = np.stack(arrs[2:]).view(F)
        c.tsdf_color_set((0, 0, 0), vol["colour"])


def assert_bits(c, vol, tag=""):
    t, w = c.tsdf_get()
    assert bits_eq(t, vol["tsdf"]) and bits_eq(w, vol["weight"]), tag
    if vol.get("colour") is not None:
        assert bits_eq(c.tsdf_color_get(), vol["colour"]), tag


def assert_geometry(c, vol, tag=""):
    g = c.tsdf_geometry()
    base = vol.get("base", np.zeros(3, np.int64))
    assert g["base"].tolist() == [int(v) for v in base] and bits_eq(g["origin0"], np.asarray(vol.get("origin0", vol["origin"]), F)), tag
    assert bits_eq(g["origin"], np.asarray(vol["origin"], F)) and g["dims"] == tuple(vol["dims"]) and g["voxel_size"] == vol["vs"], (tag, g["origin"], vol["origin"])
    return g


def shift_both(c, vol, s, tag=""):
    c.tsdf_shift(s)
    sm.shift_volume(vol, s)
    assert_bits(c, vol, (tag, s))


def pointers(c, colour):
    t, w = c.tsdf_view()
    return (t.ptr, w.ptr) + ((c.tsdf_color_view().ptr,) if colour else ())


def snapshot(c, colour, last=True):
    """everything a refused call must leave: the arrays' bits, the geometry, the view pointers and nalo_tsdf_last"""
    t, w = c.tsdf_get()
    g = c.tsdf_geometry()
    out = [t.tobytes(), w.tobytes(), g["origin"].tobytes(), g["origin0"].tobytes(), g["base"].tobytes(), pointers(c, colour)]
    if colour:
        out.append(c.tsdf_color_get().tobytes())
    if last:
        out.append(repr(c.tsdf_last()))
    return out


# ------------------------------------------------------------------------------------------------ 1. small grids
def small_shifts(dims):
    out = [(s0, s1, s2) for s0 in range(-5, 6) for s1 in (-2, 0, 3) for s2 in (-2, 0, 3)]        # every phase of a lane's four voxels, both directions, crossed with y and z
    for a in range(3):
        for m in (dims[a] - 1, dims[a], dims[a] + 1):
            for sign in (1, -1):
                s = [0, 0, 0]
                s[a] = sign * m
                out.append(tuple(s))
    return [s for s in out if s != (0, 0, 0)]


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (5, 3, 2), (33, 17, 5), (32, 24, 40)])
def test_small_grids_at_every_phase_and_extent(dims, colour):
    """1, 8, 30 and 2805 voxels are no multiple of four (the last group is partial, and with colour the planes of 2805 start off a 16-byte boundary); 33 voxels a row
    make groups straddle rows; 32 a row take the 16-byte loads at s0 in {-4, 0, 4} and the narrower ones elsewhere. The volume is planted anew before every shift."""
    c = ctx()
    vol = create(c, dict(SMALL, dims=dims), colour)
    rng = np.random.RandomState(sum(dims) + 7 * colour)
    n_total = n_whole = 0
    for s in small_shifts(dims):
        plant_words(c, vol, rng)
        shift_both(c, vol, s)
        gone = any(abs(s[a]) >= dims[a] for a in range(3))
        if gone:                                                                # |s| of dim and dim + 1 (and whatever else exceeds a small grid) leaves a volume of initial values
            assert (vol["tsdf"].view(U) == sm.ONE).all() and (vol["weight"].view(U) == 0).all() and (not colour or (vol["colour"].view(U) == 0).all())
        n_total += 1
        n_whole += gone
    assert n_total >= 100 and n_whole >= 6 and (n_whole < n_total or max(dims) <= 2)
    assert_geometry(c, vol)
    c.close()


# ------------------------------------------------------------------------------------------------ 2. zero shift, pointers and geometry
@pytest.mark.parametrize("colour", [False, True])
def test_zero_shift_the_pointer_swap_and_the_geometry_of_a_walk(colour):
    g = dict(origin=(-12.8, -12.8, 0.3), vs=0.1, dims=(33, 17, 5), trunc=0.3, mw=4.0)
    c = ctx()
    vol = create(c, g, colour)
    rng = np.random.RandomState(3)
    plant_words(c, vol, rng)
    p0 = pointers(c, colour)
    c.tsdf_shift((0, 0, 0))                                                     # queues, swaps and allocates nothing
    assert pointers(c, colour) == p0
    assert_bits(c, vol, "zero shift")
    assert_geometry(c, vol)
    shift_both(c, vol, (1, 0, -1))
    p1 = pointers(c, colour)
    assert all(a != b for a, b in zip(p0, p1)), (p0, p1)                        # every array moved to its spare
    c.tsdf_shift((0, 0, 0))
    assert pointers(c, colour) == p1
    shift_both(c, vol, (-2, 3, 0))
    assert pointers(c, colour) == p0                                            # and back: two sets, no third
    # a walk of 50 seeded shifts: base and origin equal the formula bit for bit, and an accumulated origin would not
    acc, differ = np.asarray(vol["origin"], F).copy(), 0
    for k in range(50):
        s = rng.randint(-40, 41, 3)
        c.tsdf_shift(s)
        sm.shift_volume(vol, s)
        acc = (acc + s.astype(F) * F(g["vs"])).astype(F)
        got = assert_geometry(c, vol, k)
        differ += int(not bits_eq(got["origin"], acc))
    assert differ >= 25, differ
    back = -vol["base"]
    assert np.abs(back).max() > 0
    for a in range(3):                                                          # home one axis at a time: base returns to 0 and the origin to origin0, exactly
        s = [0, 0, 0]
        s[a] = int(back[a])
        c.tsdf_shift(s)
        sm.shift_volume(vol, s)
    got = assert_geometry(c, vol, "home")
    assert got["base"].tolist() == [0, 0, 0] and bits_eq(got["origin"], got["origin0"]) and bits_eq(got["origin"], np.asarray(g["origin"], F))
    assert_bits(c, vol, "after the walk")
    # nalo_tsdf_reset resets the values and keeps base; nalo_tsdf_create starts from base 0
    shift_both(c, vol, (2, -1, 1))
    c.tsdf_reset()
    vol["tsdf"][:], vol["weight"][:] = 1.0, 0.0
    if colour:
        vol["colour"][:] = 0.0
    assert_bits(c, vol, "reset")
    assert assert_geometry(c, vol)["base"].tolist() == [2, -1, 1]
    vol = create(c, g, False)
    assert assert_geometry(c, vol)["base"].tolist() == [0, 0, 0]
    c.close()


def test_colour_enabled_and_disabled_around_shifts():
    """colour enabled after a shift gets its spare at the next shift; disabled, both blocks go and a later enable starts from zeros"""
    c = ctx()
    vol = create(c, dict(SMALL, dims=(33, 17, 5)), False)
    rng = np.random.RandomState(9)
    plant_words(c, vol, rng)
    shift_both(c, vol, (1, 2, 0))
    c.tsdf_color_enable()
    vol["colour"] = np.zeros((3,) + vol["tsdf"].shape, F)
    assert_bits(c, vol, "enabled behind a shift")
    plant_words(c, vol, rng)
    shift_both(c, vol, (-3, 0, 1))
    shift_both(c, vol, (4, -1, 0))
    c.tsdf_color_disable()
    vol["colour"] = None
    shift_both(c, vol, (0, 1, -1))
    c.tsdf_color_enable()
    vol["colour"] = np.zeros((3,) + vol["tsdf"].shape, F)
    shift_both(c, vol, (1, 0, 0))
    assert_geometry(c, vol)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. a shifted volume is a volume
def fuse_coloured(c, vol, gi, rounds=1):
    for rnd in range(rounds):
        for pi, c2w in enumerate(POSES):
            depth = wavy_depth(W0, H0, 10 * gi + pi, base=2.0 + 0.02 * rnd)
            bgr = np.random.RandomState(100 + 10 * gi + pi + rnd).randint(0, 256, (H0, W0, 3)).astype(np.uint8)
            c.tsdf_integrate_depth(dev(depth), K0, c2w, 0.5, 3.5, colour=dev(bgr))
            cm.integrate(vol, depth, bgr, K0, c2w, 0.5, 3.5)


def twin_of(c, vol):
    """a context whose volume is created from nalo_tsdf_geometry's descriptor and filled with the model's arrays"""
    g = c.tsdf_geometry()
    d = g["desc"]
    t = ctx()
    t.tsdf_create(tuple(d.origin), d.voxel_size, tuple(d.dims), d.trunc, d.max_weight)
    t.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    if vol.get("colour") is not None:
        t.tsdf_color_enable()
        t.tsdf_color_set((0, 0, 0), vol["colour"])
    return t


def same_arrays(a, b, tag):
    if isinstance(a, dict):
        assert set(a) == set(b), tag
        return all(same_arrays(a[k], b[k], (tag, k)) for k in a)
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), tag
        return all(same_arrays(x, y, tag) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), tag
        return True
    assert a == b, (tag, a, b)
    return True


@pytest.mark.parametrize("gi", [0, 1])
def test_a_shifted_volume_is_a_volume(gi):
    g = GRIDS[gi]
    c = ctx()
    vol = create(c, g, True)
    fuse_coloured(c, vol, gi)
    assert_bits(c, vol, "fused")
    for s in ((3, -2, 1), (-1, 3, 2)):
        shift_both(c, vol, s, "fused")
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_last()                                                           # the last box was in the old indices
    geo = assert_geometry(c, vol)
    assert geo["base"].tolist() == [2, 1, 3] and (vol["weight"] > 0).sum() > 500
    t = twin_of(c, vol)
    both = (c, t)
    # a plain integration: device, twin and the model on the shifted origin agree, and the culling box of the geometry's descriptor holds every updated voxel
    depth, c2w = wavy_depth(W0, H0, 70 + gi, base=2.05), POSES[1]
    for x in both:
        x.tsdf_integrate_depth(dev(depth), K0, c2w, 0.5, 3.5)
    r = tm.integrate(vol, depth, K0, c2w, 0.5, 3.5)
    st = c.tsdf_last()
    assert st == t.tsdf_last() and st["updated"] == r["updated"] > 100
    lo, hi = binding.tsdf_frustum_box(geo["desc"], W0, H0, K0, c2w, 3.5)
    box = tm.updated_box(r["code"])
    assert (st["lo"], st["hi"]) == (tuple(lo), tuple(hi)) == tm.frustum_box(vol, W0, H0, K0, c2w, 3.5)
    assert all(lo[a] <= box[0][a] and box[1][a] <= hi[a] for a in range(3))
    assert_bits(c, vol, "integrate_depth behind shifts")
    assert_bits(t, vol, "integrate_depth on the twin")
    # a coloured one
    depth, c2w = wavy_depth(W0, H0, 80 + gi, base=1.95), POSES[2]
    bgr = np.random.RandomState(200 + gi).randint(0, 256, (H0, W0, 3)).astype(np.uint8)
    for x in both:
        x.tsdf_integrate_depth(dev(depth), K0, c2w, 0.5, 3.5, colour=dev(bgr))
    r = cm.integrate(vol, depth, bgr, K0, c2w, 0.5, 3.5)
    assert c.tsdf_last() == t.tsdf_last() and c.tsdf_last()["updated"] == r["updated"] > 100
    assert_bits(c, vol, "integrate_depth_color behind shifts")
    assert_bits(t, vol, "integrate_depth_color on the twin")
    # the readers: surface points, the coloured mesh, the ray-cast with normals and colour
    pts = [x.tsdf_surface_points(1.0) for x in both]
    assert len(pts[0]) > 100 and same_arrays(pts[0], pts[1], "surface points") and bits_eq(pts[0], tm.surface_points(vol, 1.0))
    meshes = [x.tsdf_mesh(1.0, colour=True) for x in both]
    assert len(meshes[0][1]) > 100 and same_arrays(meshes[0], meshes[1], "mesh_color")
    nx, ny, nz = g["dims"]
    sub = [x.tsdf_mesh(1.0, (1, 2, 1), (nx - 3, ny - 5, nz - 2), colour=True) for x in both]
    assert same_arrays(sub[0], sub[1], "mesh_color of a sub-box")
    casts = [x.tsdf_raycast(W0, H0, K0, POSES[0], 0.5, 3.5, 0.04, 1.0, True, True) for x in both]
    assert casts[0]["n_hit"] > 50 and casts[0]["n_normal"] > 0 and same_arrays(casts[0], casts[1], "raycast")      # not vacuous: the five-voxel-deep grid is hit by few rays
    for x in both:
        x.close()


def test_integrate_frame_behind_a_shift():
    """nalo_tsdf_integrate_frame at 80 x 48 into a shifted volume against nalo_tsdf_integrate_depth of the model's plane into a twin made from the geometry"""
    import plane_model as pm
    import test_dense_map_gpu as tdm
    w, h = 80, 48
    sc = frame_scene(w, h)
    c = tdm.context(sc)
    vol = create(c, dict(FRAME_GRID, origin=(-1.26, -0.94, 3.26)), False)       # two, two and three voxels off FRAME_GRID: the shifts below bring it there
    assert c.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] > 1000
    with np.errstate(all="ignore"):
        D = tm.frame_plane(c.map_dense_get(tdm.FID), w, h)
    plant = tm.integrate(vol, wavy_depth(w, h, 5, base=2.5), sc["K"], tdm.C2W, 0.5, 8.0)
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    assert plant["updated"] > 100
    shift_both(c, vol, (2, 0, 3))
    shift_both(c, vol, (0, -2, 0))
    t = twin_of(c, vol)
    c.tsdf_integrate_frame(tdm.FID, tdm.C2W, sc["K"], 0.5, 8.0)
    t.tsdf_integrate_depth(dev(D), sc["K"], tdm.C2W, 0.5, 8.0)
    r = tm.integrate(vol, D, sc["K"], tdm.C2W, 0.5, 8.0)
    assert c.tsdf_last() == t.tsdf_last() and c.tsdf_last()["updated"] == r["updated"] > 300
    assert_bits(c, vol, "integrate_frame behind shifts")
    assert_bits(t, vol, "the twin")
    c.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 4. no cell is lost
def triangle_rows(xyz, tri):
    """the triangles as sorted rows of nine coordinate words: a multiset that does not depend on the vertex numbering"""
    rows = np.ascontiguousarray(xyz[tri.reshape(-1)].reshape(-1, 9)).view(U)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


@pytest.mark.parametrize("s", [(8, 0, 0), (5, -3, 2), (-40, 1, 0)])
def test_no_cell_is_lost(s):
    """voxel_size 0.25 and an origin on its multiples: the voxel centres are exact in the old and in the shifted volume, so the vertices of a cell both hold
    compare bit for bit. The meshes of nalo_tsdf_shift_boxes' boxes before the shift plus the mesh of the whole volume after it are the mesh before it."""
    g = dict(origin=(-5.0, -1.5, 1.0), vs=0.25, dims=(40, 12, 12), trunc=0.5, mw=4.0)
    c = ctx()
    vol = create(c, g, False)
    rng = np.random.RandomState(17)
    shape = vol["tsdf"].shape
    smooth = np.sin(np.arange(40) * 0.45)[None, None, :] + np.cos(np.arange(12) * 0.7)[None, :, None] + np.sin(np.arange(12) * 0.9)[:, None, None]
    vol["tsdf"] = (0.4 * smooth + rng.uniform(-0.5, 0.5, shape)).astype(F)     # a seeded sign field
    vol["weight"] = (2.0 * (rng.rand(*shape) < 0.85)).astype(F)                 # under a random valid mask
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    before = triangle_rows(*c.tsdf_mesh(1.0))
    assert len(before) > 1000
    boxes = binding.tsdf_shift_boxes(g["dims"], s)
    assert boxes == sm.shift_boxes(g["dims"], s) and len(boxes["boxes"]) == {(8, 0, 0): 1, (5, -3, 2): 3, (-40, 1, 0): 1}[s]
    parts = [triangle_rows(*c.tsdf_mesh(1.0, lo, size)) for lo, size in boxes["boxes"]]
    assert all(len(p) > 0 for p in parts)
    shift_both(c, vol, s)
    parts.append(triangle_rows(*c.tsdf_mesh(1.0)))
    assert (len(parts[-1]) == 0) == (s[0] == -40)
    got = np.concatenate(parts)
    got = got[np.lexsort(got.T[::-1])]
    assert got.shape == before.shape and got.tobytes() == before.tobytes(), (s, got.shape, before.shape)
    c.close()


# ------------------------------------------------------------------------------------------------ 5. stream order
def test_stream_order_without_a_host_wait():
    """integrate -> shift -> integrate, queued behind 0.2 s of a producer's matmuls, return while those run; the result (the volume and a ray-cast of it) equals a
    twin's that synchronises after every call. nalo_tsdf_release on a second stream still orders a rewrite of the depth tensor behind both integrations."""
    g = GRIDS[1]
    c, t = ctx(), ctx()
    rng = np.random.RandomState(23)
    da, db = wavy_depth(W0, H0, 21), wavy_depth(W0, H0, 22, base=2.1)
    for x in (c, t):
        create(x, g, True)
        x.tsdf_shift((1, 0, 0))                                                 # steady state: the spares and the events exist
        x.tsdf_integrate_depth(dev(da), K0, POSES[0], 0.5, 3.5)
        x.sync()
    bgr = dev(rng.randint(0, 256, (H0, W0, 3)).astype(np.uint8))
    a_dev, b_dev = dev(da), dev(db)
    ta, tb = torch.empty_like(a_dev), torch.empty_like(b_dev)
    a = torch.randn(4096, 4096, device="cuda")
    out = torch.empty_like(a)
    S, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    s = (-3, 2, 1)
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
            ta.copy_(a_dev)
            tb.copy_(b_dev)
            behind = torch.cuda.Event()
            behind.record(S)
            c.tsdf_integrate_depth(ta, K0, POSES[1], 0.5, 3.5, release=False, colour=bgr)     # stream=None: torch's current stream, S
            c.tsdf_shift(s)
            c.tsdf_integrate_depth(tb, K0, POSES[2], 0.5, 3.5, release=False)
            returned_early = not behind.query()
            c.tsdf_release(S2.cuda_stream)
        with torch.cuda.stream(S2):
            ta.fill_(1.9)                                                       # usable depths, on the second stream, directly behind the release
            tb.fill_(1.8)
        assert returned_early, "integrate -> shift -> integrate waited for the producer stream"
        cast = c.tsdf_raycast(W0, H0, K0, POSES[0], 0.5, 3.5, 0.04, 1.0, True, True)
        t.tsdf_integrate_depth(a_dev, K0, POSES[1], 0.5, 3.5, colour=bgr)
        t.sync()
        t.tsdf_shift(s)
        t.sync()
        t.tsdf_integrate_depth(b_dev, K0, POSES[2], 0.5, 3.5)
        t.sync()
        want = t.tsdf_raycast(W0, H0, K0, POSES[0], 0.5, 3.5, 0.04, 1.0, True, True)
        assert want["n_hit"] > 50 and same_arrays(cast, want, "raycast")
        assert c.tsdf_last() == t.tsdf_last() and c.tsdf_last()["updated"] > 100
        assert same_arrays(c.tsdf_get(), t.tsdf_get(), "volume") and same_arrays(c.tsdf_color_get(), t.tsdf_color_get(), "colour")
        assert same_arrays(c.tsdf_geometry()["origin"], t.tsdf_geometry()["origin"], "origin")
        S2.synchronize()
    finally:
        S.synchronize()
        c.close()
        t.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. refusals
def shift_rc(c, s):
    a = None if s is None else np.ascontiguousarray(s, np.int32)
    return c.L.nalo_tsdf_shift(c.h_, None if a is None else a.ctypes.data_as(binding.c_ip))


def test_refusals_leave_everything_as_it_was():
    INT_MAX = 2 ** 31 - 1
    c = ctx()
    geo = binding.TsdfGeometry()
    assert shift_rc(c, (1, 0, 0)) == ERR_STATE and shift_rc(c, (0, 0, 0)) == ERR_STATE and shift_rc(c, None) == ERR_STATE       # no volume
    assert c.L.nalo_tsdf_geometry(c.h_, C.byref(geo)) == ERR_STATE
    g = dict(origin=(0.0, 0.0, 2.0), vs=2.0 ** -10, dims=(33, 17, 5), trunc=0.25, mw=4.0)      # a small box on the optical axis of POSES[0]
    vol = create(c, g, True)
    rng = np.random.RandomState(31)
    assert c.L.nalo_tsdf_geometry(c.h_, None) == ERR_ARG
    depth = np.full((H0, W0), 2.2, F)
    c.tsdf_integrate_depth(dev(depth), K0, POSES[0], 0.5, 3.5)                  # so that nalo_tsdf_last has something to lose
    assert tm.integrate(vol, depth, K0, POSES[0], 0.5, 3.5)["updated"] > 100
    shift_both(c, vol, (1, 1, 0))                                               # the spares exist: a refusal must not swap them either
    c.tsdf_integrate_depth(dev(depth), K0, POSES[0], 0.5, 3.5)
    tm.integrate(vol, depth, K0, POSES[0], 0.5, 3.5)
    before = snapshot(c, True)
    for s in (None, (INT_MAX, 0, 0), (0, -INT_MAX - 1, 0), (0, 0, (1 << 24) + 1), (-(1 << 24) - 2, 0, 0), (1, 1, INT_MAX)):
        assert shift_rc(c, s) == ERR_ARG, s
        assert snapshot(c, True) == before, s
    assert_bits(c, vol, "refused shifts")
    # base taken to exactly 2^24 is accepted (everything leaves), one more is refused
    s = ((1 << 24) - 1, 0, 0)
    shift_both(c, vol, s, "to the bound")
    assert assert_geometry(c, vol)["base"].tolist() == [1 << 24, 1, 0] and (vol["tsdf"].view(U) == sm.ONE).all()
    before = snapshot(c, True, last=False)
    assert shift_rc(c, (1, 0, 0)) == ERR_ARG and shift_rc(c, (0, 1 << 24, 0)) == ERR_ARG and snapshot(c, True, last=False) == before
    shift_both(c, vol, (-(1 << 25), -1 - (1 << 24), 0), "to the other bound")
    assert assert_geometry(c, vol)["base"].tolist() == [-(1 << 24), -(1 << 24), 0]
    assert shift_rc(c, (-1, 0, 0)) == ERR_ARG and shift_rc(c, (0, -1, 0)) == ERR_ARG
    # the next legal call works
    plant_words(c, vol, rng)
    shift_both(c, vol, (1 << 24, 1 << 24, 0), "home")
    shift_both(c, vol, (2, -1, 1), "the next legal call")
    # a voxel so large that the shifted origin overflows
    vol = create(c, dict(g, vs=1e32, trunc=1e32), False)
    plant_words(c, vol, rng)
    shift_both(c, vol, (1, 0, 0), "a huge voxel")
    before = snapshot(c, False, last=False)
    assert sm.shift_refusal(vol["origin0"], vol["base"], (1 << 22, 0, 0), vol["vs"]) and not sm.shift_refusal(vol["origin0"], vol["base"], (1 << 20, 0, 0), vol["vs"])
    assert shift_rc(c, (1 << 22, 0, 0)) == ERR_ARG and shift_rc(c, (0, 0, -(1 << 23))) == ERR_ARG and snapshot(c, False, last=False) == before
    shift_both(c, vol, (0, 1 << 20, 0), "still finite")
    assert np.isfinite(assert_geometry(c, vol)["origin"]).all()
    c.close()


# ------------------------------------------------------------------------------------------------ 7. the chain
LAST_SHIFT = (37, -5, 20)


def run_chain(roll):
    """tests/test_tsdf_gpu.py's chain at 1224x368, W = 8, three keyframes into 256x64x256 voxels, with colour; before each integration the volume is shifted by
    what nalo_tsdf_shift_for gives for the camera position, and once more behind the last keyframe by LAST_SHIFT. roll: 'shift' calls nalo_tsdf_shift; 'host' rolls the volume through
    nalo_tsdf_get -> the model -> nalo_tsdf_create + nalo_tsdf_set. Returns the volume's bytes after every keyframe, the shifts and the integrations' records."""
    import lifecycle_model as lm
    import lifecycle_scenes as lsc
    import plane_cases as pc
    import plane_model as pm
    from nalo_slam_amd import synth
    WW, KF, w, h, s = 8, 3, 1224, 368, 3e-4
    DIMS = (256, 64, 256)
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
    cur, vols, shifts, stats = list(fids), [], [], []
    model = None

    def roll_by(sh):
        shifts.append(tuple(int(v) for v in sh))
        if roll == "shift":
            c.tsdf_shift(sh)
        elif any(shifts[-1]):
            model["tsdf"], model["weight"] = c.tsdf_get()
            model["colour"] = c.tsdf_color_get()
            sm.shift_volume(model, sh)
            c.tsdf_create(model["origin"], model["vs"], DIMS, model["trunc"], model["max_weight"])
            c.tsdf_color_enable()
            c.tsdf_set((0, 0, 0), model["tsdf"], model["weight"])
            c.tsdf_color_set((0, 0, 0), model["colour"])

    def volume_bytes():
        return [a.tobytes() for a in c.tsdf_get()] + [c.tsdf_color_get().tobytes(), c.tsdf_geometry()["origin"].tobytes()]
    for kf in range(KF):
        if kf:
            c.ba_marginalize_frame(0)
            c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            cur = cur[1:] + [200 + WW - 1 + kf]
        c.ba_linearize(False)
        c.ba_linearize(True)
        hf, slot = WW - 3, WW - 3 + kf
        T = synth.se3_inv(win.world_to_cam[slot])
        c.dense_update_map(hf, pm.make_draws(60 + kf), T)
        if kf == 0:
            # the volume is laid around the camera: wide enough, on every axis, for the first keyframe's dense points (their 2nd .. 98th percentiles)
            xyz = c.map_dense_world_points(cur[hf], T)
            ok = np.isfinite(xyz).all(1)
            reach = np.maximum(np.abs(np.percentile(xyz[ok], 2, axis=0) - T[:, 3]), np.abs(np.percentile(xyz[ok], 98, axis=0) - T[:, 3]))
            vs = float(max(2.0 * reach / np.array(DIMS)) * 1.05)
            origin = T[:, 3] - 0.5 * vs * np.array(DIMS) + vs * np.array([7.3, -4.6, 9.2])     # off centre: the first shift_for has something to do
            dep = 1.0 / c.map_dense_get(cur[hf])["idepth"].astype(np.float64)
            dep = dep[np.isfinite(dep) & (dep > 0)]
            rng_d = (float(np.percentile(dep, 2)) * 0.5, float(np.percentile(dep, 98)) * 2.0)
            c.tsdf_create(origin, vs, DIMS, 4 * vs, 16.0)
            c.tsdf_color_enable()
            model = cm.volume(origin, vs, DIMS, 4 * vs, 16.0)
        roll_by(binding.tsdf_shift_for(c.tsdf_geometry()["desc"], T[:, 3], (0, 0, 0)))
        c.tsdf_integrate_frame(cur[hf], T, win.K, rng_d[0], rng_d[1])
        stats.append(c.tsdf_last())
        vols.append(volume_bytes())
        ff = np.zeros(WW, np.uint8)
        ff[0] = 1
        c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
    # the window's camera moves by a fraction of a voxel per keyframe: one more shift, by whole tens of voxels, rolls the volume with three keyframes fused into it
    roll_by(LAST_SHIFT)
    vols.append(volume_bytes())
    c.close()
    return vols, shifts, stats


def test_three_keyframes_of_the_device_chain_with_a_volume_that_follows_the_camera():
    a, shifts, stats = run_chain("shift")
    print("TSDF shift chain 1224x368 into 256x64x256: shifts", shifts, "stats", stats)
    assert any(shifts[0]) and shifts[3] == LAST_SHIFT and all(st["visited"] >= st["updated"] > 0 for st in stats) and sum(st["updated"] for st in stats) > 1000
    b, shifts_b, stats_b = run_chain("host")
    assert shifts_b == shifts and stats_b == stats
    for kf in range(4):
        assert a[kf] == b[kf], kf                                               # against the twin that rolls on the host, after every keyframe and the last shift
    assert a[3] != a[2]
    a2, shifts2, stats2 = run_chain("shift")
    assert a2 == a and shifts2 == shifts and stats2 == stats                    # two runs give the same bytes
