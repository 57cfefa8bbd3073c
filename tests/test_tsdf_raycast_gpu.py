"""nalo_tsdf_raycast on the device (include/nalo_gpu.h, "The ray-cast") against tests/tsdf_raycast_model.py. Every comparison is bit for bit - a NaN as a NaN
for floats, exact for bytes and counts: the definition contains only correctly rounded float operations. The model evaluates EVERY sample of every ray, the
device only a conservative interval of them: equality is what shows the interval to be conservative. The shapes are the smallest at which the kernel can go
wrong: whole 16 x 16 tiles, partial tiles both ways, one row, one pixel; the small grids of tests/test_tsdf_gpu.py, one cell, and a grid without a cell."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import tsdf_color_model as cm
import tsdf_mesh_model as mm
import tsdf_model as tm
import tsdf_raycast_model as rm
from nalo_slam_amd import binding
from test_tsdf_cpu import EYE, pose, wavy_depth
from test_tsdf_gpu import GRIDS, H0, K0, POSES, W0, bits_eq, ctx
from test_tsdf_raycast_cpu import cell, plane_volume

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4
# the views: whole tiles, partial tiles both ways, one row of nine, one pixel
VIEWS = [(64, 48, K0), (70, 33, (70.0, 68.0, 34.5, 16.0)), (9, 1, (9.0, 9.0, 4.0, 0.0)), (1, 1, (1.0, 1.0, 0.0, 0.0))]
INSIDE = pose(0.1, -0.15, 0.05, (0.1, -0.1, 1.9))                              # stands inside both grids
AWAY = pose(0.0, math.pi, 0.0, (0.0, 0.0, 0.5))                                # in front of both grids, looking away from them
K86 = (8.0, 8.0, 3.5, 2.5)                                                      # the hand cases' view: 8 x 6, rx and ry multiples of 1 / 16


def same(got, want, tag=""):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in ("n_steps", "n_hit", "n_back", "n_normal"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert mm.same_floats(got["depth"], want["depth"]), (tag, "depth", int((got["depth"] != want["depth"]).sum()))
    if "normal" in want:
        assert mm.same_floats(got["normal"], want["normal"]), (tag, "normal")
    if "rgba" in want:
        assert got["rgba"].dtype == np.uint8 and got["rgba"].shape == want["rgba"].shape and got["rgba"].tobytes() == want["rgba"].tobytes(), (tag, "rgba")


def cast_both(c, vol, w, h, K, c2w, mn, mx, st, mw, normals=False, colour=False, tag=""):
    got = c.tsdf_raycast(w, h, K, c2w, mn, mx, st, mw, normals, colour)
    want = rm.raycast(vol, w, h, K, c2w, mn, mx, st, mw, normals, colour)
    same(got, want, (tag, w, h, normals, colour))
    return got


def plant(c, vol):
    """a model volume, colour included when it has one, onto the device through nalo_tsdf_set / nalo_tsdf_color_set"""
    c.tsdf_create(vol["origin"], vol["vs"], vol["dims"], vol["trunc"], vol["max_weight"])
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    if "colour" in vol:
        c.tsdf_color_enable()
        c.tsdf_color_set((0, 0, 0), vol["colour"])
    return vol


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse(c, g, gi):
    """the three poses of tests/test_tsdf_gpu.py integrated twice with colour, on the device and in the model"""
    c.tsdf_create(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    c.tsdf_color_enable()
    vol = cm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    for rnd in range(2):
        for pi, c2w in enumerate(POSES):
            depth = wavy_depth(W0, H0, 10 * gi + pi, base=2.0 + 0.02 * rnd)
            bgr = np.random.RandomState(100 + 10 * gi + pi + rnd).randint(0, 256, (H0, W0, 3)).astype(np.uint8)
            c.tsdf_integrate_depth(dev(depth), K0, c2w, 0.5, 3.5, colour=dev(bgr))
            cm.integrate(vol, depth, bgr, K0, c2w, 0.5, 3.5)
    t, w = c.tsdf_get()
    assert bits_eq(t, vol["tsdf"]) and bits_eq(w, vol["weight"]) and mm.same_floats(c.tsdf_color_get(), vol["colour"])
    return vol


@pytest.fixture(scope="module")
def fused():
    out = []
    for gi, g in enumerate(GRIDS):
        c = ctx()
        out.append((c, fuse(c, g, gi)))
    yield out
    for c, _ in out:
        c.close()


# ------------------------------------------------------------------------------------------------ fused volumes
@pytest.mark.parametrize("gi", [0, 1])
def test_fused_volumes_from_their_poses_from_inside_and_looking_away(fused, gi):
    c, vol = fused[gi]
    hits = {}
    for pi, c2w in enumerate(POSES + [INSIDE, AWAY]):
        for vi, (w, h, K) in enumerate(VIEWS):
            if vi >= 2 and pi not in (0, 3):
                continue
            for normals, colour in ((False, False), (True, True)) + (((True, False), (False, True)) if (pi, vi) == (1, 1) else ()):
                r = cast_both(c, vol, w, h, K, c2w, 0.3, 4.0, 0.03, 1.0, normals, colour, tag=(gi, pi))
                hits[pi, vi] = r["n_hit"]
                assert r["n_steps"] == 124
                if normals:
                    assert r["n_normal"] <= r["n_hit"] and (r["n_hit"] == 0 or vi >= 2 or r["n_normal"] > 0)
    # not vacuous: every pose that looks at the grid sees surface (the thin grid, five voxels deep, holds less of it, and none that the pose inside it faces)
    assert all(hits[pi, 0] > (300, 50)[gi] and hits[pi, 1] > (200, 50)[gi] for pi in range((4, 3)[gi])), hits
    assert hits[4, 0] == 0 and hits[4, 1] == 0                                  # looking away: every pixel misses, the conservative interval is empty
    assert hits[0, 3] == 1 or hits[0, 2] > 0                                    # the one-pixel and the one-row view hit too


def test_vectorised_model_equals_the_literal_one_on_a_fused_grid(fused):
    """the yardstick itself on the device's data: 70 x 33 over the thin grid, every flag on"""
    _, vol = fused[1]
    w, h, K = VIEWS[1]
    a = rm.raycast(vol, w, h, K, POSES[0], 0.3, 4.0, 0.06, 1.0, True, True)
    px = [(int(u), int(v)) for u, v in np.random.RandomState(0).randint(0, (w, h), (300, 2))]
    b = rm.raycast_literal(vol, w, h, K, POSES[0], 0.3, 4.0, 0.06, 1.0, True, True, pixels=px)
    n = 0
    for u, v in px:
        assert mm.same_floats(a["depth"][v, u], b["depth"][v, u]) and mm.same_floats(a["normal"][v, u], b["normal"][v, u]) and (a["rgba"][v, u] == b["rgba"][v, u]).all()
        n += a["depth"][v, u] > 0
    assert n > 20


def test_skipping_is_conservative_with_most_samples_outside(fused):
    """min_depth = 0 and a max_depth sixty times the grid's far side: 4096 samples a ray, most of them outside the grid, and the model visits them all"""
    c, vol = fused[0]
    r = cast_both(c, vol, 9, 7, (9.0, 9.0, 4.0, 3.0), POSES[0], 0.0, 255.9375, 0.0625, 1.0, True, True, tag="4096 steps")
    assert r["n_steps"] == 4096 and r["n_hit"] > 10
    r = cast_both(c, vol, 9, 7, (9.0, 9.0, 4.0, 3.0), AWAY, 0.0, 255.9375, 0.0625, 1.0, tag="4096 steps, away")
    assert r["n_hit"] == 0


# ------------------------------------------------------------------------------------------------ planted volumes
def test_one_cell_and_a_grid_without_a_cell():
    c = ctx()
    vol = plant(c, cell([0.375, -0.625]))                                       # 2 x 2 x 2: one cell
    r = cast_both(c, vol, 1, 1, (8.0, 8.0, 0.0, 0.0), EYE, 0.5, 1.5, 0.0625, 1.0, True, tag="one cell, the axis ray")
    assert r["depth"][0, 0] == F(0.59375) and (r["n_hit"], r["n_normal"]) == (1, 0) and not r["normal"].any()    # q* +- 1 leaves the grid: a hit with a zero normal
    r = cast_both(c, vol, 70, 33, (70.0, 68.0, 34.5, 16.0), EYE, 0.25, 1.5, 0.03125, 1.0, True, tag="one cell")
    assert 0 < r["n_hit"] < 70 * 33
    vol = plant(c, cell([-0.5, 0.5, -0.5]))                                     # a back face in front of a front face
    r = cast_both(c, vol, 1, 1, (8.0, 8.0, 0.0, 0.0), EYE, 0.5, 1.5, 0.0625, 1.0, tag="back before front")
    assert (r["n_hit"], r["n_back"]) == (0, 1) and r["depth"][0, 0] == 0
    r = cast_both(c, vol, 64, 48, K0, EYE, 0.25, 1.5, 0.03125, 1.0, True, tag="back before front, 64 x 48")
    assert r["n_back"] > 0 and r["n_hit"] == 0
    r = cast_both(c, vol, 64, 48, K0, pose(0, 0, 0, (0, 0, 0.4)), 0.25, 1.5, 0.03125, 1.0, True, tag="the camera inside, beyond the back face")
    assert r["n_hit"] > 0
    g = tm.volume((-0.1, -0.5, 1.0), 0.2, (1, 5, 5), 0.4, 4.0)                    # 1 x 5 x 5: no cell, every pixel misses
    g["tsdf"][:] = np.where(np.arange(5)[:, None, None] < 2, 0.5, -0.5)
    g["weight"][:] = 2.0
    plant(c, g)
    for w, h, K in VIEWS:
        r = cast_both(c, g, w, h, K, EYE, 0.5, 3.0, 0.05, 1.0, True, tag="no cell")
        assert (r["n_hit"], r["n_back"]) == (0, 0) and not r["depth"].any()
    c.close()


def test_weights_on_either_side_of_min_weight_and_special_corners():
    """the plane z = 1.3125 of the hand case: the crossing lies between the z planes k = 3 (z = 1.25) and k = 4 (z = 1.5) of the grid"""
    c = ctx()
    below = np.nextafter(F(1.0), F(0.0))
    base = None
    for k in (3, 4):                                                            # a corner on either side of the crossing
        for wv in (below, F(1.0)):
            vol = plane_volume(1.3125)
            vol["weight"][k, 6, 6] = wv                                         # the voxel at x = y = 0
            plant(c, vol)
            r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 2.5, 0.125, 1.0, True, tag=("weight", k, float(wv)))
            if wv == 1.0:
                assert r["n_hit"] == 48 and (r["depth"] == F(1.3125)).all()       # exactly min_weight is valid
                base = r
            else:
                assert 0 < r["n_hit"] < 48                                       # the four pixels round the axis lose their cell, the others keep theirs
    assert base["n_normal"] == 48 and (base["normal"] == np.array([0, 0, -1], F)).all()
    for tv in (np.nan, np.inf, -np.inf, 0.0, -0.0):
        vol = plane_volume(1.3125)
        vol["tsdf"][3, 6, 6] = tv
        vol["tsdf"][4, 5, 7] = tv
        plant(c, vol)
        r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 2.5, 0.125, 1.0, True, tag=("corner", tv))
        assert 0 < r["n_hit"] <= 48 and (tv == 0 or r["n_hit"] < 48 or np.isnan(r["depth"]).any())
    # a whole plane of -0.0f and of 0.0f in front of the inside: both are outside, the crossing starts at them
    for tv in (0.0, -0.0):
        vol = plane_volume(1.3125)
        vol["tsdf"][3] = tv
        plant(c, vol)
        r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 2.5, 0.125, 1.0, True, tag=("zero plane", tv))
        assert r["n_hit"] == 48 and (r["depth"] == F(1.25)).all()
    c.close()


def test_last_pair_integer_coordinates_grid_corner_and_overflowing_rays():
    c = ctx()
    vol = plant(c, plane_volume(1.3125))
    # the crossing in the last pair (n = N - 1 = 7 at z = 1.375), and a max_depth one step short of it
    r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 1.375, 0.125, 1.0, True, tag="last pair")
    assert r["n_steps"] == 8 and r["n_hit"] == 48 and (r["depth"] == F(1.3125)).all()
    r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 1.25, 0.125, 1.0, True, tag="one step short")
    assert r["n_steps"] == 7 and r["n_hit"] == 0
    r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 0.5, 0.125, 1.0, True, tag="N = 1")
    assert r["n_steps"] == 1 and r["n_hit"] == 0
    # rays along voxel-centre planes: cx, cy on a pixel, so the middle column has x = 0 (q_x = 6) and the middle row y = 0: f = 0 on that axis
    r = cast_both(c, vol, 9, 7, (8.0, 8.0, 4.0, 3.0), EYE, 0.5, 2.5, 0.125, 1.0, True, tag="centre planes")
    assert r["n_hit"] == 63 and (r["depth"] == F(1.3125)).all()
    # a ray through the grid's corner: the camera on the line x = y = -1.5 through the centres of the corner column, q_x = q_y = 0 on the middle ray
    r = cast_both(c, vol, 9, 7, (8.0, 8.0, 4.0, 3.0), pose(0, 0, 0, (-1.5, -1.5, 0.0)), 0.5, 2.5, 0.125, 1.0, True, tag="grid corner")
    assert r["depth"][3, 4] == F(1.3125) and r["n_hit"] == 5 * 4 and not r["depth"][:3].any() and not r["depth"][:, :4].any()
    assert not r["normal"][3, 4].any() and r["n_normal"] < r["n_hit"]            # q*_x - 1 leaves the grid there
    # an fx so small that rx overflows: infinite on the outer columns, huge inside; with fy alike NaN directions (0 * inf) as well
    for K in ((1e-38, 8.0, 3.5, 2.5), (1e-38, 1e-38, 3.5, 2.5), (-1e-38, 8.0, 3.5, 2.5), (1e-45, 1e-45, 3.5, 2.5)):
        with np.errstate(all="ignore"):
            assert np.isinf((F(0.0) - F(K[2])) / F(K[0]))
        r = cast_both(c, vol, 8, 6, K, EYE, 0.5, 2.5, 0.125, 1.0, True, tag=("overflow", K))
        assert r["n_hit"] == 0 and r["n_back"] == 0
    # a rotated pose over the same overflow: every entry of R meets an infinity
    r = cast_both(c, vol, 8, 6, (1e-38, 8.0, 3.5, 2.5), POSES[1], 0.5, 2.5, 0.125, 1.0, True, tag="overflow, rotated")
    assert r["n_hit"] == 0
    c.close()


def test_normals_next_to_invalid_cells_zero_gradient_and_colour_conversion():
    c = ctx()
    # an invalid voxel two planes in front of the crossing: the march's pair (cells of k = 3, 4) is valid, S(q* - e_z) (cell of k = 2, 3) is not
    vol = plane_volume(1.3125)
    vol["weight"][2, 6, 6] = 0.0
    plant(c, vol)
    r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 2.5, 0.125, 1.0, True, tag="normal next to an invalid cell")
    assert r["n_hit"] == 48 and r["n_normal"] == 32 and not r["normal"][1:5, 2:6].any()    # the sixteen rays whose cell at q* - e_z has the voxel for a corner
    # a zero gradient: z planes alternate 0.5, -0.5 and the rays start at the plane k = 3, so S(q* + e_z) == S(q* - e_z)
    vol = plane_volume(1.3125)
    vol["tsdf"][:] = np.where(np.arange(10) % 2 == 1, 0.5, -0.5).astype(F)[:, None, None]
    plant(c, vol)
    r = cast_both(c, vol, 8, 6, K86, EYE, 1.25, 2.5, 0.125, 1.0, True, tag="zero gradient")
    assert r["n_hit"] == 48 and (r["depth"] == F(1.375)).all() and r["n_normal"] == 0 and not r["normal"].any()
    # colour outside 0 .. 255, NaN and infinite, on the voxels round the crossing
    vol = plane_volume(1.3125)
    rng = np.random.RandomState(8)
    vol["colour"][:] = rng.choice(np.array([-40.0, 0.0, 0.4999, 0.5, 100.25, 254.5, 255.0, 256.0, 1e30, np.nan, np.inf, -np.inf], F), vol["colour"].shape)
    plant(c, vol)
    r = cast_both(c, vol, 70, 33, (70.0, 68.0, 34.5, 16.0), EYE, 0.5, 2.5, 0.125, 1.0, True, True, tag="colour conversion")
    assert r["n_hit"] > 1000 and (r["rgba"][..., 3][r["depth"] > 0] == 255).all() and (r["rgba"][r["depth"] == 0] == 0).all()
    assert {0, 255} <= set(np.unique(r["rgba"][..., :3]).tolist()) and len(np.unique(r["rgba"][..., :3])) > 20
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_color_disable() or c.tsdf_raycast(8, 6, K86, EYE, 0.5, 2.5, 0.125, 1.0, colour=True)
    c.close()


# ------------------------------------------------------------------------------------------------ views, buffer reuse, the round trip
def view_arrays(c):
    c.sync()
    return {k: (None if v is None else torch.as_tensor(v, device="cuda").cpu().numpy()) for k, v in c.tsdf_raycast_view().items()}


def test_views_download_false_and_buffer_reuse(fused):
    c, vol = fused[0]
    twin = ctx()
    fuse(twin, GRIDS[0], 0)
    stream = c.L.nalo_stream(c.h_)
    big, small = VIEWS[1], (9, 5, (9.0, 9.0, 4.0, 2.0))
    for step_i, ((w, h, K), normals, colour) in enumerate(((small, True, True), (big, True, True), (small, False, False), (big, True, False), (big, False, True))):
        got = cast_both(c, vol, w, h, K, POSES[step_i % 3], 0.3, 4.0, 0.03, 1.0, normals, colour, tag=("reuse", step_i))
        v = c.tsdf_raycast_view()
        assert v["depth"].shape == (h, w) and v["depth"].stream == stream and (v["normal"] is None) == (not normals) and (v["rgba"] is None) == (not colour)
        a = view_arrays(c)
        assert mm.same_floats(a["depth"], got["depth"])
        assert not normals or (a["normal"].shape == (h, w, 3) and mm.same_floats(a["normal"], got["normal"]))
        assert not colour or (a["rgba"].shape == (h, w, 4) and a["rgba"].tobytes() == got["rgba"].tobytes())
        # the twin leaves the images on the device: the same counts, the same images through the view
        cnt = twin.tsdf_raycast(w, h, K, POSES[step_i % 3], 0.3, 4.0, 0.03, 1.0, normals, colour, download=False)
        assert set(cnt) == {"n_hit", "n_back", "n_normal", "n_steps"} and all(cnt[k] == got[k] for k in cnt)
        b = view_arrays(twin)
        assert mm.same_floats(b["depth"], a["depth"]) and all((a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()) for k in ("normal", "rgba"))
    # the descriptors are what nalo_dev_plane_check accepts
    d = binding.TsdfRaycastDev()
    assert c.L.nalo_tsdf_raycast_view(c.h_, C.byref(d)) == 0 and (d.w, d.h) == big[:2] and d.normal.ptr is None and d.rgba.ptr is not None
    assert c.L.nalo_dev_plane_check(c.h_, C.byref(d.depth)) == 0 and c.L.nalo_dev_plane_check(c.h_, C.byref(d.rgba)) == 0
    assert (d.depth.dtype, d.depth.channels, d.rgba.dtype, d.rgba.channels, d.rgba.stride_x, d.rgba.stride_c) == (binding.DT_F32, 1, binding.DT_U8, 3, 4, 1)
    twin.close()


def test_depth_view_of_one_context_integrated_into_another_behind_queued_work(fused):
    """context A's depth view goes into context B with producer_stream = nalo_stream(A). On A's stream the view is first overwritten with another depth, then
    0.2 s of matmuls run, then the ray-cast's own depth is copied back: B must wait for all of it on the device, and the call must not wait on the host"""
    a, vol = fused[0]
    w, h, K = VIEWS[1]
    want = rm.raycast(vol, w, h, K, POSES[1], 0.3, 4.0, 0.03, 1.0)
    g = GRIDS[0]
    b = ctx()
    b.tsdf_create(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    mvol = tm.volume(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    warm = wavy_depth(w, h, 77)
    b.tsdf_integrate_depth(dev(warm), K, POSES[0], 0.5, 3.5)                     # steady state: B's events exist
    tm.integrate(mvol, warm, K, POSES[0], 0.5, 3.5)
    got = a.tsdf_raycast(w, h, K, POSES[1], 0.3, 4.0, 0.03, 1.0)
    same(got, want, "round trip, the ray-cast")
    view = a.tsdf_raycast_view()["depth"]
    t = torch.as_tensor(view, device="cuda")
    assert t.data_ptr() == view.ptr and view.stream == a.L.nalo_stream(a.h_)
    right, wrong = t.clone(), t.clone() + 0.7
    m = torch.randn(4096, 4096, device="cuda")
    out = torch.empty_like(m)
    torch.cuda.synchronize()
    S = torch.cuda.ExternalStream(view.stream)
    try:
        with torch.cuda.stream(S):
            torch.mm(m, m, out=out)
            S.synchronize()
            t0 = time.perf_counter()
            torch.mm(m, m, out=out)
            S.synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
            t.copy_(wrong)
            for _ in range(min(int(math.ceil(0.25 / one)) + 1, 20000)):
                torch.mm(m, m, out=out)
            t.copy_(right)
            behind = torch.cuda.Event()
            behind.record(S)
            b.tsdf_integrate_depth(view, K, POSES[1], 0.5, 3.5)                  # stream = None: the view's own, A's main stream
            assert not behind.query(), "nalo_tsdf_integrate_depth waited for the producer stream"
        r = tm.integrate(mvol, want["depth"], K, POSES[1], 0.5, 3.5)            # the model's integration of the model's ray-cast
        assert b.tsdf_last()["updated"] == r["updated"] > 100
        tt, tw = b.tsdf_get()
        assert bits_eq(tt, mvol["tsdf"]) and bits_eq(tw, mvol["weight"])
    finally:
        S.synchronize()
        b.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ no side effects
def test_a_context_that_ray_casts_equals_a_twin_that_never_does():
    outs = []
    for casts in (True, False, True):
        c = ctx()
        fuse(c, GRIDS[1], 1)
        imgs = []
        if casts:
            for (w, h, K), c2w in ((VIEWS[0], POSES[0]), (VIEWS[1], INSIDE), (VIEWS[2], POSES[2])):
                r = c.tsdf_raycast(w, h, K, c2w, 0.3, 4.0, 0.03, 1.0, True, True)
                imgs += [r["depth"].tobytes(), r["normal"].tobytes(), r["rgba"].tobytes(), repr([r[k] for k in ("n_hit", "n_back", "n_normal", "n_steps")])]
        t, w = c.tsdf_get()
        outs.append(([t.tobytes(), w.tobytes(), c.tsdf_color_get().tobytes(), repr(c.tsdf_last())], imgs))
        c.close()
    assert outs[0][0] == outs[1][0] == outs[2][0]                               # volume, colour and nalo_tsdf_last: the ray-cast reads only
    assert outs[0][1] == outs[2][1] and len(outs[0][1]) == 12                   # two runs give the same bytes


# ------------------------------------------------------------------------------------------------ refusals
def raw_args(w=8, h=6, K=K86, c2w=EYE, mn=0.5, mx=2.5, st=0.125, mw=1.0, normals=0, colour=0, bufs=None):
    a = binding.TsdfRaycastArgs()
    a.w, a.h = w, h
    a.K[:] = K
    a.camToWorld[:] = [float(v) for v in np.asarray(c2w, np.float64).reshape(-1)]
    a.min_depth, a.max_depth, a.step, a.min_weight, a.with_normals, a.with_colour = mn, mx, st, mw, normals, colour
    a.n_hit = a.n_back = a.n_normal = a.n_steps = 77
    if bufs is not None:
        a.depth, a.normal, a.rgba = (None if b is None else b.ctypes.data_as(t) for b, t in zip(bufs, (binding.c_fp, binding.c_fp, binding.c_u8p)))
    return a


def test_refusals_leave_everything_as_it_was():
    c = ctx()
    v = binding.TsdfRaycastDev()
    assert c.L.nalo_tsdf_raycast(c.h_, C.byref(raw_args())) == ERR_STATE and c.L.nalo_tsdf_raycast_view(c.h_, C.byref(v)) == ERR_STATE       # no volume
    vol = plane_volume(1.3125)
    colour = vol.pop("colour")                                                  # a volume without colour first
    plant(c, vol)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_raycast_view()                                                   # before the first ray-cast
    a = raw_args(colour=1)
    assert c.L.nalo_tsdf_raycast(c.h_, C.byref(a)) == ERR_STATE and (a.n_hit, a.n_back, a.n_normal, a.n_steps) == (0, 0, 0, 0)                  # colour is not enabled
    assert c.L.nalo_tsdf_raycast_view(c.h_, C.byref(v)) == ERR_STATE
    vol["colour"] = colour
    vol["colour"][:] = 100.0
    plant(c, vol)
    first = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 2.5, 0.125, 1.0, True, True, tag="before the refusals")
    assert first["n_hit"] == 48
    before = (c.tsdf_get()[0].tobytes(), c.tsdf_get()[1].tobytes(), c.tsdf_color_get().tobytes())
    images = {k: a_.tobytes() for k, a_ in view_arrays(c).items()}
    nan_pose, inf_pose = np.array(EYE), np.array(EYE)
    nan_pose[1, 2], inf_pose[0, 3] = np.nan, np.inf
    bad = [dict(w=0), dict(h=0), dict(w=-3), dict(w=8193, h=8192), dict(w=1 << 30, h=1 << 30), dict(K=(np.nan, 8.0, 3.5, 2.5)), dict(K=(8.0, 8.0, np.inf, 2.5)), dict(K=(0.0, 8.0, 3.5, 2.5)),
           dict(K=(8.0, -0.0, 3.5, 2.5)), dict(c2w=nan_pose), dict(c2w=inf_pose), dict(mn=np.nan), dict(mx=np.inf), dict(st=np.nan), dict(st=np.inf), dict(mn=-0.125), dict(mn=3.0, mx=2.5),
           dict(st=0.0), dict(st=-0.125), dict(mw=np.nan), dict(st=1e-4), dict(mn=0.0, mx=4096.0, st=1.0)]
    for kw in bad:
        d, n, r = np.full((6, 8), 7.0, F), np.full((6, 8, 3), 7.0, F), np.full((6, 8, 4), 7, np.uint8)
        a = raw_args(normals=1, colour=1, bufs=(d, n, r), **kw)
        assert c.L.nalo_tsdf_raycast(c.h_, C.byref(a)) == ERR_ARG, kw
        assert (a.n_hit, a.n_back, a.n_normal, a.n_steps) == (0, 0, 0, 0) and (d == 7).all() and (n == 7).all() and (r == 7).all(), kw
    # a host normal or rgba without its flag; NULL arguments
    for flags, bufs in (((0, 1), (None, np.full((6, 8, 3), 7.0, F), None)), ((1, 0), (None, None, np.full((6, 8, 4), 7, np.uint8)))):
        a = raw_args(normals=flags[0], colour=flags[1], bufs=bufs)
        assert c.L.nalo_tsdf_raycast(c.h_, C.byref(a)) == ERR_ARG and all(b is None or (b == 7).all() for b in bufs) and a.n_steps == 0
    assert c.L.nalo_tsdf_raycast(c.h_, None) == ERR_ARG and c.L.nalo_tsdf_raycast_view(c.h_, None) == ERR_ARG
    # volume, colour and the previous device images are what they were, and the view still names them
    assert (c.tsdf_get()[0].tobytes(), c.tsdf_get()[1].tobytes(), c.tsdf_color_get().tobytes()) == before
    assert {k: a_.tobytes() for k, a_ in view_arrays(c).items()} == images
    # the next legal calls work: min_weight = +inf is legal (no voxel is valid), and so is 4096 steps
    r = cast_both(c, vol, 8, 6, K86, EYE, 0.5, 2.5, 0.125, np.inf, True, True, tag="min_weight = inf")
    assert r["n_hit"] == 0
    r = cast_both(c, vol, 8, 6, K86, EYE, 0.0, 4095.0 / 1024, 1.0 / 1024, 1.0, True, True, tag="4096 steps")
    assert r["n_steps"] == 4096 and r["n_hit"] == 48
    c.tsdf_destroy()
    assert c.L.nalo_tsdf_raycast_view(c.h_, C.byref(v)) == ERR_STATE
    c.close()


# ------------------------------------------------------------------------------------------------ the device chain
def test_three_keyframes_of_the_device_chain_with_a_ray_cast_after_each(monkeypatch):
    """tests/test_tsdf_gpu.py's chain (1224x368, W = 8, 256x64x256 voxels, three keyframes): after every integration a 306 x 92 view (K / 4) from the keyframe's
    pose against the vectorised model of the volume as it stands; after the last one the full 1224 x 368 view twice, and 2000 seeded pixels of it against
    the literal model"""
    import test_tsdf_gpu as tg
    made, seen = {}, []
    create, integrate = binding.Context.tsdf_create, binding.Context.tsdf_integrate_frame

    def create_and_note(self, origin, voxel_size, dims, trunc, max_weight):
        made["vol"] = tm.volume(origin, voxel_size, dims, trunc, max_weight)
        return create(self, origin, voxel_size, dims, trunc, max_weight)

    def integrate_and_cast(self, fid, T, K, mn, mx):
        integrate(self, fid, T, K, mn, mx)
        vol = made["vol"]
        vol["tsdf"], vol["weight"] = self.tsdf_get()
        st = (mx - mn) / 250.0
        K4 = tuple(float(k) / 4 for k in K)
        r = cast_both(self, vol, 306, 92, K4, T, mn, mx, st, 1.0, True, tag=("chain", len(seen)))
        assert r["n_steps"] <= 256
        # the dense map marks every third pixel, so after three keyframes few cells have eight observed corners and none has its six neighbours: with
        # min_weight = 0 the unobserved voxels (tsdf 1, weight 0) count as outside, and the normals have something to say
        r0 = cast_both(self, vol, 306, 92, K4, T, mn, mx, st, 0.0, True, tag=("chain, min_weight 0", len(seen)))
        seen.append((r["n_hit"], r["n_back"], r["n_normal"], r["n_steps"], r0["n_hit"], r0["n_back"], r0["n_normal"]))
        if len(seen) == 3:                                                        # once, at the full size: two runs give the same bytes; seeded pixels against the literal model
            Kf = tuple(float(k) for k in K)
            a = self.tsdf_raycast(1224, 368, Kf, T, mn, mx, st, 1.0, True)
            b = self.tsdf_raycast(1224, 368, Kf, T, mn, mx, st, 1.0, True)
            assert all(a[k].tobytes() == b[k].tobytes() for k in ("depth", "normal")) and all(a[k] == b[k] for k in ("n_hit", "n_back", "n_normal", "n_steps"))
            px = [(int(u), int(v)) for u, v in np.random.RandomState(12).randint(0, (1224, 368), (2000, 2))]
            lit = rm.raycast_literal(vol, 1224, 368, Kf, T, mn, mx, st, 1.0, True, pixels=px)
            us, vs = np.array([p[0] for p in px]), np.array([p[1] for p in px])
            assert mm.same_floats(a["depth"][vs, us], lit["depth"][vs, us]) and mm.same_floats(a["normal"][vs, us], lit["normal"][vs, us])
            made["full"] = (a["n_hit"], int((lit["depth"][vs, us] > 0).sum()))

    monkeypatch.setattr(binding.Context, "tsdf_create", create_and_note)
    monkeypatch.setattr(binding.Context, "tsdf_integrate_frame", integrate_and_cast)
    tg.run_chain(True)
    print("TSDF ray-cast, chain 1224x368 into 256x64x256, 306x92 views (hit, back, normal, N; hit, back, normal at min_weight 0) per keyframe:", seen,
          "full view (hits, literal pixels that hit):", made["full"])
    assert len(seen) == 3 and all(s[0] > 30 for s in seen) and seen[2][0] > seen[0][0] and seen[2][6] > 0 and made["full"][0] > 1000 and made["full"][1] > 10
