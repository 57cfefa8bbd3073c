"""nalo_map_render_mesh - the TSDF meshes in the viewer's 3-D panel - against the literal model of tests/render_mesh_model.py.

Every comparison is bit for bit over EVERY pixel of rgb and depth and over the eleven counts (render_mesh_model.same); tests that go beyond the planted shapes
use the vectorised model, which tests/test_map_render_mesh_cpu.py holds equal to the literal one. Viewports are 16x8, 64x32 and 70x33 (the chain: 306x92).
Triangles are planted through torch tensors as the user source; the archive and the live mesh are fed to the model from nalo_tsdf_archive_get and the downloaded
mesh.

  1  edges and classes: edges and vertices on pixel centres, shared edges in both orders and windings, slivers, one pixel, the lane / wave threshold, the whole
     viewport, every drop class with its count, 1 .. 257 triangles
  2  the depth test: triangle against triangle, point and line; equal depths; coplanar triangles
  3  colour: bytes 0 and 255, a triangle seen edge-on
  4  the three sources, alone and together; a user mesh produced on a second stream without a host wait
  5  a context that has only a volume
  6  no source selected: nalo_map_render's bytes
  7  determinism, no side effects, the key plane cleans itself
  8  refusals
  9  three keyframes of the device chain at 1224x368, followed, archived, meshed and rendered"""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import map_model as mm
import render_mesh_model as rmm
import render_model as rm
import test_map_render_gpu as tmr
import test_tsdf_archive_gpu as tag
from nalo_slam_amd import binding
from test_map_render_gpu import small                                          # noqa: F401 (the module fixture)
from test_tsdf_gpu import ctx
from test_tsdf_mesh_gpu import device_mesh, grid

pytestmark = pytest.mark.gpu

f32 = np.float32
ERR_ARG, ERR_STATE = -1, -4
EYE = np.eye(3, 4)
GREY = tmr.GREY
UNIT = dict(fx=1, fy=1, cx=0, cy=0)
TH = dict(scaledTH=tmr.BIG, absTH=tmr.BIG, minRelBS=0.0)                         # refreshPC's thresholds off, as the models' clouds are built
LANE_BOX = 64                                                                  # kMrLaneBox: not observable; the shapes below lie either side of it


def unit_cam(vw, vh, znear=0.5, zfar=100.0):
    return rm.make_cam(vw, vh, znear=znear, zfar=zfar, **UNIT)


def at(u, v, z=1.0):
    return [u * z, v * z, z]


def soup(points, colours=None):
    """triangles given as [[p0, p1, p2], ...] -> (xyz [3 n][3], tri [n][3], rgba [3 n][4]), three vertices of its own each"""
    xyz = np.asarray(points, f32).reshape(-1, 3)
    n = len(xyz) // 3
    rgba = np.full((3 * n, 4), 255, np.uint8)
    rgba[:, :3] = np.random.RandomState(n).randint(0, 256, (3 * n, 3)) if colours is None else np.repeat(np.asarray(colours, np.uint8).reshape(n, 3), 3, 0)
    return xyz, np.arange(3 * n, dtype=np.int32).reshape(n, 3), rgba


def on_device(mesh):
    xyz, tri, rgba = mesh
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    return dev(np.asarray(xyz).reshape(-1, 3), f32), dev(np.asarray(tri).reshape(-1, 3), np.int32), None if rgba is None else dev(np.asarray(rgba).reshape(-1, 4), np.uint8)


def call(c, cam, view, user=None, archive=False, live=False, mode=0, box=0, frames=(), background=GREY, stream=None, **kw):
    return c.map_render_mesh(cam["vw"], cam["vh"], view, frames, archive=archive, live=live, mesh=None if user is None else on_device(user), colour_mode=mode,
                             max_box_pixels=box, mesh_stream=stream, background=background, **dict(tmr.cam_kw(cam), **kw))


def check(c, cam, view, user=None, model_meshes=None, archive=False, live=False, mode=0, box=0, literal=True, clouds=(), segs=(), what="", **kw):
    """the device call against the model. model_meshes: what the model draws (default: the user mesh); clouds / segs: render_model's points and lines"""
    meshes = ([] if user is None else [user]) if model_meshes is None else model_meshes
    want = rmm.render(cam, GREY, view, meshes, mode, box, clouds, segs, literal)
    got = call(c, cam, view, user, archive, live, mode, box, **kw)
    bad = rmm.same(got, want)
    assert bad == [], (what, bad, {k: (got[k], want[k]) for k in bad if k.startswith("n_")}, int((got["rgb"] != want["rgb"]).any(2).sum()))
    return got


@pytest.fixture(scope="module")
def vc():
    """a context with nothing but a volume: no window, no frames"""
    c = ctx()
    c.tsdf_create((-1.0, -1.0, 0.5), 0.25, (8, 8, 8), 0.5, 4.0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1: edges and classes
def test_edges_and_vertices_on_pixel_centres(vc):
    cam = unit_cam(16, 8)
    a, b, cc, d = at(2.5, 1.5, 1.0), at(6.5, 1.5, 2.0), at(6.5, 5.5, 1.5), at(2.5, 5.5, 3.0)
    up, low = (200, 10, 10), (10, 200, 10)                                       # the triangle above the diagonal a-cc and the one below it
    # two triangles that share the diagonal through four centres, in both submission orders and both windings
    pics = []
    for (t0, c0), (t1, c1) in ((((a, b, cc), up), ((a, cc, d), low)), (((a, cc, d), low), ((a, b, cc), up)), (((a, cc, b), up), ((a, d, cc), low)), (((cc, a, b), up), ((d, a, cc), low))):
        g = check(vc, cam, EYE, soup([t0, t1], [c0, c1]), what="shared edge")
        assert g["n_tri_pixels"] == 16 and np.isfinite(g["depth"][1:5, 2:6]).all() and np.isfinite(g["depth"]).sum() == 16     # every pixel once: left and top edges in
        pics.append(g)
    assert all(rmm.same(p, pics[0]) == [] for p in pics[1:])
    # slivers that cover no centre, drawn with an empty box and drawn with a box that holds centres none of which is inside
    g = check(vc, cam, EYE, soup([[at(2.6, 1.6), at(3.4, 1.7), at(2.7, 2.4)], [at(1.6, 1.4), at(9.4, 4.4), at(9.4, 4.45)]]), what="slivers")
    assert g["n_triangles"] == 2 and g["n_tri_pixels"] == 0 and np.isinf(g["depth"]).all()
    # a triangle of one pixel: its vertex is the centre of (0, 0); the centres on its other two corners belong to edges that are not top-left... the hypotenuse
    g = check(vc, cam, EYE, soup([[at(0.5, 0.5), at(1.5, 0.5), at(0.5, 1.5)]]), what="one pixel")
    assert g["n_tri_pixels"] == 1 and np.isfinite(g["depth"][0, 0])
    # vertices and edges on the viewport's borders and outside it
    check(vc, cam, EYE, soup([[at(-3.5, -2.5), at(15.5, 0.5), at(0.5, 7.5)], [at(15.5, 7.5), at(20.5, 7.5), at(15.5, 12.5)]]), what="borders")


@pytest.mark.parametrize("size", [(16, 8), (64, 32), (70, 33)])
def test_boxes_either_side_of_the_threshold_and_the_whole_viewport(vc, size):
    cam = unit_cam(*size)
    vw, vh = size
    tris, boxes = [], []
    for k, (bw, bh) in enumerate(((8, 8), (9, 7), (13, 5), (16, 4), (5, 13), (2, 2), (65, 1), (1, 8))):
        bw, bh = min(bw, vw), min(bh, vh)
        x, y = (3 * k) % max(vw - bw, 1) + 0.5, (5 * k) % max(vh - bh, 1) + 0.5
        tris.append([at(x, y, 1.0 + 0.25 * k), at(x + bw - 1, y + 0.25, 1.5), at(x + 0.25, y + bh - 1, 2.0 + 0.125 * k)])
        boxes.append(bw * bh)
    assert {LANE_BOX - 1, LANE_BOX, LANE_BOX + 1, 4} <= set(boxes)
    mesh = soup(tris)
    for mode in (0, 1):
        g = check(vc, cam, EYE, mesh, mode=mode, what="threshold %s mode %d" % (size, mode))
        assert g["n_tri_large"] == 0 and g["n_tri_pixels"] > 20
    # one triangle over the whole viewport with max_box_pixels = vw * vh, and refused as large with one less
    whole = soup([[at(-1.0, -1.0, 1.0), at(2.0 * vw + 2, -1.0, 2.0), at(-1.0, 2.0 * vh + 2, 4.0)]], [(250, 130, 20)])
    g = check(vc, cam, EYE, whole, box=vw * vh, what="whole viewport")
    assert g["n_tri_pixels"] == vw * vh and np.isfinite(g["depth"]).all()
    g = check(vc, cam, EYE, whole, box=vw * vh - 1, what="one pixel too large")
    assert g["n_tri_large"] == 1 and g["n_tri_pixels"] == 0


def test_every_drop_class_with_its_count(vc):
    cam = unit_cam(16, 8, znear=0.5, zfar=1.6)
    good = [at(0.5, 0.5, 1.0), at(4.5, 0.5, 2.0), at(0.5, 4.5, 4.0)]             # tests/test_map_render_mesh_cpu.py's hand-worked triangle: depth 1.6 == zfar at pixel (0, 2)
    tris = [good,
            [at(8.5, 1.5, 0.5), at(12.5, 1.5, 1.0), at(8.5, 5.5, 1.0)],          # zv exactly znear
            [[np.nan, 1.0, 1.0], at(12.5, 1.5), at(8.5, 5.5)],                   # one vertex NaN
            [at(8.5, 1.5), [1.0, np.inf, 1.0], at(8.5, 5.5)],
            [at(8.5, 1.5), at(131072.0, 1.5), at(8.5, 5.5)],                     # guard, exactly on it
            [at(8.5, 1.5), at(12.5, 1.5), at(8.5, -131072.0)],
            [at(8.5, 1.5), at(8.5, 1.5), at(8.5, 5.5)],                          # zero area
            [at(8.5, 1.5), at(10.5, 2.5), at(12.5, 3.5)],
            [at(8.5, 0.5), at(14.5, 0.5), at(8.5, 6.5)]]                         # a box of 49 pixels against max_box_pixels = 30
    xyz, tri, rgba = soup(tris)
    tri = np.concatenate([tri, [[0, 1, -1], [0, 27, 1], [27, 28, 29], [-2147483648, 0, 1], [0, 1, 2147483647]]]).astype(np.int32)      # nv = 27
    g = check(vc, cam, EYE, (xyz, tri, rgba), box=30, what="classes")
    assert [g[k] for k in rmm.COUNTS] == [14, 5, 3, 2, 2, 1, g["n_tri_pixels"]] and 0 < g["n_tri_pixels"] < 10
    assert np.isinf(g["depth"][2, 0]) and g["depth"][0, 2] == f32(4.0 / 3.0)     # depth exactly zfar at a pixel is no candidate
    g = check(vc, cam, EYE, (xyz, tri, rgba), box=49, mode=1, what="classes, box 49")
    assert g["n_tri_large"] == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves_and_workgroups(vc, n):
    view = rm.look_at((0.3, -0.4, -2.0), (0, 0, 3.0), (0, -1, 0))
    cam = rm.make_cam(70, 33, fx=37.5, fy=31.25, znear=0.7, zfar=5.0)
    mesh = rmm.seeded_mesh(100 + n, n, cam, view, size=4.0)
    for mode in (0, 1):
        g = check(vc, cam, view, mesh, mode=mode, box=200, literal=n <= 65, what="%d triangles mode %d" % (n, mode))
        assert g["n_triangles"] == n
    if n == 257:
        assert all(g[k] > 0 for k in rmm.COUNTS), {k: g[k] for k in rmm.COUNTS}


# ------------------------------------------------------------------------------------------------ 2: the depth test
def test_depth_test_between_triangles_points_and_lines():
    cam = rm.make_cam(64, 32, fx=32, fy=32, cx=16, cy=8, znear=0.1, zfar=1000)  # undoes test_map_render_gpu's PK: a depth-2 point at (u, v) has its vertices on u + dx, v + dy
    c, S = tmr.planted([10.0, 30.0], [10.0, 10.0], [0.5, 0.5], color=np.array([[200] * 8, [50] * 8], f32))
    recs = mm.set_from_kf(None, tmr.active_records(c, S, 0))
    ci, _ = tmr.calib(c)
    cloud = (rm.transform(EYE, EYE),) + rm.sparse_vertices(recs, ci, 1, tmr.BIG, tmr.BIG, 0.0)
    frames = [(10, EYE)]
    pts = dict(frames=frames, display_mode=1, **TH)
    P = lambda u, v, z: [(u - 16) / 32 * z, (v - 8) / 32 * z, z]
    # a triangle at the points' depth 2 over both points: where the colours tie in depth the smaller colour word wins, whichever kind it belongs to
    flat = [[P(4.5, 4.5, 2.0), P(40.5, 4.5, 2.0), P(4.5, 40.5, 2.0)]]
    g = check(c, cam, EYE, soup(flat, [(100, 100, 100)]), clouds=[cloud], what="equal depth against points", **pts)
    assert g["depth"][10, 10] == 2 and tuple(g["rgb"][10, 10]) == (100, 100, 100) and tuple(g["rgb"][10, 30]) == (50, 50, 50) and g["n_drawn_points"] == 16
    # in front of and behind the points
    for z, wins in ((1.0, True), (4.0, False)):
        g = check(c, cam, EYE, soup([[P(4.5, 4.5, z), P(40.5, 4.5, z), P(4.5, 40.5, z)]], [(250, 250, 250)]), clouds=[cloud], what="z %g" % z, **pts)
        assert (tuple(g["rgb"][10, 10]) == (250, 250, 250)) == wins
    # against a line at equal depth: the strip is green (0, 255, 0), width 3; a darker and a brighter triangle
    poses = np.array([P(2.5, 20.5, 2.0), P(50.5, 20.5, 2.0)], f32)
    seg = rm.segments(EYE, [], np.ones(4, f32), 1, 1, all_poses=poses)
    for col, wins in (((0, 200, 0), True), ((0, 255, 1), False)):
        g = check(c, cam, EYE, soup([[P(4.5, 14.5, 2.0), P(40.5, 14.5, 2.0), P(4.5, 50.5, 2.0)]], [col]), segs=seg, all_poses=poses, display_mode=3, what="line %s" % (col,))
        tie = g["depth"][20, 5:20] == 2                                          # the strip's samples whose interpolated depth is exactly the triangle's
        assert tie.any() and ((g["rgb"][20, 5:20][tie] == col).all() if wins else (g["rgb"][20, 5:20][tie] == (0, 255, 0)).all()) and g["n_line_samples"] > 10
    # triangle against triangle: two that cross (each is nearer somewhere), in both orders; two coplanar ones with different colours
    t0, t1 = [P(4.5, 4.5, 1.0), P(44.5, 4.5, 3.0), P(4.5, 28.5, 1.0)], [P(4.5, 4.5, 3.0), P(44.5, 4.5, 1.0), P(4.5, 28.5, 3.0)]
    ga = check(c, cam, EYE, soup([t0, t1], [(255, 0, 0), (0, 0, 255)]), display_mode=3, what="crossing")
    gb = check(c, cam, EYE, soup([t1, t0], [(0, 0, 255), (255, 0, 0)]), display_mode=3, what="crossing, other order")
    assert rmm.same({**ga}, {**gb}) == [] and tuple(ga["rgb"][6, 6]) == (255, 0, 0) and tuple(ga["rgb"][6, 36]) == (0, 0, 255)
    g = check(c, cam, EYE, soup([flat[0], flat[0]], [(9, 200, 30), (9, 100, 250)]), display_mode=3, what="coplanar")
    assert tuple(g["rgb"][10, 10]) == (9, 100, 250) and g["n_tri_pixels"] == 2 * int(np.isfinite(g["depth"]).sum())
    c.close()


# ------------------------------------------------------------------------------------------------ 3: colour
def test_colour_bytes_and_a_triangle_seen_edge_on(vc):
    cam = unit_cam(16, 8)
    xyz, tri, rgba = soup([[at(0.5, 0.5, 1.0), at(12.5, 0.5, 2.0), at(0.5, 6.5, 4.0)], [at(15.5, 7.5, 1.0), at(3.5, 7.5, 1.0), at(15.5, 1.5, 1.0)]])
    rgba[:3, :3] = [[0, 255, 0], [255, 0, 255], [0, 0, 255]]
    rgba[3:, :3] = [[255, 255, 255], [255, 255, 255], [0, 0, 0]]
    rgba[:, 3] = [0, 255, 7, 1, 2, 3]                                           # alpha is ignored
    g = check(vc, cam, EYE, (xyz, tri, rgba), what="bytes 0 and 255")
    assert tuple(g["rgb"][0, 0]) == (0, 255, 0) and g["rgb"].max() == 255 and g["rgb"][np.isfinite(g["depth"])].min() == 0
    other = (xyz, tri, np.concatenate([rgba[:, :3], 255 - rgba[:, 3:]], 1))
    assert rmm.same(call(vc, cam, EYE, other), g) == []
    # colour_mode 1: the plane x = 1 holds the view direction of none of its points but its normal has nz = 0: grey 64; a fronto-parallel one: 255
    cam2 = rm.make_cam(16, 8, fx=8, fy=8, cx=2, cy=2, znear=0.5, zfar=100)
    edge_on = soup([[[1.0, 0.0, 1.0], [1.0, 0.0, 2.0], [1.0, 1.0, 1.5]], [[-0.2, 0.1, 3.0], [0.3, 0.1, 3.0], [-0.2, 0.6, 3.0]]])
    g = check(vc, cam2, EYE, (edge_on[0], edge_on[1], None), mode=1, what="edge-on")
    assert {tuple(px) for px in g["rgb"][np.isfinite(g["depth"])]} == {(64, 64, 64), (255, 255, 255)}


# ------------------------------------------------------------------------------------------------ 4: the three sources
def mesh_view(dims):
    g = grid(dims)
    lo, ext = np.array(g["origin"]), np.array(dims) * g["vs"]
    mid = lo + 0.5 * ext
    return g, rm.look_at((mid[0] + 0.1, mid[1] - 0.2, lo[2] - 1.6), mid, (0, -1, 0))


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("dims,size", [((5, 3, 2), (16, 8)), ((33, 17, 5), (70, 33))])
def test_archive_live_mesh_and_user_together(dims, size, colour):
    g, view = mesh_view(dims)
    f = 0.8 * size[0] * (1.6 + 0.5 * dims[2] * g["vs"]) / (dims[0] * g["vs"])   # the grid's width over four fifths of the picture
    cam = rm.make_cam(*size, fx=f, fy=f, znear=0.3, zfar=50)
    c = ctx()
    tag.planted(c, g, colour, 29)
    A, B = tag.cut(dims, 0, dims[0] // 2) if dims[0] > 5 else (None, (None, None))       # the small grid whole in both: the same triangles twice, equal depths everywhere
    c.tsdf_archive_mesh(1.0, A)
    arch = c.tsdf_archive_get()
    live = c.tsdf_mesh(1.0, B[0], B[1], colour=colour)
    arch_m = (arch[0], arch[1], arch[2] if colour else None)
    live_m = (live[0], live[1], live[2] if colour else None)
    user = rmm.seeded_mesh(7, 40, cam, view, size=3.0)
    literal = dims == (5, 3, 2)
    modes = (0, 1) if colour else (1,)
    for mode in modes:
        ga = check(c, cam, view, None, [arch_m], archive=True, mode=mode, literal=literal, what="archive %s" % (dims,))
        gl = check(c, cam, view, None, [live_m], live=True, mode=mode, literal=literal, what="live %s" % (dims,))
        gu = check(c, cam, view, user, mode=mode, literal=literal, what="user")
        gall = check(c, cam, view, user, [arch_m, live_m, user], archive=True, live=True, mode=mode, literal=literal, what="all three")
        assert ga["n_triangles"] == len(arch[1]) > 0 and gl["n_triangles"] == len(live[1]) > 0 and gu["n_triangles"] == 40
        assert all(gall[k] == ga[k] + gl[k] + gu[k] for k in rmm.COUNTS)         # each source's share: the counts are sums
        assert ga["n_tri_pixels"] > 0 and gl["n_tri_pixels"] > 0
    if not colour:                                                               # colour_mode 0 needs colours in every selected source; the user mesh alone has them
        for kw in (dict(archive=True), dict(live=True)):
            with pytest.raises(binding.NaloError):
                call(c, cam, view, user, mode=0, **kw)
        check(c, cam, view, user, mode=0, literal=literal, what="user colours beside uncoloured meshes that are not selected")
    c.close()


def test_a_user_mesh_produced_on_a_second_stream_without_a_host_wait(vc):
    cam = unit_cam(64, 32)
    mesh = rmm.seeded_mesh(3, 300, cam, EYE, size=5.0, odd=False)
    want = rmm.render(cam, GREY, EYE, [mesh], 0, 0, literal=False)
    good = on_device(mesh)
    xyz = torch.full_like(good[0], float("nan"))                                 # what a call that does not wait would read: every triangle `near`
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
            for _ in range(min(int(math.ceil(0.2 / one)) + 1, 20000)):
                torch.mm(a, a, out=out)
            xyz.copy_(good[0], non_blocking=True)
            behind = torch.cuda.Event()
            behind.record(S)
        queued = not behind.query()
        got = vc.map_render_mesh(64, 32, EYE, mesh=(xyz, good[1], good[2]), mesh_stream=S.cuda_stream, background=GREY, **tmr.cam_kw(cam))
        assert queued, "the producer had finished before the call was made: the test shows nothing"
        assert behind.query()                                                    # the call ends with its host wait, behind the producer: the arrays are the caller's again
        assert rmm.same(got, want) == [] and got["n_tri_near"] == 0 and got["n_tri_pixels"] > 1000
    finally:
        S.synchronize()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5: a context that has only a volume
def test_a_volume_only_context_draws_its_mesh_and_the_trajectory():
    g, view = mesh_view((33, 17, 5))
    cam = rm.make_cam(70, 33, fx=30, fy=30, znear=0.3, zfar=50)
    c = ctx()
    tag.planted(c, g, True, 31, archive=False)
    live = c.tsdf_mesh(1.0, colour=True)
    poses = (np.array(g["origin"], f32) + np.cumsum(np.random.RandomState(2).rand(12, 3) * 0.3, 0)).astype(f32)
    segs = rm.segments(view, [], np.ones(4, f32), 1, 1, all_poses=poses)
    got = check(c, cam, view, None, [live], live=True, literal=False, segs=segs, all_poses=poses, what="volume only")
    assert got["n_tri_pixels"] > 100 and got["n_segments"] == 11 and got["n_line_samples"] > 10
    a, keep = c.map_render_args(70, 33, view, [(1, EYE)], **tmr.cam_kw(cam))
    m = binding.MapRenderMeshArgs()
    m.with_live_mesh = 1
    rgb, depth = np.full((33, 70, 3), 0xA5, np.uint8), np.full((33, 70), -7.0, f32)
    a.rgb, a.depth = binding._u8(rgb), binding._f(depth)
    for patch in (dict(), dict(n_frames=0, show_kf_cams=1), dict(n_frames=0, show_current_cam=1)):
        for k, v in dict(dict(n_frames=1, show_kf_cams=0, show_current_cam=0), **patch).items():
            setattr(a, k, v)
        m.n_triangles = m.n_tri_pixels = 77
        assert c.L.nalo_map_render_mesh(c.h_, C.byref(a), C.byref(m)) == ERR_STATE, patch     # a frame is listed, or a camera is drawn: that needs the window
        assert (rgb == 0xA5).all() and (depth == -7.0).all() and m.n_triangles == 0 and m.n_tri_pixels == 0
    assert c.L.nalo_map_render(c.h_, C.byref(a)) == ERR_STATE                    # nalo_map_render itself still needs a window, whatever it draws
    a.show_current_cam = 0
    assert c.L.nalo_map_render(c.h_, C.byref(a)) == ERR_STATE and (rgb == 0xA5).all()
    assert rmm.same(call(c, cam, view, live=True, all_poses=poses), got) == []
    c.close()


# ------------------------------------------------------------------------------------------------ 6: no source selected
def test_no_source_selected_is_map_render_bit_for_bit(small):
    A, frames, view, cam = small["A"], small["frames"], small["view"], small["cam"]
    kw = dict(display_mode=1, background=GREY, show_kf_cams=True, show_trajectory=True, **TH, **tmr.cam_kw(cam))
    want = A.map_render(cam["vw"], cam["vh"], view, frames, **kw)
    got = A.map_render_mesh(cam["vw"], cam["vh"], view, frames, **kw)
    assert want["n_drawn_points"] > 500 and rm.same(got, want) == [] and got["rgb"].tobytes() == want["rgb"].tobytes() and got["depth"].tobytes() == want["depth"].tobytes()
    assert all(got[k] == 0 for k in rmm.COUNTS)
    empty = (np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), np.zeros((0, 4), np.uint8))
    got = A.map_render_mesh(cam["vw"], cam["vh"], view, frames, mesh=on_device(empty), **kw)       # a user source without a triangle
    assert rm.same(got, want) == [] and all(got[k] == 0 for k in rmm.COUNTS)
    # and a mesh in front of the cloud: points, lines and triangles in one depth test, against the model's points and lines
    recs = small["recs"]
    ci, cf = tmr.calib(A)
    clouds = [(rm.transform(view, m),) + rm.sparse_vertices(recs[f], ci, 1, tmr.BIG, tmr.BIG, 0.0) for f, m in frames]
    segs = rm.segments(view, frames, cf, A.w, A.h, show_kf_cams=True, show_trajectory=True)
    user = rmm.seeded_mesh(5, 120, cam, view, size=9.0)
    g = check(A, cam, view, user, literal=False, clouds=clouds, segs=segs, frames=frames, display_mode=1, show_kf_cams=True, show_trajectory=True, what="cloud and mesh", **TH)
    assert g["n_drawn_points"] == want["n_drawn_points"] and g["n_tri_pixels"] > 500 and not np.array_equal(g["rgb"], want["rgb"])


# ------------------------------------------------------------------------------------------------ 7: determinism and side effects
def test_two_runs_a_twin_that_never_renders_and_the_key_plane():
    g, view = mesh_view((33, 17, 5))
    cam = rm.make_cam(70, 33, fx=30, fy=30, znear=0.3, zfar=50)
    A2, B2 = tag.cut((33, 17, 5), 0, 16)

    def make():
        c, S = tmr.planted([10.0, 30.0], [10.0, 10.0], [0.5, 0.25])
        tag.planted(c, g, True, 37)
        c.tsdf_archive_mesh(1.0, A2)
        c.tsdf_mesh(1.0, B2[0], B2[1], download=False, colour=True)
        return c

    a, b = make(), make()
    user = rmm.seeded_mesh(9, 100, cam, view, size=6.0)
    frames = [(10, EYE), (11, EYE)]
    runs = [call(a, cam, view, user, archive=True, live=True, mode=mode, frames=frames, show_kf_cams=True) for mode in (0, 1, 0, 1)]
    assert rmm.same(runs[0], runs[2]) == [] and rmm.same(runs[1], runs[3]) == [] and runs[0]["rgb"].tobytes() == runs[2]["rgb"].tobytes()
    assert runs[0]["depth"].tobytes() == runs[2]["depth"].tobytes() and runs[0]["n_tri_pixels"] > 100 and runs[0]["rgb"].tobytes() != runs[1]["rgb"].tobytes()
    # the twin never rendered: volume, archive, device mesh and window are bit-identical
    assert all(x.tobytes() == y.tobytes() for x, y in zip(tuple(a.tsdf_get()) + (a.tsdf_color_get(),), tuple(b.tsdf_get()) + (b.tsdf_color_get(),)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.tsdf_archive_get(keys=True), b.tsdf_archive_get(keys=True)))
    assert [m[1:] for m in device_mesh(a, True)] == [m[1:] for m in device_mesh(b, True)]
    pa, pb = a.ba_get_points(), b.ba_get_points()
    assert all(mm.bits_equal(pa[q], pb[q]) for q in pa)
    # the key plane cleans itself behind a mesh call: the next picture without a source is the background, at this size and at a larger one
    for vw, vh in ((70, 33), (64, 32), (200, 90)):
        e = a.map_render(vw, vh, view, [], background=GREY)
        assert (e["rgb"] == np.array(GREY, np.uint8)).all() and np.isinf(e["depth"]).all()
        call(a, rm.make_cam(vw, vh, fx=30, fy=30, znear=0.3, zfar=50), view, user, archive=True, live=True)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_leave_outputs_and_context_alone_and_the_next_call_is_correct():
    g, view = mesh_view((5, 3, 2))
    cam = rm.make_cam(16, 8, fx=12, fy=12, znear=0.3, zfar=50)
    c = ctx()
    user = rmm.seeded_mesh(4, 30, cam, view, size=3.0)
    dev = on_device(user)
    want = rmm.render(cam, GREY, view, [user], 0, 0, literal=True)

    def refused(code, what, patch_a=None, patch_m=None, src=dev, src_patch=None, **mkw):
        a, keep = c.map_render_args(16, 8, view, [], background=GREY, **tmr.cam_kw(cam))
        rgb, depth = np.full((8, 16, 3), 0xA5, np.uint8), np.full((8, 16), -7.0, f32)
        a.rgb, a.depth = binding._u8(rgb), binding._f(depth)
        a.n_vertices = a.n_segments = 5
        m = binding.MapRenderMeshArgs()
        for k in binding.MESH_COUNTS:
            setattr(m, k, 9)
        s = None
        if src is not None:
            s, keep2 = c.render_mesh_src(src)
            for k, v in (src_patch or {}).items():
                setattr(s, k, v)
            m.user = C.pointer(s)
        for k, v in mkw.items():
            setattr(m, k, v)
        for k, v in (patch_a or {}).items():
            setattr(a, k, v)
        assert c.L.nalo_map_render_mesh(c.h_, C.byref(a), C.byref(m) if patch_m != "null" else None) == code, what
        assert (rgb == 0xA5).all() and (depth == -7.0).all(), what
        assert all(getattr(m, k) == (9 if patch_m == "null" else 0) for k in binding.MESH_COUNTS) and a.n_vertices == 0 and a.n_segments == 0, what
        assert rmm.same(call(c, cam, view, user), want) == [], what               # the next legal call paints the right picture

    refused(ERR_ARG, "NULL m", patch_m="null")
    refused(ERR_ARG, "vw above 65536", patch_a=dict(vw=65537, vh=1))
    refused(ERR_ARG, "vh above 65536", patch_a=dict(vw=1, vh=65537))
    refused(ERR_ARG, "colour_mode 2", colour_mode=2)
    refused(ERR_ARG, "colour_mode -1", colour_mode=-1)
    refused(ERR_ARG, "negative max_box_pixels", max_box_pixels=-1)
    refused(ERR_ARG, "negative n_vertices", src_patch=dict(n_vertices=-1))
    refused(ERR_ARG, "negative n_triangles", src_patch=dict(n_triangles=-1))
    refused(ERR_ARG, "n_triangles 2^31", src_patch=dict(n_triangles=1 << 31))
    refused(ERR_ARG, "n_vertices 2^31", src_patch=dict(n_vertices=1 << 31))
    refused(ERR_ARG, "xyz NULL", src_patch=dict(xyz=None))
    refused(ERR_ARG, "tri NULL", src_patch=dict(tri=None))
    refused(ERR_ARG, "znear 0 (a refusal of nalo_map_render)", patch_a=dict(znear=0.0))
    refused(ERR_ARG, "rgb NULL", patch_a=dict(rgb=None))
    refused(ERR_STATE, "user rgba NULL in colour_mode 0", src_patch=dict(rgba=None))
    refused(ERR_STATE, "archive not enabled", with_archive=1)
    refused(ERR_STATE, "live mesh without a volume", with_live_mesh=1)
    vol_g = grid((5, 3, 2))
    tag.planted(c, vol_g, False, 3, archive=True)                                # an uncoloured volume and archive
    refused(ERR_STATE, "live mesh before any mesh call", with_live_mesh=1, colour_mode=1)
    c.tsdf_archive_mesh(1.0)
    before = [x.tobytes() for x in c.tsdf_archive_get(keys=True)] + [m_[1:] for m_ in device_mesh(c)]
    refused(ERR_STATE, "uncoloured archive in colour_mode 0", with_archive=1)
    refused(ERR_STATE, "a live mesh left by the plain nalo_tsdf_mesh in colour_mode 0", with_live_mesh=1)
    refused(ERR_ARG, "colour_mode 2 with every source selected", with_archive=1, with_live_mesh=1, colour_mode=2)
    assert [x.tobytes() for x in c.tsdf_archive_get(keys=True)] + [m_[1:] for m_ in device_mesh(c)] == before      # archive and device mesh as they were
    g1 = call(c, cam, view, user, archive=True, live=True, mode=1)               # both are legal in colour_mode 1
    assert g1["n_triangles"] == 30 + 2 * c.tsdf_archive_stats()["n_triangles"] > 30
    c.close()


# ------------------------------------------------------------------------------------------------ 9: the device chain
def chain_keyframes():
    """tests/test_tsdf_archive_gpu.py's chain (1224x368, W = 8, three keyframes fused into a coloured 256x64x256 volume that follows the camera, the leaving boxes
    archived) as the viewer loop of INTEGRATION.md: a generator that yields (keyframe, context, view, listed frames) after each keyframe, with the grid's coloured
    mesh built on the device; the context is closed when the generator is. scripts/diag/map_render_mesh_time.py measures on its last state"""
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
    c2w = {200 + i: synth.se3_inv(win.world_to_cam[i]) for i in range(nF)}
    cur, seen = list(fids), list(fids)
    for kf in range(KF):
        if kf:
            c.ba_marginalize_frame(0)
            c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            cur = cur[1:] + [200 + WW - 1 + kf]
            seen.append(cur[-1])
        c.ba_linearize(False)
        c.ba_linearize(True)
        hf, slot = WW - 3, WW - 3 + kf
        T = synth.se3_inv(win.world_to_cam[slot])
        c.dense_update_map(hf, pm.make_draws(60 + kf), T)
        if kf == 0:
            xyz = c.map_dense_world_points(cur[hf], T)
            ok = np.isfinite(xyz).all(1)
            reach = np.maximum(np.abs(np.percentile(xyz[ok], 2, axis=0) - T[:, 3]), np.abs(np.percentile(xyz[ok], 98, axis=0) - T[:, 3]))
            vs = float(max(2.0 * reach / np.array(DIMS)) * 1.05)
            origin = T[:, 3] - 0.5 * vs * np.array(DIMS) + vs * np.array([7.3, -4.6, 9.2])
            dep = 1.0 / c.map_dense_get(cur[hf])["idepth"].astype(np.float64)
            dep = dep[np.isfinite(dep) & (dep > 0)]
            rng_d = (float(np.percentile(dep, 2)) * 0.5, float(np.percentile(dep, 98)) * 2.0)
            c.tsdf_create(origin, vs, DIMS, 4 * vs, 16.0)
            c.tsdf_color_enable()
            c.tsdf_archive_enable()
        # the viewer loop of INTEGRATION.md: follow, integrate, mesh the grid, render. The chain's camera moves less than a voxel, so the second and third
        # keyframes follow a planted centre whose seams cut the fused surface (test_tsdf_archive_gpu.planted_shift): boxes with triangles leave for the archive
        centre = T[:, 3]
        if kf:
            geo, sh = c.tsdf_geometry(), tag.planted_shift(c, DIMS)
            centre = [float(np.float64(geo["origin"][a]) + (DIMS[a] // 2 + sh[a] + 0.5) * np.float64(geo["voxel_size"])) for a in range(3)]
        c.tsdf_follow(centre, (0, 0, 0), 1.0)
        c.tsdf_integrate_frame(cur[hf], T, win.K, rng_d[0], rng_d[1])
        ff = np.zeros(WW, np.uint8)
        ff[0] = 1
        c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
        c.tsdf_mesh(1.0, download=False, colour=True)
        if kf == 0:                                                              # a view from above and behind that holds the first camera and the fused surface
            sp = c.tsdf_surface_points(1.0).astype(np.float64)
            sp = sp[np.isfinite(sp).all(1)]
            lo, hi = np.percentile(sp, 5, axis=0), np.percentile(sp, 95, axis=0)
            target = 0.5 * (0.5 * (lo + hi) + T[:, 3])
            dist = 0.6 * (np.linalg.norm(0.5 * (lo + hi) - T[:, 3]) + np.max(hi - lo))
            view = rm.look_at(target + dist * np.array([0.25, -0.8, -0.55]), target, (0, -1, 0))
        # the listed frames: everything seen so far, the corridor's poses (3e-4 apart) spread out so that cameras and trajectory are more than a pixel
        frames = [(f, np.concatenate([c2w[f][:, :3], c2w[f][:, 3:] + (c2w[f][:, 3:] - c2w[200][:, 3:]) * 1999], 1)) for f in seen]
        try:
            yield kf, c, view, frames
        except GeneratorExit:
            c.close()
            raise
    c.close()


def test_three_keyframes_of_the_device_chain_rendered_after_each():
    """after each keyframe of the chain archive, live mesh, points, cameras and trajectory are rendered into a 306x92 view: against the vectorised model fed from
    nalo_tsdf_archive_get and the downloaded mesh, and against a second run. The points are the dense archive's (display_mode 3 draws no sparse record), which
    nalo_map_dense_get names frame by frame"""
    cam = rm.make_cam(306, 92, fx=110, fy=110)
    tri_total = 0
    for kf, c, view, frames in chain_keyframes():
        live = tuple(torch.as_tensor(v, device="cuda").cpu().numpy() for v in c.tsdf_mesh_view() + (c.tsdf_mesh_color_view(),))       # the downloaded mesh
        arch = c.tsdf_archive_get()
        ci, cf = tmr.calib(c)
        clouds = []
        for f, m in frames:
            try:
                clouds.append((rm.transform(view, m),) + rm.dense_vertices(c.map_dense_get(f), ci))
            except binding.NaloError:
                pass
        assert len(clouds) == kf + 1
        segs = rm.segments(view, frames, cf, c.w, c.h, show_kf_cams=True, show_trajectory=True)
        kw = dict(frames=frames, display_mode=3, with_dense=True, show_kf_cams=True, show_trajectory=True)
        got = check(c, cam, view, None, [arch[:3], live], archive=True, live=True, literal=False, clouds=clouds, segs=segs, what="chain keyframe %d" % kf, **kw)
        print("RENDER MESH chain keyframe %d: archive %d + live %d triangles, %d pixels, near %d guard %d degenerate %d large %d; %d points drawn" %
              (kf, len(arch[1]), len(live[1]), got["n_tri_pixels"], got["n_tri_near"], got["n_tri_guard"], got["n_tri_degenerate"], got["n_tri_large"], got["n_drawn_points"]))
        assert got["n_triangles"] == len(arch[1]) + len(live[1]) and got["n_tri_pixels"] > 100 and got["n_segments"] > 0 and got["n_vertices"] > 1000
        again = call(c, cam, view, archive=True, live=True, **kw)
        assert rmm.same(again, got) == [] and again["rgb"].tobytes() == got["rgb"].tobytes() and again["depth"].tobytes() == got["depth"].tobytes()
        tri_total = got["n_triangles"]
        if kf:
            assert len(arch[1]) > 0
    assert tri_total > 1000
