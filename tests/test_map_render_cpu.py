"""nalo_map_render's model (tests/render_model.py) by hand, its vectorised form against the literal one, and nalo_view_look_at (a host function: no device).
The device is held against the model in tests/test_map_render_gpu.py."""
import numpy as np
import pytest

import render_model as rm
from nalo_slam_amd import binding

f32 = np.float32
EYE = np.eye(3, 4).reshape(12).astype(f32)
WHITE = (255, 255, 255)


def unit_cam(vw=48, vh=40, **kw):
    """fx = fy = 1, cx = cy = 0: at z = 1 a view-space point IS its pixel coordinate"""
    return rm.make_cam(vw, vh, fx=1, fy=1, cx=0, cy=0, **kw)


def cloud(points, cols, M=EYE):
    return (M, np.asarray(points, f32).reshape(-1, 3), np.asarray(cols, np.uint32))


def drawn(r):
    ys, xs = np.nonzero(np.isfinite(r["depth"]))
    return sorted(zip(xs.tolist(), ys.tolist()))


def random_scene(seed, vw, vh):
    rng = np.random.RandomState(seed)
    cam = rm.make_cam(vw, vh, fx=60, fy=55, znear=0.5, zfar=30)
    view = rm.look_at((0.3, -2.0, -6.0), (0, 0, 0), (0, -1, 0))
    clouds = []
    for k in range(3):
        c2w = np.concatenate([np.linalg.qr(rng.randn(3, 3))[0], rng.uniform(-1, 1, (3, 1))], 1)
        n = 400
        xyz = (rng.randn(n, 3) * [2, 2, 4]).astype(f32)
        xyz[::37] = np.nan
        xyz[5::41, 2] = np.inf
        xyz[::9] = np.round(xyz[::9])                                     # vertices that share pixels and depths
        col = rng.randint(0, 1 << 24, n).astype(np.uint32)
        col[::9] = rng.randint(0, 4, len(col[::9]))
        clouds.append((rm.transform(view, c2w), xyz, col))
    segs = []
    for k in range(40):
        a, b = (rng.randn(3) * [4, 4, 6] + [0, 0, 4]).astype(f32), (rng.randn(3) * [4, 4, 6] + [0, 0, 4]).astype(f32)
        segs.append((a, b, int(rng.randint(0, 1 << 24)), int(rng.randint(1, 4))))
    segs.append((np.array([1e30, -1e30, 5], f32), np.array([-1e30, 1e30, 2], f32), rm.RED, 3))
    segs.append((np.array([np.nan, 0, 5], f32), np.array([0, 0, 2], f32), rm.RED, 3))
    segs.append((np.array([1, 1, 3], f32), np.array([1, 1, 3], f32), rm.GREEN, 2))
    return cam, clouds, segs


@pytest.mark.parametrize("seed,vw,vh", [(1, 48, 40), (2, 33, 17), (3, 1, 1)])
def test_vectorised_model_equals_the_literal_one(seed, vw, vh):
    cam, clouds, segs = random_scene(seed, vw, vh)
    a, b = rm.render_literal(cam, (10, 20, 30), clouds, segs), rm.render_vector(cam, (10, 20, 30), clouds, segs)
    assert rm.same(a, b) == []
    if vw > 1:
        assert a["n_drawn_points"] > 20 and a["n_line_samples"] > 100 and 30 <= a["n_segments"] <= 42 and np.isinf(a["depth"]).any()
        assert a["n_line_samples"] <= 42 * (vw + vh + 10)


def test_look_at_against_the_model_and_by_hand():
    got = binding.view_look_at((0, -5, -10), (0, 0, 0), (0, -1, 0))
    assert np.array_equal(got.view(np.uint64), rm.look_at((0, -5, -10), (0, 0, 0), (0, -1, 0)).view(np.uint64))
    s = np.sqrt(125.0)
    want = np.array([[1, 0, 0, 0], [0, 10 / s, -5 / s, 0], [0, 5 / s, 10 / s, s]])          # x right; the world's origin straight ahead at distance sqrt(125)
    assert np.allclose(got, want, rtol=0, atol=4e-16 * s)
    assert got[0, 0] == 1.0 and got[0, 1] == 0.0 and got[0, 3] == 0.0
    rng = np.random.RandomState(4)
    for _ in range(20):
        e, t, u = rng.randn(3) * 5, rng.randn(3), rng.randn(3)
        g = binding.view_look_at(e, t, u)
        assert np.array_equal(g.view(np.uint64), rm.look_at(e, t, u).view(np.uint64))
        assert np.allclose(g[:, :3] @ g[:, :3].T, np.eye(3), atol=1e-12) and np.linalg.det(g[:, :3]) > 0
        assert np.allclose(g[:, :3] @ t + g[:, 3], [0, 0, np.linalg.norm(e - t)], atol=1e-12)     # the target lies on the optical axis, in front
    for bad in (((0, 0, 0), (0, 0, 0), (0, -1, 0)), ((0, -3, 0), (0, 0, 0), (0, -1, 0)), ((np.nan, 0, 1), (0, 0, 0), (0, -1, 0))):
        with pytest.raises(binding.NaloError):
            binding.view_look_at(*bad)


def test_transform_by_hand():
    V = np.array([[1, 0, 0, 10], [0, 1, 0, 20], [0, 0, 1, 30.0]])
    Cm = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3.0]])
    assert np.array_equal(rm.transform(V, Cm).reshape(3, 4), np.array([[0, -1, 0, 11], [1, 0, 0, 22], [0, 0, 1, 33]], f32))
    # the cast comes last: 2^24 + 1 survives the double sum and rounds only at the end
    V2 = np.array([[1, 1, 0, 1.0], [0, 1, 0, 0], [0, 0, 1, 0]])
    C2 = np.array([[0, 0, 0, 2.0 ** 24], [0, 0, 0, 1.0], [0, 0, 1, 0]])
    assert rm.transform(V2, C2)[3] == f32(2.0 ** 24 + 2)


def test_projection_by_hand():
    cam = rm.make_cam(48, 40, fx=40, fy=40, znear=0.1, zfar=1000)
    r = rm.render_literal(cam, WHITE, [cloud([[0.5, -0.25, 2.0]], [0x102030])], [])
    assert drawn(r) == [(34, 15)]                                          # u = 40 * 0.25 + 24, v = 40 * -0.125 + 20
    assert r["depth"][15, 34] == f32(2) and tuple(r["rgb"][15, 34]) == (0x10, 0x20, 0x30) and tuple(r["rgb"][0, 0]) == WHITE
    assert (r["n_vertices"], r["n_drawn_points"]) == (1, 1)
    c = unit_cam(znear=1, zfar=4)
    pts = [[0, 0, 1], [0, 0, 4], [-0.5, 3, 2], [-0.0, 3, 2], [96, 3, 2], [95.5, 79.5, 2], [3, 80, 2], [np.nan, 0, 2], [3e38, 0, 1.5]]
    r = rm.render_literal(c, WHITE, [cloud(pts, np.arange(9))], [])
    # zv == znear and zv == zfar are culled; u in (-1, 0) is culled (a truncating cast would draw it); -0.0 is column 0; u == vw and v == vh are culled
    assert drawn(r) == [(0, 1), (47, 39)] and r["n_drawn_points"] == 2 and r["n_vertices"] == 9


def test_a_3_4_5_segment():
    c = unit_cam()
    a, b = np.array([10, 10, 1], f32), np.array([13, 14, 1], f32)
    L = rm.clip_line(c, a, b)
    assert (L["n"], L["k0"], L["count"]) == (4, 0, 5)
    assert [(x, y) for x, y, _ in rm.line_samples(c, L)] == [(10, 10), (10, 11), (11, 12), (12, 13), (13, 14)]      # u = 10 + 0.75 k
    r = rm.render_literal(c, WHITE, [], [(a, b, rm.RED, 1)])
    assert drawn(r) == [(10, 10), (10, 11), (11, 12), (12, 13), (13, 14)] and (r["n_segments"], r["n_line_samples"]) == (1, 5)
    # depth is interpolated in 1 / z
    L = rm.clip_line(c, np.array([0, 0, 1], f32), np.array([0, 8, 2], f32))         # v: 0 -> 4
    assert [z for _, _, z in rm.line_samples(c, L)] == [f32(1 / (1 - t / 2)) for t in (0, 0.25, 0.5, 0.75, 1)]


def test_near_clip_by_hand():
    c = unit_cam(znear=1, zfar=100)
    L = rm.clip_line(c, np.array([2, 0, 0], f32), np.array([4, 0, 2], f32))         # t = (1 - 0) / (2 - 0): the end becomes (3, 0, 1)
    assert (L["ua"], L["va"], L["za"], L["ub"], L["zb"]) == (3, 0, 1, 2, 2)
    M = rm.clip_line(c, np.array([4, 0, 2], f32), np.array([2, 0, 0], f32))         # from the other end
    assert (M["ub"], M["zb"], M["ua"], M["za"]) == (3, 0 + 1, 2, 2)
    assert rm.clip_line(c, np.array([2, 0, 0], f32), np.array([4, 0, 1], f32)) is None          # both z <= znear
    assert rm.clip_line(c, np.array([2, 0, np.inf], f32), np.array([4, 0, 2], f32)) is None
    far = rm.clip_line(c, np.array([1e30, 0, 2], f32), np.array([-1e30, 5, 2], f32))
    assert 0 < far["count"] <= 48 + 40 + 10
    out = rm.clip_line(c, np.array([-50, 5, 2], f32), np.array([-20, 30, 2], f32))               # wholly left of the viewport: a segment without a sample
    assert out is not None and out["count"] == 0


def test_width_blocks():
    assert [list(rm.width_block(L)) for L in (1, 2, 3)] == [[0], [-1, 0], [-1, 0, 1]]
    c = unit_cam()
    p = np.array([5.5, 7.5, 1], f32)
    for L, want in ((1, [(5, 7)]), (2, [(4, 6), (4, 7), (5, 6), (5, 7)]), (3, [(x, y) for x in (4, 5, 6) for y in (6, 7, 8)])):
        r = rm.render_literal(c, WHITE, [], [(p, p, rm.GREEN, L)])
        assert drawn(r) == sorted(want) and r["n_line_samples"] == 1
    r = rm.render_literal(c, WHITE, [], [(np.array([0.5, 0.5, 1], f32),) * 2 + (rm.GREEN, 3)])    # clipped to the image at the corner
    assert drawn(r) == [(0, 0), (0, 1), (1, 0), (1, 1)]


def test_the_tie_rule():
    c = unit_cam()
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        pts = np.array([[3, 3, 2], [3.5, 3.25, 2], [3, 3, 3]], f32)[list(order)]
        cols = np.array([0x00FF00, 0x0000FF, 0x000001], np.uint32)[list(order)]
        for render in (rm.render_literal, rm.render_vector):
            r = render(c, WHITE, [cloud(pts, cols)], [])
            # (3, 3, 2) and (3.5, 3.25, 2) share pixel (1, 1) at depth 2: the smaller colour word wins; the farther vertex loses whatever its colour
            assert drawn(r) == [(1, 1)] and tuple(r["rgb"][1, 1]) == (0, 0, 255) and r["depth"][1, 1] == 2 and r["n_drawn_points"] == 3
