"""nalo_map_render - the viewer's 3-D panel on the device - against the literal model of tests/render_model.py.

Every comparison is bit for bit over EVERY pixel of rgb and depth and over the four counts (render_model.same). The model's point input is what
map_model.set_from_kf / refresh_pc give for the records the library's public read-backs show (the way tests/test_map_gpu.py builds them: scene, plant,
keyframe, immature_set, frame_records) and dense_map_model.refresh_pc_fast for nalo_map_dense_get's points.

  1  planted single points (frame 64x32, view 48x40): the viewport's and the depth range's edges, -0.0, idepths 0 / negative / NaN / +inf, an overflowing x / z
  2  the depth test: submission orders, two frames, sparse against dense, point against line, equal depths, display_mode 0's colours
  3  display modes, every filter clause, with_immature; n_vertices against nalo_map_frame_cloud
  4  the work split: planted record counts, chunks of 64 records, 1 / 2 / 17 listed frames, a frame with dense records only
  5  lines: frusta, planted segments, strips, constraints
  6  the key plane's self-cleaning over sizes
  7  three keyframes of the device chain at 1224x368, W = 8, everything on, view 640x480
  8  no side effects
  9  refusals"""
import ctypes as C

import numpy as np
import pytest

import lifecycle_model as lm
import lifecycle_scenes as sc
import map_model as mm
import plane_cases as pc
import plane_model as pm
import render_model as rm
import test_dense_map_gpu as tdm
import test_map_gpu as tmg
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
ERR_ARG, ERR_STATE = -1, -4
BIG = 1e30
EYE = np.eye(3, 4)
START = rm.look_at((0, -5, -10), (0, 0, 0), (0, -1, 0))                      # the viewer's start view
GREY = (40, 50, 60)


# ------------------------------------------------------------------------------------------------ device call and model side by side
def cam_kw(cam):
    return dict(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], znear=cam["znear"], zfar=cam["zfar"])


def calib(c):
    cal = c.ba_get_frames()[2]
    return mm.calib_inverse(cal), np.asarray(cal[:4], f32)


def expect(c, cam, view, frames, recs=None, dense=None, mode=0, th=(BIG, BIG, 0.0), literal=False, background=GREY, extra_segs=(), **lines):
    """the model's picture. recs: {frame_id: RECORD array (setFromKF's list)}; dense: {frame_id: nalo_map_dense_get's points}; lines: render_model.segments' flags"""
    ci, cf = calib(c)
    clouds = []
    for fid, m in frames:
        M = rm.transform(view, m)
        if recs is not None and fid in recs:
            clouds.append((M,) + rm.sparse_vertices(recs[fid], ci, mode, *th))
        if dense is not None and fid in dense:
            clouds.append((M,) + rm.dense_vertices(dense[fid], ci))
    segs = rm.segments(view, frames, cf, c.w, c.h, **lines) + list(extra_segs)
    return (rm.render_literal if literal else rm.render_vector)(cam, background, clouds, segs)


def call(c, cam, view, frames, mode=0, th=(BIG, BIG, 0.0), with_immature=True, with_dense=False, background=GREY, connections=None, show_active=False, show_all=False,
         show_kf_cams=False, current_cam=None, show_trajectory=False, all_poses=None):
    return c.map_render(cam["vw"], cam["vh"], view, frames, display_mode=mode, scaledTH=th[0], absTH=th[1], minRelBS=th[2], with_immature=with_immature, with_dense=with_dense,
                        background=background, show_active_constraints=show_active, show_all_constraints=show_all, show_kf_cams=show_kf_cams, current_cam=current_cam,
                        show_trajectory=show_trajectory, all_poses=all_poses, **cam_kw(cam))


def check(c, cam, view, frames, recs=None, dense=None, mode=0, th=(BIG, BIG, 0.0), with_immature=True, literal=False, what="", **lines):
    want = expect(c, cam, view, frames, recs, dense, mode, th, literal, **lines)
    got = call(c, cam, view, frames, mode, th, with_immature, dense is not None, **lines)
    bad = rm.same(got, want)
    assert bad == [], (what, bad, {k: (got[k], want[k]) for k in bad if k.startswith("n_")}, int((got["rgb"] != want["rgb"]).any(2).sum()))
    return got


def drawn(r):
    ys, xs = np.nonzero(np.isfinite(r["depth"]))
    return sorted(zip(xs.tolist(), ys.tolist()))


# ------------------------------------------------------------------------------------------------ planted windows
PK = (32.0, 32.0, 16.0, 8.0)           # fxi = 1 / 32, cxi = -0.5, cyi = -0.25: with a depth that is a power of two, x / z of a vertex is exactly (u + dx) / 32 - 0.5


def planted(u, v, idepth, host=None, color=None, w=64, h=32, K=PK, W=2, fids=None, c2w=None, chunk=0, archive=False):
    """a window of W frames (identity poses unless c2w) with exactly these points, all valid -> (context, S)"""
    u, v, idepth = (np.ascontiguousarray(a, f32) for a in (u, v, idepth))
    P = len(u)
    host = np.zeros(P, np.int32) if host is None else np.ascontiguousarray(host, np.int32)
    color = np.tile(np.arange(8, dtype=f32) * 10 + 100, (P, 1)) if color is None else np.ascontiguousarray(color, f32).reshape(P, 8)
    fids = [10 + i for i in range(W)] if fids is None else list(fids)
    c = binding.Context(w, h, K, n_slots=W)
    rng = np.random.RandomState(1)
    for i in range(W):
        c.frame_upload(i, rng.uniform(5, 250, (h, w)).astype(f32))
    c2w = np.tile(EYE, (W, 1, 1)) if c2w is None else np.asarray(c2w, np.float64)
    c.ba_set_window(list(range(W)), np.stack([synth.se3_inv(m) for m in c2w]), frame_ids=fids)
    c.ba_set_points(host, u, v, idepth, color, np.ones((P, 8), f32))
    if archive:
        c.map_enable(chunk_points=chunk)
    return c, dict(host=host, u=u, v=v, color=color, fids=fids, c2w=c2w, hp=np.zeros(P, np.int32))


def active_records(c, S, widx, keep=None):
    """status 1 of window frame widx from the context's read-backs (every point valid unless keep says otherwise)"""
    p = c.ba_get_points()
    sel = S["host"] == widx
    if keep is not None:
        sel &= keep
    idx = np.nonzero(sel)[0]
    act = np.zeros(len(idx), mm.RECORD)
    act["u"], act["v"], act["idepth"], act["color"] = S["u"][idx], S["v"][idx], p["idepth"][idx], S["color"][idx]
    act["idepth_hessian"] = lm.idepth_hessian(p["Hdd"], p["HdiF"], S["hp"])[idx]
    act["maxRelBaseline"] = p["maxRelBaseline"][idx]
    return act


def archive_records(c, fid):
    a = c.map_get_frame(fid)
    return a[a["status"] == 2], a[a["status"] == 3]


PCAM = rm.make_cam(48, 40, fx=32, fy=32, cx=16, cy=8, znear=0.1, zfar=1000)    # undoes PK: a vertex of a depth-2 point at (u, v) lands on u_pix = u + dx, v_pix = v + dy


def test_planted_points_at_the_edges():
    #       0: a vertex with u exactly 0 (dx = -2) | 1: u_pix in (-1, 0) | 2: u == vw | 3-6: idepth 0, negative, NaN, +inf | 7: an ordinary point | 8: x = +0 (the -0.0 case)
    u = [2.0, 1.5, 46.0, 20, 22, 24, 26, 30.25, 16.0]
    v = [10.0, 20.0, 30.0, 5, 5, 5, 5, 12.5, 25.0]
    idp = [0.5, 0.5, 0.5, 0.0, -0.5, np.nan, np.inf, 0.25, 0.5]
    c, S = planted(u, v, idp)
    recs = {10: mm.set_from_kf(None, active_records(c, S, 0))}
    assert mm.bits_equal(recs[10]["idepth"], np.array(idp, f32))                                 # the planted values reached the window as they are
    frames = [(10, EYE)]
    inf = float("inf")
    g = check(c, PCAM, EYE, frames, recs, th=(inf, inf, 0.0), literal=True, what="edges")
    d = drawn(g)
    assert (0, 10) in d and g["depth"][10, 0] == 2                                               # u == 0 exactly is column 0
    assert (0, 20) not in d and (0, 19) in d and (1, 19) not in d                                # u_pix = -0.5 (dx = -2) is culled; u_pix = 0.5 (dx = -1, dy = -1) is drawn
    assert (47, 29) in d and (47, 30) not in d and (46, 30) in d                                 # u_pix = 47 (dx = 1, dy = -1) is the last column; u_pix == 48 == vw (dx = 2) is culled
    assert (30, 12) in d and g["depth"][12, 30] == 4
    # idepth +inf: depth 0, all 8 vertices at the camera centre: zv = 0 fails the depth range. idepth 0 with infinite thresholds: depth inf, NaN / inf vertices
    assert g["n_vertices"] == 8 * 8 and g["n_drawn_points"] >= len(d)                            # every record but the negative one passes the filter
    assert not any(y < 8 for x, y in d if 15 <= x <= 30)                                        # nothing of points 3-6 is drawn
    # zv == znear and zv == zfar (depth-2 points): both culled, the depth-4 point stays
    for zn, zf in ((2.0, 1000.0), (0.1, 2.0)):
        cam = dict(PCAM, znear=f32(zn), zfar=f32(zf))
        g2 = check(c, cam, EYE, frames, recs, th=(inf, inf, 0.0), literal=True, what="range %g %g" % (zn, zf))
        assert (0, 10) not in drawn(g2) and ((30, 12) in drawn(g2)) == (zf > 4)
    # the camera centre 1 behind the view plane moves +inf-idepth vertices (depth 0) to zv = 1: all 8 on the principal point, one pixel
    back = np.concatenate([np.eye(3), [[0], [0], [1.0]]], 1)
    g3 = check(c, PCAM, back, frames, recs, th=(inf, inf, 0.0), literal=True, what="idepth inf")
    assert g3["depth"][8, 16] == 1
    # -0.0: a view whose first row is (-1, -0, -0, -0) and cx = -0.0 give u = -0.0 for x = +0 (u + dx = 16): column 0, not culled
    flip = np.array([[-1.0, -0.0, -0.0, -0.0], [0, 1, 0, 0], [0, 0, 1, 0]])
    camz = dict(PCAM, cx=f32(-0.0))
    assert np.signbit(rm.transform(flip, EYE)[:4]).all()
    g4 = check(c, camz, flip, frames, recs, th=(inf, inf, 0.0), literal=True, what="-0.0")
    assert g4["depth"][25, 0] == 2 and g4["depth"][23, 0] == 2 and g4["depth"][27, 0] == 2
    # xv / zv overflows: a view translation of 3e38 and depth-0.5 vertices... the planted depths are 2 and 4, so scale the view instead: x / z = 3e38 / 2 * 4 overflows in u
    far = np.array([[1.0, 0, 0, 3e38], [0, 1, 0, 0], [0, 0, 1e-3, 0]])
    camf = dict(PCAM, znear=f32(1e-4))
    with np.errstate(all="ignore"):
        p = rm.apply(rm.transform(far, EYE), np.array([0, 0, 2], f32))
        assert np.isinf(p[0] / p[2])
    g5 = check(c, camf, far, frames, recs, th=(inf, inf, 0.0), literal=True, what="overflow")
    assert g5["n_drawn_points"] == 0 and g5["n_vertices"] == 8 * 8 and (g5["rgb"] == np.array(GREY, np.uint8)).all() and np.isinf(g5["depth"]).all()
    c.close()


def test_depth_test():
    # points 0 and 1 share every pixel at different depths, 2 and 3 are the same pair submitted in the other order; 4 and 5 have equal depths and different colours
    u = [10, 10, 30, 30, 20, 20, 40]
    v = [10, 10, 10, 10, 25, 25, 25]
    idp = [0.5, 0.25, 0.25, 0.5, 0.5, 0.5, 1.0]
    col = np.array([[200] * 8, [50] * 8, [50] * 8, [200] * 8, [90] * 8, [30] * 8, [120] * 8], f32)
    host = [0, 0, 0, 0, 0, 0, 1]
    c, S = planted(u, v, idp, host=host, color=col)
    recs = {10: mm.set_from_kf(None, active_records(c, S, 0)), 11: mm.set_from_kf(None, active_records(c, S, 1))}
    frames = [(10, EYE), (11, EYE)]
    g = check(c, PCAM, EYE, frames, recs, mode=1, literal=True, what="orders")
    assert tuple(g["rgb"][10, 10]) == (200,) * 3 and tuple(g["rgb"][10, 30]) == (200,) * 3 and g["depth"][10, 10] == 2 and g["depth"][10, 30] == 2     # the nearer one, in both orders
    assert tuple(g["rgb"][25, 20]) == (30,) * 3                                                  # equal depths: the smaller colour word
    # display_mode 0: status 1 is (0, 255, 0) whatever the record's colours
    g0 = check(c, PCAM, EYE, frames, recs, mode=0, literal=True, what="mode 0")
    assert tuple(g0["rgb"][10, 10]) == (0, 255, 0) and tuple(g0["rgb"][25, 40]) == (0, 255, 0)
    # across two frames: frame 11's point (depth 1, x = 0.75) moved by -0.625 lands on frame 10's pixel (20, 25), in front of the two points there
    near = np.concatenate([np.eye(3), [[-0.625], [0], [0]]], 1)
    frames2 = [(10, EYE), (11, near)]
    g2 = check(c, PCAM, EYE, frames2, recs, mode=1, literal=True, what="two frames")
    assert g2["depth"][25, 20] == 1 and tuple(g2["rgb"][25, 20]) == (120,) * 3 and g["depth"][25, 20] == 2
    # a point against a line: a width-3 strip through pixel (10, 10) in front of the point, and one behind it
    for z, wins in ((1.0, True), (3.0, False)):
        x0, y0 = (10.5 - 16) / 32 * z, (10.5 - 8) / 32 * z
        poses = np.array([[x0 - 0.2 * z, y0, z], [x0 + 0.2 * z, y0, z]], f32)
        g3 = check(c, PCAM, EYE, frames, recs, mode=1, literal=True, all_poses=poses, what="line %g" % z)
        assert (tuple(g3["rgb"][10, 10]) == (0, 255, 0)) == wins and g3["n_line_samples"] > 5
    c.close()


# ------------------------------------------------------------------------------------------------ the small keyframe of tests/test_map_gpu.py
@pytest.fixture(scope="module")
def small():
    """tests/test_map_gpu.py's small scene after one keyframe with host 1 flagged, on an archiving context with the graph on and a resident immature set"""
    S = tmg.scene(640, 480, 4, 400)
    A = tmg.make_ctx(S)
    A.map_enable(chunk_points=64)
    A.map_graph_enable()
    A.ba_set_point_history(*sc.plant_history(400, 4))
    A.ba_linearize(False)
    A.ba_linearize(True)
    k = tmg.keyframe(A, S, sc.flag_sets(4)[1])
    imm = tmg.immature_set(500, 4, 640, 480)
    A.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
    c2w = [synth.se3_inv(S["win"].world_to_cam[i]) for i in range(4)]
    frames = [(100 + i, c2w[i]) for i in range(4)]
    recs = {100 + i: tmg.frame_records(S, k, 100 + i, i, imm) for i in range(4)}
    noimm = {100 + i: tmg.frame_records(S, k, 100 + i, i, None) for i in range(4)}
    # a view from behind and above the first camera that sees most of the cloud
    view = rm.look_at((0.5, -1.5, -4.0), (0, 0, 3.0), (0, -1, 0))
    yield dict(S=S, A=A, k=k, imm=imm, frames=frames, recs=recs, noimm=noimm, view=view, cam=rm.make_cam(96, 72, fx=60, fy=60, znear=0.1, zfar=1000))
    A.close()


def test_modes_clauses_and_immature(small):
    A, frames, view, cam = small["A"], small["frames"], small["view"], small["cam"]
    rec = np.concatenate([small["recs"][f] for f, _ in frames])
    ok = rec["idepth"] >= 0
    var, sc4 = tmg.clause_values(rec)
    th_sc, th_abs, th_bs = np.median(sc4[ok & np.isfinite(sc4)]), np.median(var[ok]), np.median(rec["maxRelBaseline"][rec["maxRelBaseline"] > 0])
    n_all = None
    for mode, th, what in ((0, (BIG, BIG, 0.0), "all"), (0, (th_sc, BIG, 0.0), "scaled"), (0, (BIG, th_abs, 0.0), "abs"), (0, (BIG, BIG, th_bs), "baseline"),
                           (1, (th_sc, th_abs, th_bs), "mode 1"), (1, (BIG, BIG, 0.0), "mode 1 all"), (2, (BIG, BIG, 0.0), "mode 2"), (3, (BIG, BIG, 0.0), "mode 3")):
        g = check(A, cam, view, frames, small["recs"], mode=mode, th=th, what=what)
        n_cloud = sum(len(A.map_frame_cloud(f, mode, *th)["xyz"]) for f, _ in frames)
        print("RENDER small %-10s vertices %d drawn %d" % (what, g["n_vertices"], g["n_drawn_points"]))
        assert g["n_vertices"] == n_cloud
        if what == "all":
            n_all = g["n_vertices"]
            assert g["n_drawn_points"] > 500 and len(np.unique(g["rgb"].reshape(-1, 3), axis=0)) >= 5       # background + the four status colours
        elif mode == 3:
            assert g["n_vertices"] == 0 and (g["rgb"] == np.array(GREY, np.uint8)).all()
        else:
            assert 0 < g["n_vertices"] < n_all, what                                                         # the clause (the mode) rejects some records and keeps some
    g = check(A, cam, view, frames, small["noimm"], mode=0, with_immature=False, what="without the immature class")
    assert g["n_vertices"] == sum(len(A.map_frame_cloud(f, 0, BIG, BIG, 0.0, with_immature=False)["xyz"]) for f, _ in frames) < n_all
    # the literal model on one frame and a smaller picture
    check(A, rm.make_cam(40, 30, fx=25, fy=25), view, frames[2:3], small["recs"], mode=1, literal=True, what="literal")


def test_frusta_trajectories_and_constraints(small):
    A, frames, view, cam, recs = small["A"], small["frames"], small["view"], small["cam"], small["recs"]
    conn = A.map_graph_connections()
    act = conn["fwdAct"] + conn["bwdAct"]
    print("RENDER small connections: %d, with act %d" % (len(conn), int((act > 0).sum())))
    assert (act > 0).sum() >= 3
    # the cameras are 3e-4 apart in this scene: spread the listed poses so that frusta and strips cover pixels (the library draws the poses it is given)
    spread = [(f, np.concatenate([m[:, :3], m[:, 3:] + [[0.8 * i], [0.1 * i], [0.5 * i]]], 1)) for i, (f, m) in enumerate(frames)]
    cur = np.concatenate([np.eye(3), [[-0.6], [-0.3], [1.0]]], 1)
    poses = np.cumsum(np.random.RandomState(3).randn(300, 3) * 0.05, 0).astype(f32) + f32([0, 0, 2])
    g = check(A, cam, view, spread, None, mode=3, what="lines only", show_kf_cams=True, current_cam=cur, connections=conn, show_active=True, show_all=True, show_trajectory=True, all_poses=poses)
    cols = {tuple(x) for x in np.unique(g["rgb"].reshape(-1, 3), axis=0)}
    assert {(0, 0, 255), (255, 0, 0), (0, 255, 0), GREY} <= cols and g["n_segments"] >= 4 * 8 + 8 + 3 + 3 + 250
    g1 = check(A, cam, view, spread, recs, mode=1, what="lines and points", show_kf_cams=True, current_cam=cur, connections=conn, show_active=True, show_trajectory=True)
    assert g1["n_drawn_points"] > 500 and g1["n_line_samples"] > 100
    # an unlisted end: without frame 101 every connection that touches it is skipped
    three = [s for s in spread if s[0] != 101]
    g2 = check(A, cam, view, three, None, mode=3, what="unlisted end", connections=conn, show_active=True, show_all=True)
    marg = conn["fwdMarg"] + conn["bwdMarg"]
    drawn_c = (act > 0) | ((act == 0) & (marg > 0))
    assert g2["n_segments"] == int((drawn_c & (conn["from_id"] != 101) & (conn["to_id"] != 101)).sum()) < int(drawn_c.sum())
    # strips of 0, 1 and 2 poses; 0 and 1 listed frames with show_trajectory
    for n in (0, 1, 2):
        g3 = check(A, cam, view, spread[:n], None, mode=3, what="strip %d" % n, show_trajectory=True, all_poses=poses[:n])
        assert g3["n_segments"] == 2 * max(n - 1, 0)
    # the literal model on a small picture
    check(A, rm.make_cam(40, 30, fx=25, fy=25), view, spread, None, mode=3, literal=True, what="literal lines", show_kf_cams=True, current_cam=cur, connections=conn, show_active=True,
          show_trajectory=True, all_poses=poses[:40])


def seg_poses(cam, pts):
    """all_poses that draw the segments pts[i] -> pts[i + 1] (view space = world space under the identity view)"""
    return np.asarray(pts, f32).reshape(-1, 3)


def test_planted_segments():
    c, S = planted([30.0], [12.0], [0.5])
    cam = rm.make_cam(48, 40, fx=1, fy=1, cx=0, cy=0, znear=1, zfar=100)          # at z = 2 a point (x, y, 2) is the pixel (x / 2, y / 2)
    z = 2.0
    px = lambda x, y, zz=z: [x * zz, y * zz, zz]
    cases = {
        "horizontal": [px(3.5, 5.5), px(40.5, 5.5)], "vertical": [px(7.5, 2.5), px(7.5, 37.5)], "diagonal": [px(1.5, 1.5), px(30.5, 30.5)], "steep": [px(20.5, 1.5), px(23.5, 38.5)],
        "A == B": [px(9.5, 9.5), px(9.5, 9.5)], "two corners": [px(0, 0), px(48, 40)], "other corners": [px(48, 0), px(0, 40)], "outside": [px(-30, 5), px(-5, 60)],
        "behind": [[1, 1, 0.5], [5, 5, -3]], "crossing from A": [[5, 5, -1], [40, 30, 3]], "crossing from B": [[40, 30, 3], [5, 5, -1]], "touching the plane": [[5, 5, 1], [40, 30, 3]],
        "1e30": [[1e30, -1e30, 5], [-1e30, 1e30, 2]], "1e30 far": [[1e30, 1e30, 1e30], [-1e30, 3, 2]], "NaN": [[np.nan, 3, 2], [5, 5, 2]], "inf": [[np.inf, 3, 2], [5, 5, 2]],
        "beyond zfar": [px(3, 3, 50), px(40, 30, 150)],
    }
    for name, pts in cases.items():
        g = check(c, cam, EYE, [], None, literal=True, what=name, all_poses=seg_poses(cam, pts))
        assert g["n_line_samples"] <= 48 + 40 + 10, name
        if name in ("outside",):
            assert g["n_segments"] == 1 and g["n_line_samples"] == 0
        if name in ("behind", "NaN", "inf"):
            assert g["n_segments"] == 0 and np.isinf(g["depth"]).all()
        if name in ("horizontal", "vertical", "diagonal", "steep", "A == B", "two corners", "crossing from A", "crossing from B", "1e30"):
            assert g["n_segments"] == 1 and g["n_line_samples"] >= 1 and np.isfinite(g["depth"]).any(), name
    # widths 1, 2 and 3 against every border: the trajectory strip is width 3, the current camera width 2, the keyframe cameras width 1; a frame along each border
    ring = [px(0.5, 0.5), px(47.5, 0.5), px(47.5, 39.5), px(0.5, 39.5), px(0.5, 0.5)]
    g = check(c, cam, EYE, [], None, literal=True, what="width 3 on the borders", all_poses=seg_poses(cam, ring))
    assert all(np.isfinite(g["depth"][e]).all() for e in ((0, slice(None)), (39, slice(None)), (slice(None), 0), (slice(None), 47)))
    # the frustum of a camera whose image corners project onto the view's corners: base z = sz, corners (sz * (0 - cx) / fx ..): widths 2 (current) and 1 (keyframe)
    fr = rm.frustum(calib(c)[1], c.w, c.h, 0.2)
    sx, sy = 47.0 / (fr[3, 0] - fr[1, 0]), 39.0 / (fr[3, 1] - fr[1, 1])
    # (the keyframe camera's base, sz = 0.1, has the same x / z and y / z: one view camera serves both)
    camw = rm.make_cam(48, 40, fx=0.2 * sx, fy=0.2 * sy, cx=0.5 - sx * fr[1, 0], cy=0.5 - sy * fr[1, 1], znear=0.01, zfar=100)
    for width, kw in ((2, dict(current_cam=EYE)), (1, dict(show_kf_cams=True))):
        g = check(c, camw, EYE, [(10, EYE)], None, mode=3, literal=True, what="width %d on the borders" % width, **kw)      # display_mode 3: no points
        assert g["n_segments"] >= 4 and np.isfinite(g["depth"][0]).sum() > 40 and np.isfinite(g["depth"][:, 0]).sum() > 30 and np.isfinite(g["depth"][39]).sum() > 40 and np.isfinite(g["depth"][:, 47]).sum() > 30
    c.close()


def test_constraint_classes():
    """a connection with act > 0, one with act == 0 && marg > 0 (a frame whose points were all removed and that nobody observes), one with neither (a frame without
    any residual)"""
    WW = 6
    win = synth.make_window(w=320, h=240, W=WW, P=1200, seed=sc.SEED, n_extra=0, step_z=0.8 * 3e-4, step_x=0.03 * 3e-4, full_graph=False)
    A = binding.Context(win.w, win.h, win.K, n_slots=WW)
    for i in range(WW):
        A.frame_upload(i, win.images[i])
    fids = [200 + i for i in range(WW)]
    A.map_graph_enable()
    A.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)[:WW], frame_ids=fids)
    A.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    exists = win.exists.copy()
    exists[:, 0] = 0                                                                            # nobody observes in frame 0: once its own points are gone its pairs have no live residual
    exists[:, WW - 1] = 0                                                                       # nobody observes in the newest frame ...
    exists[win.host == WW - 1] = 0                                                              # ... and its points observe nowhere: its pairs never had a residual
    A.ba_set_residuals(exists)
    A.ba_set_point_history(*sc.plant_history(len(win.host), WW))
    A.map_enable()
    A.ba_linearize(False)
    A.ba_linearize(True)
    ff = np.zeros(WW, np.uint8); ff[0] = 1
    dec, _, _ = A.ba_flag_points(ff)
    A.ba_marginalize_flagged()
    conn = A.map_graph_connections()
    act, marg = conn["fwdAct"] + conn["bwdAct"], conn["fwdMarg"] + conn["bwdMarg"]
    print("RENDER constraint classes: decisions %s; act %d, marg only %d, neither %d of %d" %
          (np.bincount(dec, minlength=4).tolist(), (act > 0).sum(), ((act == 0) & (marg > 0)).sum(), ((act == 0) & (marg == 0)).sum(), len(conn)))
    assert (act > 0).any() and ((act == 0) & (marg > 0)).any() and ((act == 0) & (marg == 0)).any()
    c2w = {200 + i: np.concatenate([np.eye(3), [[0.7 * i - 1.5], [0.2 * (i % 2)], [2.0 + 0.3 * i]]], 1) for i in range(WW)}
    frames = [(f, c2w[f]) for f in sorted(c2w)]
    cam = rm.make_cam(64, 48, fx=30, fy=30)
    kw = dict(connections=conn, literal=True, mode=3)
    both = check(A, cam, EYE, frames, None, what="both", show_active=True, show_all=True, **kw)
    a = check(A, cam, EYE, frames, None, what="active", show_active=True, **kw)
    b = check(A, cam, EYE, frames, None, what="all", show_all=True, **kw)
    assert a["n_segments"] == (act > 0).sum() and b["n_segments"] == ((act == 0) & (marg > 0)).sum() and both["n_segments"] == a["n_segments"] + b["n_segments"]
    assert (0, 0, 255) in {tuple(x) for x in a["rgb"].reshape(-1, 3)} and (0, 255, 0) in {tuple(x) for x in b["rgb"].reshape(-1, 3)}
    A.close()


# ------------------------------------------------------------------------------------------------ 4: the work split
def test_record_counts_chunk_borders_and_many_frames():
    """tests/test_map_gpu.py's planted removal sizes (0, 1, 255, 256, 257, 513 of 600 points per host) with chunks of 64 records: archive runs cross chunk borders,
    the window segments hold 600, 599, 345, 344, 343 and 87 records; then immature sets of 0, 1, 63, 64, 65 points"""
    sizes = [0, 1, 255, 256, 257, 513]
    S = tmg.planted_scene(sizes)
    A = tmg.make_ctx(S)
    A.map_enable(chunk_points=64)
    A.ba_set_point_history(*tmg.plant(S, sizes, 20))
    A.ba_linearize(False)
    k = tmg.keyframe(A, S, np.zeros(6, np.uint8))
    assert [int(((S["host"] == h) & (k["dec"] != lm.KEEP)).sum()) for h in range(6)] == sizes
    win = S["win"]
    c2w = [synth.se3_inv(win.world_to_cam[i]) for i in range(6)]
    view = rm.look_at((0.5, -1.5, -4.0), (0, 0, 3.0), (0, -1, 0))
    cam = rm.make_cam(96, 72, fx=60, fy=60)
    for n_imm in (0, 1, 63, 64, 65):
        imm = None
        if n_imm:
            imm = tmg.immature_set(n_imm, 1, win.w, win.h, seed=n_imm)
            imm["host_idx"][:] = 5
            A.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
        recs = {100 + i: tmg.frame_records(S, k, 100 + i, i, imm) for i in range(6)}
        for lst in ([0], [5, 2], [3, 4, 5, 0, 1, 2]) if n_imm in (0, 65) else ([5],):
            frames = [(100 + i, c2w[i]) for i in lst]
            g = check(A, cam, view, frames, recs, mode=0, what="imm %d frames %s" % (n_imm, lst))
            assert g["n_vertices"] == sum(len(A.map_frame_cloud(f, 0, BIG, BIG, 0.0)["xyz"]) for f, _ in frames)
    A.close()


def test_planted_class_sizes():
    """window hosts of exactly 0, 1, 63, 64, 65, 255, 256, 257 and 513 valid points (nine frames, every kind-1 segment of another length, borders between segments
    at every phase of the 256-lane workgroups and of their four waves), then resident immature sets of 255, 256, 257 and 513 points, all of one host and spread over
    the hosts. The archive's sizes are planted in the test above; the dense class has no planted sizes: a frame's dense points are what makeMap leaves of a fitted
    cluster's grid, so their number is an outcome of the fit, not an input (the dense tests below print the counts they get and run with chunks of 64 points)."""
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 513]
    W, P = len(sizes), sum(sizes)
    rng = np.random.RandomState(8)
    host = np.repeat(np.arange(W), sizes)
    c2w = [np.concatenate([np.eye(3), [[0.5 * i - 2.0], [0.3 * (i % 3) - 0.3], [0.25 * i]]], 1) for i in range(W)]
    c, S = planted(rng.uniform(4, 60, P), rng.uniform(4, 28, P), rng.uniform(0.2, 1.0, P), host=host, color=rng.uniform(0, 255, (P, 8)), W=W, c2w=c2w)
    frames = [(10 + i, c2w[i]) for i in range(W)]
    cam = rm.make_cam(96, 72, fx=40, fy=40)
    view = rm.look_at((0.5, -1.0, -4.0), (0, 0, 2.0), (0, -1, 0))
    act = {i: active_records(c, S, i) for i in range(W)}
    assert [len(act[i]) for i in range(W)] == sizes

    def records(imm):
        out = {}
        for i in range(W):
            im = None
            if imm is not None:
                sel = imm["host_idx"] == i
                im = dict(u=imm["u"][sel], v=imm["v"][sel], idepth_min=imm["idmin"][sel], idepth_max=imm["idmax"][sel], color=imm["color"][sel])
            out[10 + i] = mm.set_from_kf(im, act[i])
        return out

    recs = records(None)
    for lst in ([0], [1], [2, 3], [4, 5, 6], [8, 7], list(range(W)), list(range(W))[::-1]):
        g = check(c, cam, view, [frames[i] for i in lst], recs, mode=1, what="window hosts %s" % lst)
        assert g["n_vertices"] == 8 * sum(sizes[i] for i in lst)                                 # positive depths, thresholds off: every record survives
    for n_imm, one_host in ((255, True), (256, True), (257, False), (513, True), (513, False)):
        imm = tmg.immature_set(n_imm, W, 64, 32, seed=n_imm)
        if one_host:
            imm["host_idx"][:] = 4
        c.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
        recs = records(imm)
        n0 = sum(int((r["status"] == 0).sum()) for r in recs.values())
        assert n0 == n_imm
        for lst in ([4], [0, 4], list(range(W))):
            fr = [frames[i] for i in lst]
            g = check(c, cam, view, fr, recs, mode=0, what="immature %d %s frames %s" % (n_imm, one_host, lst))
            assert g["n_vertices"] == sum(len(c.map_frame_cloud(f, 0, BIG, BIG, 0.0)["xyz"]) for f, _ in fr)
        check(c, cam, view, frames, records(None), mode=0, with_immature=False, what="immature %d switched off" % n_imm)
    c.close()


def test_seventeen_frames_with_departed_ones_and_a_dense_only_frame():
    """W = 6 windows re-issued with new frame ids three times on one archiving context: 18 frame ids, 12 of them only in the archive (chunks of 64); 17 are listed.
    Then a frame whose only records are dense ones"""
    sizes = [40, 1, 65, 64, 63, 129]
    S = tmg.planted_scene(sizes)
    A = tmg.make_ctx(S)
    A.map_enable(chunk_points=64)
    win = S["win"]
    c2w = [synth.se3_inv(win.world_to_cam[i]) for i in range(6)]
    recs, frames = {}, []
    for rnd in range(3):
        S = dict(S, fids=[100 + 10 * rnd + i for i in range(6)])
        tmg.issue(A, S)
        A.ba_set_point_history(*tmg.plant(S, sizes, 30 + rnd))
        A.ba_linearize(False)
        k = tmg.keyframe(A, S, np.zeros(6, np.uint8))
        for i, f in enumerate(S["fids"]):
            shift = np.concatenate([c2w[i][:, :3], c2w[i][:, 3:] + [[0.4 * rnd], [0], [0]]], 1)
            frames.append((f, shift))
            recs[f] = tmg.frame_records(S, k, f, i, None) if rnd == 2 else mm.set_from_kf(None, None, *k["exp"][f])
    view = rm.look_at((0.5, -1.5, -4.0), (0, 0, 3.0), (0, -1, 0))
    cam = rm.make_cam(96, 72, fx=60, fy=60)
    g = check(A, cam, view, frames[1:], recs, mode=0, what="17 frames", show_kf_cams=True)
    assert len(frames[1:]) == 17 and g["n_drawn_points"] > 2000
    check(A, cam, view, frames[3:5], recs, mode=1, what="2 departed frames")
    A.close()
    # dense: tests/test_dense_map_gpu.py's planted scene; its frame FID then leaves the window (a new window with other ids): dense records only
    w, h = 80, 48
    regions = [dict(value=float(10 + 3 * dy + dx), sel=tdm.rect_sel(w, h, 3 + 16 * dy, 3 + 16 * dy + 9 + dx, 3 + 25 * dx, 3 + 25 * dx + 19 + dy), n=12 + 3 * dy + dx,
                    kind="wall", par=2.0 + 0.1 * dx) for dy in range(3) for dx in range(3)]
    scn = tdm.scene(w, h, tdm.small_K(w, h), regions, seed=2, background=1.0)
    D = tdm.context(scn, chunk=64)
    _, _, napp = D.dense_update_map(0, pm.make_draws(2), tdm.C2W)
    pts = D.map_dense_get(tdm.FID)
    assert napp == len(pts) > 50
    P = len(scn["u"])
    SD = dict(host=np.zeros(P, np.int32), u=scn["u"], v=scn["v"], color=np.full((P, 8), 100, f32), hp=np.zeros(P, np.int32))
    camd = rm.make_cam(64, 48, fx=40, fy=40)
    viewd = rm.look_at((0.2, -0.5, -1.0), (0, 0, 2.0), (0, -1, 0))
    fr = [(tdm.FID, EYE), (tdm.FID + 1, EYE)]
    recd = {tdm.FID: mm.set_from_kf(None, active_records(D, SD, 0)), tdm.FID + 1: mm.set_from_kf(None, None)}
    both = check(D, camd, viewd, fr, recd, dense={tdm.FID: pts}, mode=1, literal=True, what="sparse against dense")
    only_sparse = check(D, camd, viewd, fr, recd, mode=1, what="sparse alone")
    assert both["n_vertices"] == only_sparse["n_vertices"] + int((~(pts["idepth"] < 0)).sum()) and both["n_drawn_points"] > only_sparse["n_drawn_points"] > 0
    only_dense = check(D, camd, viewd, fr, recd, dense={tdm.FID: pts}, mode=3, what="dense alone")            # display_mode 3 draws no sparse record
    shared = np.isfinite(only_sparse["depth"]) & np.isfinite(only_dense["depth"])
    print("RENDER sparse against dense: %d shared pixels, dense nearer on %d" % (shared.sum(), (only_dense["depth"][shared] < only_sparse["depth"][shared]).sum()))
    assert shared.sum() >= 10                                                                    # pixels with a candidate of either kind
    assert np.array_equal(both["depth"][shared], np.minimum(only_sparse["depth"][shared], only_dense["depth"][shared]))
    D.ba_set_window([0, 1], np.tile(EYE, (2, 1, 1)), frame_ids=[700, 701])
    D.ba_set_points(SD["host"], SD["u"], SD["v"], scn["idp"], SD["color"], np.ones((P, 8), f32))
    g = check(D, camd, viewd, [(tdm.FID, EYE)], {}, dense={tdm.FID: pts}, mode=1, what="dense records only")
    assert g["n_vertices"] == int((~(pts["idepth"] < 0)).sum()) and g["n_drawn_points"] > 100
    g = check(D, camd, viewd, [(tdm.FID, EYE)], {}, mode=1, what="dense-only frame without with_dense")
    assert g["n_vertices"] == 0
    D.close()


# ------------------------------------------------------------------------------------------------ 6: the plane cleans itself
def test_plane_cleans_itself(small):
    A, frames, recs = small["A"], small["frames"], small["recs"]
    v2 = rm.look_at((-1.0, -0.5, -3.0), (0, 0, 3.0), (0, -1, 0))
    cur = np.concatenate([np.eye(3), [[-0.6], [-0.3], [1.0]]], 1)
    for cam, view in ((small["cam"], small["view"]), (small["cam"], v2), (rm.make_cam(200, 150, fx=120, fy=120), v2), (rm.make_cam(31, 17, fx=20, fy=20), small["view"]),
                      (rm.make_cam(200, 150, fx=120, fy=120), small["view"])):
        check(A, cam, view, frames, recs, mode=0, what="size %dx%d" % (cam["vw"], cam["vh"]), current_cam=cur)


# ------------------------------------------------------------------------------------------------ 7, 8: the device chain
def chain(w, h, WW, KF, P, n_imm, twin=False):
    """tests/test_dense_map_gpu.py's chain (flag -> marginalize_flagged -> marginalize_frame -> carry_window, nalo_dense_update_map each keyframe) with the graph on;
    stops after the last keyframe's marginalize_flagged, the window's points standing. -> contexts, frames, recs, dense, connections"""
    s = 3e-4
    win = synth.make_window(w=w, h=h, W=WW, P=P, seed=sc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    nF = WW + KF
    srng = np.random.RandomState(sc.SEED + 3)
    st6 = np.zeros((nF, 6))
    st6[1:, :3] = 0.004 * srng.randn(nF - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * srng.randn(nF - 1, 3)
    mask = pc.block_mask(w, h, 2, 1, [2.0, 0.0])                                                # tests/test_dense_map_gpu.py's band_mask at any size: the near ground in two values
    mask[2 * h // 3:, :w // 2] = 6.0
    mask[2 * h // 3:, w // 2:] = 8.0
    bgr = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    ctxs = [binding.Context(w, h, win.K, n_slots=nF) for _ in range(2 if twin else 1)]
    fids = [200 + i for i in range(WW)]
    imm = tmg.immature_set(n_imm, WW, w, h)
    for c in ctxs:
        for i in range(nF):
            c.frame_upload(i, win.images[i], mask=mask, bgr=bgr)
        c.ba_set_prior_carry(True)
        c.map_graph_enable()
        c.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=st6[:WW], frame_ids=fids)
        c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
        c.ba_set_residuals(win.exists)
        ng0, lt0, ls0 = lm.default_history(win.exists)
        ls0[win.host == WW - 1, 0] = lm.IN
        c.ba_set_point_history(ng0, lt0, ls0)
        c.map_enable()
        c.map_dense_enable(True, 4096)
    S = dict(host=win.host.copy(), u=win.u, v=win.v, color=win.color, hp=np.zeros(len(win.host), np.int32), fids=fids)
    c2w = {200 + i: synth.se3_inv(win.world_to_cam[i]) for i in range(nF)}
    seen, k = list(fids), None
    for kf in range(KF):
        for c in ctxs:
            if kf:
                c.ba_marginalize_frame(0)
                c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
        if kf:
            m = ctxs[0].ba_carry_map()
            S = dict(host=S["host"][m] - 1, u=S["u"][m], v=S["v"][m], color=S["color"][m], hp=S["hp"][m], fids=S["fids"][1:] + [200 + WW - 1 + kf])
            seen.append(200 + WW - 1 + kf)
        ff = np.zeros(WW, np.uint8); ff[0] = 1
        for c in ctxs:
            c.ba_linearize(False)
            c.ba_linearize(True)
            c.dense_update_map(WW - 3, pm.make_draws(60 + kf), synth.se3_inv(win.world_to_cam[WW - 3 + kf]))
        for c in ctxs[1:]:
            c.ba_flag_points(ff)
            c.ba_marginalize_flagged()
        k = tmg.keyframe(ctxs[0], S, ff)
    A = ctxs[0]
    A.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
    for c in ctxs[1:]:
        c.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
    frames = [(f, c2w[f]) for f in seen]
    recs, dense = {}, {}
    for f in seen:
        widx = S["fids"].index(f) if f in S["fids"] else -1
        if widx >= 0:                                                                            # the last keyframe's lists hold only what IT removed: the archive classes come from the read-back
            live = tmg.frame_records(S, k, f, widx, imm)
            recs[f] = np.concatenate([live[live["status"] <= 1], mm.set_from_kf(None, None, *archive_records(A, f))])
        else:
            recs[f] = mm.set_from_kf(None, None, *archive_records(A, f))
        try:
            dense[f] = A.map_dense_get(f)
        except binding.NaloError:
            pass
    return ctxs, win, frames, recs, dense, A.map_graph_connections()


def test_three_keyframes_at_1224x368_everything_on():
    (A,), win, frames, recs, dense, conn = chain(1224, 368, 8, 3, 8000, 6000)
    assert len(frames) == 10 and len(dense) == 3 and sum(len(d) for d in dense.values()) > 1000
    # the corridor's cameras are 3e-4 apart: the viewer's poses are the chain's, scaled up so that frusta and constraints are more than a pixel
    frames = [(f, np.concatenate([m[:, :3], m[:, 3:] * 2000], 1)) for f, m in frames]
    view = rm.look_at((1.0, -3.0, -8.0), (0, 0, 4.0), (0, -1, 0))
    cam = rm.make_cam(640, 480)
    poses = np.stack([m[:, 3] for _, m in frames]).astype(f32) + f32([0, 0.2, 0])
    kw = dict(show_kf_cams=True, current_cam=frames[-1][1], connections=conn, show_active=True, show_all=True, show_trajectory=True, all_poses=poses)
    g = check(A, cam, view, frames, recs, dense=dense, mode=1, what="chain", **kw)
    print("RENDER chain 1224x368: vertices %d drawn %d segments %d samples %d" % (g["n_vertices"], g["n_drawn_points"], g["n_segments"], g["n_line_samples"]))
    assert g["n_vertices"] > 50000 and g["n_drawn_points"] > 10000 and g["n_line_samples"] > 200
    again = call(A, cam, view, frames, 1, with_dense=True, **kw)
    assert rm.same(again, g) == [] and again["rgb"].tobytes() == g["rgb"].tobytes() and again["depth"].tobytes() == g["depth"].tobytes()
    check(A, cam, view, frames, recs, dense=dense, mode=0, what="chain mode 0", **kw)
    A.close()


def test_no_side_effects():
    (A, B), win, frames, recs, dense, conn = chain(320, 240, 5, 2, 1500, 300, twin=True)
    view = rm.look_at((0.5, -1.5, -4.0), (0, 0, 3.0), (0, -1, 0))
    cam = rm.make_cam(96, 72, fx=60, fy=60)
    for mode in (0, 1):
        check(A, cam, view, frames, recs, dense=dense, mode=mode, what="twin", show_kf_cams=True, connections=conn, show_active=True, show_all=True, show_trajectory=True)
    for f, _ in frames:
        assert mm.records_equal(A.map_get_frame(f), B.map_get_frame(f)), f
    pa, pb = A.ba_get_points(), B.ba_get_points()
    assert all(mm.bits_equal(pa[q], pb[q]) for q in pa)
    assert all(mm.bits_equal(np.ascontiguousarray(a), np.ascontiguousarray(b)) for a, b in zip(A.imm_resident_get(), B.imm_resident_get()))
    assert A.map_graph_connections().tobytes() == B.map_graph_connections().tobytes()
    ra, rb = A.ba_optimize(2), B.ba_optimize(2)
    assert np.float64(ra).tobytes() == np.float64(rb).tobytes()
    pa, pb = A.ba_get_points(), B.ba_get_points()
    assert all(mm.bits_equal(pa[q], pb[q]) for q in pa)
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals(small):
    A, frames, view, cam = small["A"], small["frames"], small["view"], small["cam"]
    good = call(A, cam, view, frames, mode=1)

    def refused(code, what, frames_=frames, with_dense=False, patch=None, **kw):
        a, keep = A.map_render_args(cam["vw"], cam["vh"], view, frames_, with_dense=with_dense, **dict(cam_kw(cam), **kw))
        rgb, depth = np.full((cam["vh"], cam["vw"], 3), 0xA5, np.uint8), np.full((cam["vh"], cam["vw"]), -7.0, f32)
        a.rgb, a.depth = rgb.ctypes.data_as(binding.c_u8p), depth.ctypes.data_as(binding.c_fp)
        if patch:
            patch(a)
        assert A.L.nalo_map_render(A.h_, C.byref(a)) == code, what
        assert (rgb == 0xA5).all() and (depth == -7.0).all(), what
        assert rm.same(call(A, cam, view, frames, mode=1), good) == [], what                     # the next legal call succeeds and paints the same picture

    def setattrs(**kv):
        return lambda a: [setattr(a, k, v) for k, v in kv.items()]

    refused(ERR_ARG, "vw 0", patch=setattrs(vw=0))
    refused(ERR_ARG, "vh negative", patch=setattrs(vh=-1))
    refused(ERR_ARG, "vw * vh above 2^26", patch=setattrs(vw=1 << 14, vh=(1 << 12) + 1))
    for key in ("fx", "fy", "cx", "cy", "znear", "zfar"):
        refused(ERR_ARG, key + " NaN", **{key: float("nan")})
    refused(ERR_ARG, "fx inf", fx=float("inf"))
    refused(ERR_ARG, "znear 0", znear=0.0)
    refused(ERR_ARG, "znear negative", znear=-1.0)
    refused(ERR_ARG, "zfar == znear", znear=2.0, zfar=2.0)
    refused(ERR_ARG, "n_frames negative", patch=setattrs(n_frames=-1))
    refused(ERR_ARG, "frames NULL", patch=setattrs(frames=None))
    refused(ERR_ARG, "all_poses NULL", patch=setattrs(n_all_poses=3))
    refused(ERR_ARG, "listed twice", frames_=frames + frames[:1])
    refused(ERR_ARG, "unknown frame_id", frames_=frames + [(7, EYE)])
    refused(ERR_ARG, "sparsity 2", sparsity=2)
    refused(ERR_STATE, "dense archive off", with_dense=True)
    A.map_graph_enable(False)
    refused(ERR_STATE, "graph off", show_active_constraints=True)
    refused(ERR_STATE, "graph off (all)", show_all_constraints=True)
    A.map_graph_enable(True)
    a, keep = A.map_render_args(cam["vw"], cam["vh"], view, frames, **cam_kw(cam))
    assert A.L.nalo_map_render(A.h_, C.byref(a)) == ERR_ARG and A.L.nalo_map_render(A.h_, None) == ERR_ARG and A.L.nalo_map_render(None, C.byref(a)) == ERR_ARG       # rgb NULL, args NULL, ctx NULL
    # n_frames == 0 is legal: the background
    g = call(A, cam, view, [])
    assert (g["rgb"] == np.array(GREY, np.uint8)).all() and np.isinf(g["depth"]).all() and g["n_vertices"] == 0
    g = A.map_render(cam["vw"], cam["vh"], view, frames, want_depth=False, display_mode=1, background=GREY, **cam_kw(cam))       # depth is optional
    assert g["depth"] is None and np.array_equal(g["rgb"], good["rgb"])


def test_refusals_of_window_states():
    S = tmg.scene(640, 480, 4, 400)
    view, cam = START, rm.make_cam(64, 48)
    frames = [(100 + i, synth.se3_inv(S["win"].world_to_cam[i])) for i in range(4)]

    def refused(c, code, what, fr=frames):
        a, keep = c.map_render_args(64, 48, view, fr)
        rgb, depth = np.full((48, 64, 3), 0xA5, np.uint8), np.full((48, 64), -7.0, f32)
        a.rgb, a.depth = rgb.ctypes.data_as(binding.c_u8p), depth.ctypes.data_as(binding.c_fp)
        assert c.L.nalo_map_render(c.h_, C.byref(a)) == code, what
        assert (rgb == 0xA5).all() and (depth == -7.0).all(), what

    # no window
    c = binding.Context(640, 480, S["win"].K, n_slots=4)
    refused(c, ERR_STATE, "no window", fr=[])
    for i in range(4):
        c.frame_upload(i, S["win"].images[i])
    tmg.issue(c, S)
    assert call(c, cam, view, frames)["n_vertices"] > 0                                          # with a window the next call is legal
    c.close()
    # between nalo_ba_marginalize_frame and the carry
    c = tmg.make_ctx(S, n_slots=5)
    c.ba_set_prior_carry(True)
    c.map_enable()
    c.ba_set_point_history(*sc.plant_history(400, 4))
    c.ba_linearize(False)
    c.ba_linearize(True)
    c.ba_flag_points(sc.flag_sets(4)[1])
    c.ba_marginalize_flagged()
    ok = call(c, cam, view, frames)
    c.ba_marginalize_frame(1)
    refused(c, ERR_STATE, "window points unset")
    assert call(c, cam, view, [])["n_vertices"] == 0                                             # a call that lists no window frame is legal in that state
    g = call(c, cam, view, [frames[1]])                                                          # the departed frame alone is legal: its archive classes
    assert g["n_vertices"] == len(c.map_frame_cloud(101, 0, BIG, BIG, 0.0)["xyz"]) > 0
    c.close()
    # a sharded window
    c = tmg.make_ctx(S)
    before = call(c, cam, view, frames)
    assert rm.same(before, call(c, cam, view, frames)) == []
    c.ba_set_allreduce(lambda ptr, n: None)
    refused(c, ERR_STATE, "sharded")
    assert b"sharded" in c.L.nalo_last_error(c.h_)
    c.ba_set_allreduce(None)
    assert rm.same(call(c, cam, view, frames), before) == []                                     # unsharded again: the picture of before
    # a context whose cross-rank exchange failed (the hook is cleared: this is not the sharded refusal). The state is final for the context - every later
    # call of it fails, as nalo_ba_exchange_failed documents -, so the next legal call is one on another context
    c.ba_exchange_failed("link down (map render test)")
    refused(c, ERR_STATE, "exchange failed")
    assert b"cross-rank" in c.L.nalo_last_error(c.h_)
    refused(c, ERR_STATE, "exchange failed, no frames", fr=[])
    c.close()
    c = tmg.make_ctx(S)
    assert rm.same(call(c, cam, view, frames), before) == []
    c.close()
    assert ok["n_vertices"] > 0
