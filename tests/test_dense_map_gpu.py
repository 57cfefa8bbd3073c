"""nalo_dense_update_map and the dense archive (nalo_map_dense_*) on the device.

Two yardsticks, neither of them the code under test: tests/dense_map_model.py (the oracle's orc_dense_bbox / orc_dense_make_map per cluster of tests/plane_model.py,
appended under the accept bit; the literal refreshPC and SampleOutputWrapper loops) and a SECOND CONTEXT that takes the existing route (nalo_dense_fit_planes, the
loop of nalo_dense_make_map, appending on the host under accept).

Against the second context everything is equal bit for bit. Against the oracle rects, counts, u, v, colour, bgr and accept bits are equal and idepth stays within
tests/test_dense_gpu.py's rtol = 2e-6, atol = 2e-7 (the same arithmetic with the same horizon-row cancellation); the oracle's makeMap runs on the plane the device
reports, because the fit has its own tests and its own bound (tests/test_plane_fit_gpu.py), while cluster order, mask values and fitted bits are the model's own.
accept of a cluster that kept nothing is 0 here (nothing to append); nalo_dense_make_map and the oracle report the extent test on the untouched seeds there, so
the comparison takes accept only where n > 0.

NOT reachable through makeMap, so not planted on the device: a NaN, +inf or denormal idepth. makeMap's idepth is 1 / (-p3 / ddepth) of a finite plane with
ddepth != 0 and depth != 0: a NaN needs a non-finite plane, +inf a depth below 1.2e-38 (|p3| that small), a denormal a depth above 8.5e37. The negative ones
(a plane whose horizon row crosses its box) are planted; the literal cloud model takes all of them on the CPU (tests/test_dense_map_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import dense_map_model as dm
import map_model as mm
import plane_cases as pc
import plane_model as pm
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4
FID = 500


# ------------------------------------------------------------------------------------------------ scenes
def ray(K, x, y):
    fxi, cxi, fyi, cyi = [float(t) for t in pm.ki(K)]
    return fxi * np.asarray(x, np.float64) + cxi, fyi * np.asarray(y, np.float64) + cyi


def scene(w, h, K, regions, seed=0, background=0.0):
    """regions: dicts(value, sel (bool [h][w]), n, kind = "ground" (Y = par) | "wall" (Z = par) | "id" (idepth = par)). The points of a region lie on pixels of
    the region inside the clustering border, on its plane +- 1 mm. -> dict(mask, img, bgr, u, v, idp, ...)"""
    rng = np.random.RandomState(seed)
    mask = np.full((h, w), background, F)
    for r in regions:
        mask[r["sel"]] = r["value"]
    us, vs, ids = [], [], []
    inner = np.zeros((h, w), bool)
    inner[3:h - 2, 3:w - 2] = True
    for r in regions:
        if not r.get("n"):
            continue
        sel = r["sel"] & inner
        if r["kind"] == "ground":
            sel = sel & (ray(K, np.zeros(w), np.arange(h))[1] > 0.02)[:, None]
        ys, xs = np.nonzero(sel)
        pick = rng.choice(len(xs), r["n"], replace=len(xs) < r["n"])
        x, y = xs[pick], ys[pick]
        rx, ry = ray(K, x, y)
        if r["kind"] == "ground":
            Z = (r["par"] + rng.uniform(-0.001, 0.001, len(x))) / ry
        elif r["kind"] == "wall":
            Z = r["par"] + rng.uniform(-0.001, 0.001, len(x))
        else:
            with np.errstate(divide="ignore"):
                Z = 1.0 / np.full(len(x), float(r["par"]))
        us.append(x + 0.25); vs.append(y + 0.5); ids.append(1.0 / Z)
    u, v, idp = [np.concatenate(a).astype(F) for a in (us, vs, ids)]
    perm = rng.permutation(len(u))
    return dict(w=w, h=h, K=K, mask=mask, img=rng.uniform(5, 250, (h, w)).astype(F), bgr=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), u=u[perm], v=v[perm], idp=idp[perm])


def rect_sel(w, h, y0, y1, x0, x1):
    s = np.zeros((h, w), bool)
    s[y0:y1, x0:x1] = True
    return s


def context(sc, chunk=4096, enable=True, n_slots=2):
    """a W = 2 window on the slots 0, 1; every point of the scene is hosted by frame 0 (frame_id FID)"""
    c = binding.Context(sc["w"], sc["h"], sc["K"], n_slots=n_slots)
    c.frame_upload(0, sc["img"], mask=sc["mask"], bgr=sc["bgr"])
    c.frame_upload(1, sc["img"], mask=sc["mask"], bgr=sc["bgr"])
    P = len(sc["u"])
    c.ba_set_window([0, 1], np.tile(np.eye(3, 4), (2, 1, 1)), frame_ids=[FID, FID + 1])
    c.ba_set_points(np.zeros(P, np.int32), sc["u"], sc["v"], sc["idp"], np.full((P, 8), 100, F), np.ones((P, 8), F))
    if enable:
        c.map_dense_enable(True, chunk)
    return c


C2W = np.concatenate([np.eye(3), np.array([[0.5], [0.1], [2.0]])], 1)


def route_b(c, hf, slot, draws, c2w, w, h, **kw):
    """today's route: fit, then nalo_dense_make_map per fitted cluster with its read-backs; append on the host under accept"""
    recs, _ = c.dense_fit_planes(hf, draws, **kw)
    runs = np.zeros(len(recs), binding.DENSE_RUN_DTYPE)
    runs["first"] = -1
    app, total = [], 0
    for k, r in enumerate(recs):
        if not r["fitted"]:
            continue
        d = c.dense_make_map(slot, r["plane"], float(r["mask_value"]), c2w, cap=w * h)
        runs[k]["rect"] = d["rect"]
        if r["mask_value"] == 0:
            continue
        runs[k]["n"] = d["n"]
        runs[k]["accept"] = d["accept"] if d["n"] > 0 else 0
        if d["n"] > 0 and d["accept"]:
            runs[k]["first"] = total
            total += d["n"]
            app.append(d)
    pts = np.zeros(total, binding.DENSE_POINT_DTYPE)
    if app:
        for key in ("u", "v", "idepth", "color", "bgr"):
            pts[key] = np.concatenate([a[key] for a in app])
    return recs, runs, pts


def points_equal(a, b):
    return len(a) == len(b) and all(mm.bits_equal(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])) for k in ("u", "v", "idepth", "color", "bgr")) and not a["pad"].any()


def run_both(sc, draws, c2w=C2W, hf=0, **kw):
    """-> the one-call route's (recs, runs, n_appended, points) after it was held equal to the second context's"""
    A, B = context(sc), context(sc, enable=False)
    recs, runs, napp = A.dense_update_map(hf, draws, c2w, **kw)
    pts = A.map_dense_get(FID)
    rb, runs_b, pts_b = route_b(B, hf, 0, draws, c2w, sc["w"], sc["h"], **kw)
    assert recs.tobytes() == rb.tobytes()
    assert runs.tobytes() == runs_b.tobytes(), (runs, runs_b)
    assert napp == len(pts) == len(pts_b) and points_equal(pts, pts_b)
    assert A.map_dense_counts(FID) == (napp, int((runs["first"] >= 0).sum()))
    A.close(); B.close()
    return recs, runs, napp, pts


def against_model(sc, draws, recs, runs, pts, c2w=C2W, **kw):
    m = dm.update_map(sc["u"], sc["v"], sc["idp"], sc["mask"], sc["img"], sc["bgr"], sc["w"], sc["h"], sc["K"], draws, c2w, planes=recs["plane"], **kw)
    assert len(m["clusters"]) == len(recs)
    for k, (c, r) in enumerate(zip(m["clusters"], m["runs"])):
        assert recs[k]["mask_value"] == c["mask_value"] and recs[k]["fitted"] == c["fitted"], k
        assert list(runs[k]["rect"]) == r["rect"] and runs[k]["n"] == r["n"] and runs[k]["first"] == r["first"], (k, runs[k], r)
        if r["n"] > 0:
            assert runs[k]["accept"] == r["accept"], k
        else:
            assert runs[k]["accept"] == 0
    mp = m["points"]
    assert len(pts) == len(mp["u"])
    assert np.array_equal(pts["u"], mp["u"]) and np.array_equal(pts["v"], mp["v"]) and np.array_equal(pts["color"], mp["color"]) and np.array_equal(pts["bgr"], mp["bgr"])
    err = np.abs(pts["idepth"].astype(np.float64) - mp["idepth"])
    if len(err):
        print("DENSE MAP idepth against the oracle: max abs %.3g, max rel %.3g over %d points" % (err.max(), (err / np.maximum(np.abs(mp["idepth"]), 1e-30)).max(), len(err)))
    assert np.allclose(pts["idepth"], mp["idepth"], rtol=2e-6, atol=2e-7)
    return m


def small_K(w, h):
    return (40.0 * w / 64, 40.0 * w / 64, (w - 1) / 2.0, (h - 1) / 2.0)


# ------------------------------------------------------------------------------------------------ route equality and the oracle
@pytest.mark.parametrize("w,h", [(64, 48), (80, 48)])
def test_planted_masks_small(w, h):
    """checkerboard of two values (boxes overlap completely), interleaved stripes, a value 0, a -0.0 patch that alone carries the box of value 0 to the right
    border (a band of another value lies between it and the +0 pixels), a NaN patch, a one-column and a one-row (empty) box"""
    K = small_K(w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    left = xx < w // 2
    regions = [dict(value=3.0, sel=left & (((xx // 4) + (yy // 4)) % 2 == 0), n=40, kind="wall", par=2.0),
               dict(value=4.0, sel=left & (((xx // 4) + (yy // 4)) % 2 == 1), n=30, kind="wall", par=3.0),
               dict(value=6.0, sel=~left & (yy < 30) & (yy % 4 < 2), n=25, kind="wall", par=2.5),
               dict(value=7.0, sel=~left & (yy < 30) & (yy % 4 >= 2), n=20, kind="wall", par=4.0),
               dict(value=0.0, sel=~left & (yy >= 30) & (xx < w - 12), n=15, kind="wall", par=2.0),
               dict(value=5.0, sel=~left & (yy >= 30) & (xx >= w - 12), n=0),
               dict(value=-0.0, sel=rect_sel(w, h, 40, 46, w - 8, w - 2), n=0),
               dict(value=np.nan, sel=rect_sel(w, h, 31, 36, w // 2 + 2, w // 2 + 8), n=0),
               dict(value=8.0, sel=rect_sel(w, h, 36, 46, w // 2 + 10, w // 2 + 11), n=12, kind="wall", par=2.0),       # one column: rx1 == rx0
               dict(value=9.0, sel=rect_sel(w, h, 38, 39, w // 2 + 13, w // 2 + 25), n=11, kind="wall", par=2.0)]      # one row
    sc = scene(w, h, K, regions, seed=w)
    draws = pm.make_draws(w)
    recs, runs, napp, pts = run_both(sc, draws)
    m = against_model(sc, draws, recs, runs, pts)
    by = {float(c["mask_value"]): k for k, c in enumerate(m["clusters"])}
    assert set(by) == {3.0, 4.0, 6.0, 7.0, 0.0, 8.0, 9.0} and recs["fitted"].all()
    r3, r4, r6, r7 = (m["runs"][by[v]]["rect"] for v in (3.0, 4.0, 6.0, 7.0))
    assert max(r3[0], r4[0]) < min(r3[1], r4[1]) - 20 and max(r3[2], r4[2]) < min(r3[3], r4[3]) - 20 and max(r6[2], r7[2]) < min(r6[3], r7[3]) - 20     # the boxes overlap
    r0 = m["runs"][by[0.0]]
    without = sc["mask"].copy()
    without[np.signbit(without) & (without == 0)] = 5.0
    assert np.signbit(sc["mask"]).sum() == 36 and dm.bbox(without, w, h, 0.0)[1] == w - 13                     # without the -0.0 patch the box of value 0 ends at the band
    assert r0["n"] == 0 and r0["rect"][1] == w - 3 and list(runs[by[0.0]]["rect"]) == r0["rect"] and not np.signbit(recs[by[0.0]]["mask_value"])   # -0.0 pixels belong to it
    r8, r9 = m["runs"][by[8.0]], m["runs"][by[9.0]]
    assert r8["rect"][0] == r8["rect"][1] and r8["n"] == 0 and r9["rect"][2] == r9["rect"][3] and r9["n"] == 0
    assert napp > 200 and all(m["runs"][by[v]]["accept"] and m["runs"][by[v]]["n"] > 30 for v in (3.0, 4.0, 6.0, 7.0))


def test_every_phase_of_the_box_origin():
    w, h = 80, 48
    regions = [dict(value=float(10 + 3 * dy + dx), sel=rect_sel(w, h, 3 + 16 * dy, 3 + 16 * dy + 9 + dx, 3 + 25 * dx, 3 + 25 * dx + 19 + dy), n=12 + 3 * dy + dx,
                    kind="wall", par=2.0 + 0.1 * dx) for dy in range(3) for dx in range(3)]
    sc = scene(w, h, small_K(w, h), regions, seed=2, background=1.0)
    draws = pm.make_draws(2)
    recs, runs, napp, pts = run_both(sc, draws)
    m = against_model(sc, draws, recs, runs, pts)
    fitted = [r for c, r in zip(m["clusters"], m["runs"]) if c["mask_value"] >= 10]
    assert {(r["rect"][0] % 3, r["rect"][2] % 3) for r in fitted} == {(a, b) for a in range(3) for b in range(3)} and all(r["n"] > 0 for r in fitted)


@pytest.fixture(scope="module")
def qvga():
    """320x240, one frame with the planted cases that need room:
       20  5 chunks of 1024 candidates (a box of 150 x 62), accepted
       21  a box full of candidates of which none is its own pixel (dots at i % 3 == 1, j % 3 == 1): zero kept points between two clusters with many
       22  many points but fewer than min_points of them with a finite back-projection (idepth = 0): not fitted, between fitted ones
       23  a wall at 100 m, 100 px wide at fx = 200: rejected, between accepted ones
       24  a plane Y = 0.3 whose horizon row crosses its box (the cluster's own pixels lie above and below it): negative idepths above it, accepted
       25  a wall 32 m high seen by a camera turned upside down: world y decreases along the raster
       26  a plane through the camera centre from points on the row v = cy: p3 = +-0, every depth is 0 and skipped, and ddepth == 0 on the row itself"""
    w, h = 320, 240
    K = (256.0, 256.0, 160.0, 120.0)
    yy, xx = np.mgrid[0:h, 0:w]
    regions = [dict(value=20.0, sel=rect_sel(w, h, 5, 68, 5, 156), n=90, kind="wall", par=3.0),
               dict(value=21.0, sel=rect_sel(w, h, 5, 60, 165, 230) & (yy % 3 == 1) & (xx % 3 == 1), n=80, kind="wall", par=3.0),
               dict(value=22.0, sel=rect_sel(w, h, 5, 40, 240, 300), n=70, kind="id", par=0.0),
               dict(value=23.0, sel=rect_sel(w, h, 75, 110, 5, 110), n=60, kind="wall", par=100.0),
               dict(value=24.0, sel=rect_sel(w, h, 100, 160, 120, 200) & ((yy < 111) | (yy >= 135)), n=50, kind="ground", par=0.3),
               dict(value=25.0, sel=rect_sel(w, h, 70, 236, 240, 300), n=40, kind="wall", par=50.0),
               dict(value=27.0, sel=rect_sel(w, h, 205, 236, 10, 200), n=30, kind="ground", par=1.6)]
    sc = scene(w, h, K, regions, seed=9, background=1.0)
    # value 22: five points with a depth, the rest with idepth 0; value 26: a patch across the row v = cy with its eleven points on that row
    n22 = np.nonzero(sc["mask"][sc["v"].astype(int), sc["u"].astype(int)] == 22.0)[0]
    sc["idp"][n22[:5]] = 0.4
    sc["mask"][118:123, 210:236] = 26.0
    u26 = np.arange(212, 234, 2).astype(F) + F(0.25)
    sc["u"] = np.concatenate([sc["u"], u26]); sc["v"] = np.concatenate([sc["v"], np.full(len(u26), 120.0, F)])
    sc["idp"] = np.concatenate([sc["idp"], np.linspace(0.2, 0.9, len(u26)).astype(F)])
    # upside down, slightly rolled: world y = -cam y + a little x
    a = 0.01
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.diag([1.0, -1.0, -1.0])
    c2w = np.concatenate([R, np.array([[0.5], [0.1], [2.0]])], 1)
    draws = pm.make_draws(9)
    kw = dict(threshold=0.0)                                       # no inlier ever: the winning SAMPLE is the plane, so value 26's plane is exactly (0, +-1, 0, +-0)
    recs, runs, napp, pts = run_both(sc, draws, c2w=c2w, **kw)
    return dict(sc=sc, draws=draws, c2w=c2w, kw=kw, recs=recs, runs=runs, napp=napp, pts=pts)


def quirk_extent(p, K, c2w):
    """the serial loop of :382-401 on the model's points -> (accept by the loop as written, world y extent as it would be with the typo fixed)"""
    fxi, cxi, fyi, cyi = [float(F(t)) for t in pm.ki(K)]
    m = np.asarray(c2w, np.float64)
    miny, maxy, true_max = np.inf, np.finfo(F).tiny, -np.inf
    last_q = None
    for j, i, idp in zip(p["u"], p["v"], p["idepth"].astype(np.float64)):
        cP = np.array([(fxi * j + cxi) / idp, (fyi * i + cyi) / idp, 1.0 / idp])
        y = m[1, :3] @ cP + m[1, 3]
        if y < miny:
            miny = float(F(y))
        if y > miny:
            maxy = float(F(y)); last_q = y
        true_max = max(true_max, y)
    return maxy - miny, true_max - miny


def test_planted_cases_320(qvga):
    sc, recs, runs, pts = qvga["sc"], qvga["recs"], qvga["runs"], qvga["pts"]
    m = against_model(sc, qvga["draws"], recs, runs, pts, c2w=qvga["c2w"], **qvga["kw"])
    by = {float(c["mask_value"]): k for k, c in enumerate(m["clusters"])}
    R = lambda v: m["runs"][by[v]]
    order = [float(c["mask_value"]) for c in m["clusters"]]
    print("DENSE MAP planted 320x240: order %s, n %s, accept %s" % (order, [r["n"] for r in m["runs"]], [r["accept"] for r in m["runs"]]))
    assert R(20.0)["n"] > 4 * 1024 and R(20.0)["accept"] == 1 and by[20.0] == 0             # five chunks; the next cluster's workgroups start behind them
    k21 = by[21.0]
    assert R(21.0)["n"] == 0 and m["clusters"][k21]["fitted"] and (R(21.0)["rect"][1] - R(21.0)["rect"][0]) * (R(21.0)["rect"][3] - R(21.0)["rect"][2]) > 3000
    assert any(m["runs"][j]["n"] > 500 for j in range(k21)) and any(m["runs"][j]["n"] > 500 for j in range(k21 + 1, len(order)))
    k22 = by[22.0]
    assert not m["clusters"][k22]["fitted"] and m["clusters"][k22]["n"] >= 60 and R(22.0)["rect"] == [0, 0, 0, 0]
    assert any(c["fitted"] for c in m["clusters"][:k22]) and any(c["fitted"] for c in m["clusters"][k22 + 1:])
    k23 = by[23.0]
    assert R(23.0)["n"] > 1000 and R(23.0)["accept"] == 0
    assert any(r["accept"] and r["n"] for r in m["runs"][:k23]) and any(r["accept"] and r["n"] for r in m["runs"][k23 + 1:])       # the copy pass skips a run
    p24 = R(24.0)["pts"]
    assert (p24["idepth"] < 0).sum() > 100 and (p24["idepth"] > 0).sum() > 100 and R(24.0)["accept"] == 1 and R(24.0)["rect"][2] < 120 < R(24.0)["rect"][3]   # the horizon row crosses the box
    p25 = R(25.0)["pts"]
    ext_quirk, ext_true = quirk_extent(p25, sc["K"], qvga["c2w"])
    print("DENSE MAP App. C.6: y extent as written %.3f, with the maximum %.3f, accept %d" % (ext_quirk, ext_true, R(25.0)["accept"]))
    assert ext_true > 30 > ext_quirk and R(25.0)["accept"] == 1                               # maxy is not the maximum: the loop as written accepts
    k26 = by[26.0]
    assert m["clusters"][k26]["fitted"] and recs[k26]["plane"][3] == 0 and R(26.0)["n"] == 0 and R(26.0)["rect"][3] > R(26.0)["rect"][2]
    assert (pts["idepth"] < 0).any()


def band_mask(w, h):
    """the synthetic scene's near ground (rows >= 160) in two values, the rest in two more: the near ground is a plane within the extent test"""
    mask = pc.block_mask(w, h, 2, 1, [2.0, 0.0])
    mask[160:, :w // 2] = 6.0
    mask[160:, w // 2:] = 8.0
    return mask


def dense_variant_window(mask=None):
    """the 320x240 W = 3 window of tests/test_plane_fit_gpu.py::test_dense_variant: window points (a few marginalised away) and resident immature points"""
    w, h = 320, 240
    win = synth.make_window(w=w, h=h, W=3, P=300, seed=6)
    rng = np.random.RandomState(3)
    mask = pc.block_mask(w, h, 2, 2, [2.0, 4.0, 0.0, 6.0]) if mask is None else mask
    bgr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    gone = (np.arange(len(win.host)) % 7 == 3).astype(np.uint8)
    n_imm = 500
    rng = np.random.RandomState(3)
    iu, iv = rng.randint(0, w, n_imm).astype(F), rng.randint(0, h, n_imm).astype(F)
    ihost = rng.randint(0, win.W, n_imm).astype(np.int32)
    idmin = rng.uniform(0.05, 0.3, n_imm).astype(F)
    idmax = (idmin + rng.uniform(0, 0.3, n_imm)).astype(F)
    idmax[::17] = np.nan
    ctxs = []
    for k in range(2):
        c = binding.Context(w, h, win.K, n_slots=win.W)
        for i in range(win.W):
            c.frame_upload(i, win.images[i], mask=mask, bgr=bgr)
        c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], frame_ids=[FID + i for i in range(win.W)])
        c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
        c.ba_set_residuals(win.exists)
        c.ba_linearize(False)
        c.ba_marginalize_points(gone)
        z8, z3, z1 = np.zeros((n_imm, 8), F), np.zeros((n_imm, 3), F), np.zeros(n_imm, F)
        c.imm_resident_set(iu, iv, z8, z8 + 1, z3, z1 + 10, ihost, idmin, idmax, np.zeros(n_imm, np.int32), z1)
        ctxs.append(c)
    return win, mask, bgr, gone, (iu, iv, ihost, idmin, idmax), ctxs


def test_window_points_and_resident_immature_points():
    win, mask, bgr, gone, (iu, iv, ihost, idmin, idmax), (A, B) = dense_variant_window()
    A.map_dense_enable(True, 4096)
    w, h = win.w, win.h
    idepth = A.ba_get_points()["idepth"]
    for hf in range(win.W):
        T = synth.se3_inv(win.world_to_cam[hf])
        draws = pm.make_draws(30 + hf)
        recs, runs, napp = A.dense_update_map(hf, draws, T)
        pts = A.map_dense_get(FID + hf)
        rb, runs_b, pts_b = route_b(B, hf, hf, draws, T, w, h)
        assert recs.tobytes() == rb.tobytes() and runs.tobytes() == runs_b.tobytes() and napp == len(pts) and points_equal(pts, pts_b), hf
        wsel = np.nonzero((np.asarray(win.host) == hf) & (gone == 0))[0]
        isel = np.nonzero(ihost == hf)[0]
        sc = dict(w=w, h=h, K=win.K, mask=mask, img=win.images[hf], bgr=bgr, u=np.concatenate([np.asarray(win.u, F)[wsel], iu[isel]]),
                  v=np.concatenate([np.asarray(win.v, F)[wsel], iv[isel]]), idp=np.concatenate([np.asarray(idepth, F)[wsel], ((idmax[isel] + idmin[isel]) * F(0.5)).astype(F)]))
        against_model(sc, draws, recs, runs, pts, c2w=T)
        assert len(recs) == 4 and len(wsel) > 50 and len(isel) > 100
    A.close(); B.close()


def kitti_scene():
    """1224x368, twelve mask values in irregular regions: six on the ground (two pairs interleaved as stripes and as a checkerboard: their boxes overlap), six walls
    above the horizon, near ones and far ones (rejected)"""
    w, h = 1224, 368
    K = (718.856, 718.856, 607.19, 185.2)
    yy, xx = np.mgrid[0:h, 0:w]
    low, up = yy >= 250, yy < 170
    regions = []
    for i, (x0, x1) in enumerate([(10, 400), (410, 800), (810, 1214)]):
        band = low & (xx >= x0) & (xx < x1)
        a = band & ((xx // 7 + yy // 5) % 2 == 0) if i == 1 else band & (xx % 10 < 5 + i)
        regions += [dict(value=float(30 + 2 * i), sel=a, n=260 - 20 * i, kind="ground", par=1.65), dict(value=float(31 + 2 * i), sel=band & ~a, n=150 - 10 * i, kind="ground", par=1.65)]
    for i, Z in enumerate([6.0, 9.0, 14.0, 200.0, 300.0, 25.0]):
        ell = up & (((xx - 100 - 200 * i) / (90.0 + 8 * i)) ** 2 + ((yy - 80 - 5 * i) / (50.0 + 6 * i)) ** 2 < 1)
        regions.append(dict(value=float(40 + i), sel=ell, n=120 - 9 * i, kind="wall", par=Z))
    return scene(w, h, K, regions, seed=12, background=0.0)


def test_kitti_shape_twelve_values():
    sc = kitti_scene()
    draws = pm.make_draws(12)
    recs, runs, napp, pts = run_both(sc, draws)
    m = against_model(sc, draws, recs, runs, pts)
    vals = [float(c["mask_value"]) for c in m["clusters"]]
    print("DENSE MAP 1224x368: values %s n %s accept %s appended %d" % (vals, runs["n"].tolist(), runs["accept"].tolist(), napp))
    assert len(set(vals) - {0.0}) == 12 and napp > 30000 and 0 < (runs["accept"] == 0).sum() and (runs["first"] >= 0).sum() >= 6


# ------------------------------------------------------------------------------------------------ the archive
def test_archive_chunks_frames_and_reset(qvga):
    """chunks of 4096 points (single runs straddle their borders), two calls on one frame, three frames interleaved, nalo_map_reset. (The archive across a carry and
    a frame that leaves: test_two_keyframes_of_the_device_chain.)"""
    sc = qvga["sc"]
    P = len(sc["u"])
    A = binding.Context(sc["w"], sc["h"], sc["K"], n_slots=3)
    for i in range(3):
        A.frame_upload(i, sc["img"], mask=sc["mask"], bgr=sc["bgr"])
    A.ba_set_window([0, 1, 2], np.tile(np.eye(3, 4), (3, 1, 1)), frame_ids=[FID, FID + 1, FID + 2])
    A.ba_set_points(np.repeat(np.arange(3), P).astype(np.int32), np.tile(sc["u"], 3), np.tile(sc["v"], 3), np.tile(sc["idp"], 3), np.full((3 * P, 8), 100, F), np.ones((3 * P, 8), F))
    A.map_dense_enable(True, 4096)
    want = {hf: [] for hf in range(3)}
    n_runs = {hf: 0 for hf in range(3)}
    one, runs1 = qvga["pts"], qvga["runs"]                          # every frame holds the fixture's scene: a call's answer is the one held to both yardsticks there
    acc = int((runs1["first"] >= 0).sum())
    assert len(one) > 4096 and runs1["n"][runs1["first"] >= 0].max() > 4096               # a single run crosses a chunk border
    for rnd in range(2):
        for hf in (0, 1, 2, 1, 0, 1):
            recs, runs, napp = A.dense_update_map(hf, qvga["draws"], qvga["c2w"], **qvga["kw"])
            before = sum(len(x) for x in want[hf])
            ok = runs["first"] >= 0
            assert napp == len(one) and recs.tobytes() == qvga["recs"].tobytes()
            assert np.array_equal(runs["first"][ok], runs1["first"][ok] + before) and np.array_equal(runs["n"], runs1["n"]) and np.array_equal(runs["accept"], runs1["accept"])
            want[hf].append(one); n_runs[hf] += acc
            for g in range(3):
                if want[g]:
                    assert points_equal(A.map_dense_get(FID + g), np.concatenate(want[g])), (rnd, hf, g)
                    assert A.map_dense_counts(FID + g) == (sum(len(x) for x in want[g]), n_runs[g])
        assert len(want[1]) == 3 and A.map_dense_counts(FID + 1) == (3 * len(one), 3 * acc)
        if rnd == 0:
            A.map_reset()                                           # empties the archive; the second round reuses its chunks and gives the same answers
            for hf in range(3):
                with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
                    A.map_dense_counts(FID + hf)
            want = {hf: [] for hf in range(3)}
            n_runs = {hf: 0 for hf in range(3)}
    A.close()


# ------------------------------------------------------------------------------------------------ the consumers
def test_world_points_and_cloud(qvga):
    sc, c2w, draws = qvga["sc"], qvga["c2w"], qvga["draws"]
    A = context(sc)
    A.dense_update_map(0, draws, c2w, **qvga["kw"])
    p = A.map_dense_get(FID)
    assert points_equal(p, qvga["pts"]) and (p["idepth"] < 0).sum() > 100
    ci = mm.calib_inverse(A.ba_get_frames()[2])
    rng = np.random.RandomState(5)
    m = np.concatenate([np.linalg.qr(rng.randn(3, 3))[0], [[2.5e6 + 0.37], [-8.1e5], [42.0]]], 1)
    got = A.map_dense_world_points(FID, m)
    lib = C.CDLL(binding.lib_path())
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    io = np.zeros((len(p), 3))
    u, v, idp, mc = p["u"].astype(F), p["v"].astype(F), np.ascontiguousarray(p["idepth"]), np.ascontiguousarray(m.ravel())
    assert lib.nalo_map_world_points_host(len(p), u.ctypes.data_as(fp), v.ctypes.data_as(fp), idp.ctypes.data_as(fp), ci.ctypes.data_as(fp), mc.ctypes.data_as(dp), io.ctypes.data_as(dp)) == 0
    assert mm.bits_equal(got, io)
    sub = slice(0, 400)
    assert mm.bits_equal(got[sub], dm.world_points(p["u"][sub], p["v"][sub], p["idepth"][sub], ci, m))
    # the cloud: the literal model on a prefix that holds negative idepths, the vectorised one (held equal on the CPU) on all
    rdraws = rng.randint(0, 2 ** 31 - 1, len(p)).astype(np.int32)
    for d in (None, rdraws):
        g = A.map_dense_cloud(FID, draws=d)
        xyz, rgb = dm.refresh_pc_fast(p["u"], p["v"], p["idepth"], p["bgr"], ci, d)
        assert g["records"] == len(p) and g["survivors"] == len(xyz) == int((~(p["idepth"] < 0)).sum()) < len(p)
        assert mm.bits_equal(g["xyz"], xyz) and np.array_equal(g["rgb"], rgb)
        first_neg = int(np.nonzero(p["idepth"] < 0)[0][0])
        k = min(len(p), first_neg + 300)
        lx, lr = dm.refresh_pc(p["u"][:k], p["v"][:k], p["idepth"][:k], p["bgr"][:k], ci, d)
        assert len(lx) < k and mm.bits_equal(g["xyz"][:len(lx)], lx) and np.array_equal(g["rgb"][:len(lx)], lr)
    for kw in (dict(cap=len(p) - 1), dict(draws=rdraws, n_draws=len(p) - 1)):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            A.map_dense_cloud(FID, **kw)
        assert A.dense_cloud_needed == len(p)
    n = C.c_int(-1)
    buf = np.zeros((len(p), 3))
    assert A.L.nalo_map_dense_world_points(A.h_, FID, mc.ctypes.data_as(dp), buf.ctypes.data_as(dp), len(p) - 1, C.byref(n)) == ERR_ARG and n.value == len(p) and not buf.any()
    out = np.zeros(len(p), binding.DENSE_POINT_DTYPE)
    assert A.L.nalo_map_dense_get(A.h_, FID, out.ctypes.data_as(C.c_void_p), len(p) - 1, C.byref(n)) == ERR_ARG and n.value == len(p)
    for fn in (lambda: A.map_dense_get(7), lambda: A.map_dense_world_points(7, m), lambda: A.map_dense_cloud(7), lambda: A.map_dense_counts(7)):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
            fn()
    A.close()


# ------------------------------------------------------------------------------------------------ the chain
def state_bytes(c, fids):
    """the window, the immature set, the tracker cloud and the sparse archive through the existing getters"""
    out = [c.ba_get_points()[k].tobytes() for k in ("idepth", "step", "HdiF", "bdSumF", "Hdd", "bd", "Hcd", "maxRelBaseline")]
    out += [np.ascontiguousarray(a).tobytes() for a in c.ba_get_residuals()]
    out += [np.ascontiguousarray(a).tobytes() for a in c.imm_resident_get()]
    out += [np.ascontiguousarray(a).tobytes() for a in c.trk_get_pc(0)]
    for f in fids:
        out += [c.map_get_frame(f).tobytes(), repr(c.map_counts(f)).encode()]
    return out


def test_two_keyframes_of_the_device_chain():
    """flag -> marginalize_flagged -> marginalize_frame -> carry_window at 320x240 (the window of tests/test_map_gpu.py's chain, W = 5), nalo_dense_update_map on
    frameHessians[size - 3] each keyframe, a third keyframe so that the first archived frame leaves the window; then the clouds of all archived frames. The later
    calls also check that the window, the immature set, the tracker cloud and the sparse archive are what they were."""
    import lifecycle_model as lm
    import lifecycle_scenes as lsc
    WW, KF = 5, 3
    s = 3e-4
    w, h = 320, 240
    win = synth.make_window(w=w, h=h, W=WW, P=1500, seed=lsc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    nF = WW + KF
    srng = np.random.RandomState(lsc.SEED + 3)
    st6 = np.zeros((nF, 6))
    st6[1:, :3] = 0.004 * srng.randn(nF - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * srng.randn(nF - 1, 3)
    mask = band_mask(w, h)
    bgr = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    A, B = [binding.Context(w, h, win.K, n_slots=nF) for _ in range(2)]
    fids = [200 + i for i in range(WW)]
    rng = np.random.RandomState(2)
    n_imm = 300
    z8, z3, z1 = np.zeros((n_imm, 8), F), np.zeros((n_imm, 3), F), np.zeros(n_imm, F)
    imm = (rng.randint(4, w - 4, n_imm).astype(F), rng.randint(4, h - 4, n_imm).astype(F), z8, z8 + 1, z3, z1 + 10, np.full(n_imm, WW - 1, np.int32),
           np.full(n_imm, 0.1, F), np.full(n_imm, 0.2, F), np.zeros(n_imm, np.int32), z1)
    for c in (A, B):
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
        c.imm_resident_set(*imm)
        c.trk_set_pc(WW - 1, 0, imm[0], imm[1], np.full(n_imm, 0.5, F), np.full(n_imm, 100, F))
    A.map_dense_enable(True, 4096)
    want = {}
    cur = list(fids)
    known = set()
    for kf in range(KF):
        for c in (A, B):
            if kf:
                c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            c.ba_linearize(False)
            c.ba_linearize(True)
        if kf:
            cur = cur[1:] + [200 + WW - 1 + kf]
        hf, slot = WW - 3, WW - 3 + kf
        T = synth.se3_inv(win.world_to_cam[slot])
        draws = pm.make_draws(60 + kf)
        seen = sorted(known)                                                                   # the frames the sparse archive holds so far
        before = state_bytes(A, seen) if kf else None
        recs, runs, napp = A.dense_update_map(hf, draws, T)
        if kf:
            assert state_bytes(A, seen) == before and len(seen) >= 3
        rb, runs_b, pts_b = route_b(B, hf, slot, draws, T, w, h)
        print("DENSE MAP chain keyframe %d: n %s accept %s appended %d" % (kf, runs["n"].tolist(), runs["accept"].tolist(), napp))
        assert recs.tobytes() == rb.tobytes() and runs.tobytes() == runs_b.tobytes() and napp == len(pts_b) > 4096
        want[cur[hf]] = pts_b
        ff = np.zeros(WW, np.uint8); ff[0] = 1
        for c in (A, B):
            c.ba_flag_points(ff)
            c.ba_marginalize_flagged()
            c.ba_marginalize_frame(0)
        known |= set(cur)
    ci = mm.calib_inverse(A.ba_get_frames()[2])
    assert sorted(want) == [202, 203, 204] and 202 not in cur[1:]                                # 202 has left the window
    for fid, p in want.items():
        assert points_equal(A.map_dense_get(fid), p)
        g = A.map_dense_cloud(fid)
        xyz, rgb = dm.refresh_pc_fast(p["u"], p["v"], p["idepth"], p["bgr"], ci)
        assert mm.bits_equal(g["xyz"], xyz) and np.array_equal(g["rgb"], rgb) and g["records"] == len(p)
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------ no side effects, refusals, determinism
def test_no_side_effects_and_refusals():
    win, mask, bgr, gone, imm, (A, B) = dense_variant_window(band_mask(320, 240))
    B.close()
    draws = pm.make_draws(31)
    T = synth.se3_inv(win.world_to_cam[1])

    def refused(fn, code):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % code):
            fn()

    refused(lambda: A.dense_update_map(1, draws, T), ERR_STATE)                                 # the dense archive is not enabled
    u, v = np.arange(5, 205, dtype=F), np.full(200, 50, F)
    A.trk_set_pc(1, 0, u, v, np.full(200, 0.5, F), np.full(200, 100, F))
    A.map_dense_enable(True, 4096)
    fids = []                                                                                  # (the sparse archive: test_two_keyframes_of_the_device_chain)
    before = state_bytes(A, fids)
    recs, runs, napp = A.dense_update_map(1, draws, T)
    assert napp > 0 and state_bytes(A, fids) == before
    counts = A.map_dense_counts(FID + 1)
    refused(lambda: A.dense_update_map(1, draws, None), ERR_ARG)                                # camToWorld == NULL
    refused(lambda: A.dense_update_map(1, draws, T, null_runs=True), ERR_ARG)                   # runs == NULL
    refused(lambda: A.dense_update_map(1, draws, T, cap=2), ERR_ARG)                            # cap too small: the need is reported
    assert A.plane_n_clusters == len(recs) == 4
    refused(lambda: A.dense_update_map(1, draws[:0], T), ERR_ARG)                               # nalo_dense_fit_planes' own refusals, with its codes
    refused(lambda: A.dense_update_map(1, None, T), ERR_ARG)
    refused(lambda: A.dense_update_map(1, draws, T, threshold=-1.0), ERR_ARG)
    refused(lambda: A.dense_update_map(win.W, draws, T), ERR_ARG)                               # outside the window
    assert A.map_dense_counts(FID + 1) == counts and state_bytes(A, fids) == before
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        A.map_dense_counts(FID + 2)                                                            # a refused call does not make a frame known
    A.ba_set_allreduce(lambda ptr, n: None)
    refused(lambda: A.dense_update_map(1, draws, T), ERR_STATE)                                 # sharded, as nalo_dense_fit_planes refuses it
    assert A.map_dense_counts(FID + 1) == counts
    A.close()
    c = binding.Context(64, 48, small_K(64, 48), n_slots=2)
    refused(lambda: c.dense_update_map(0, draws, T), ERR_STATE)                                 # not enabled
    c.map_dense_enable(True)
    refused(lambda: c.dense_update_map(0, draws, T), ERR_STATE)                                 # no window
    refused(lambda: c.map_dense_enable(True, -1), ERR_ARG)
    img = np.full((48, 64), 50, F)
    c.frame_upload(0, img); c.frame_upload(1, img)
    c.ba_set_window([0, 1], np.tile(np.eye(3, 4), (2, 1, 1)), frame_ids=[FID, FID + 1])
    c.ba_set_points(np.zeros(20, np.int32), np.arange(20, dtype=F) + 5, np.full(20, 20, F), np.full(20, 0.3, F), np.full((20, 8), 100, F), np.ones((20, 8), F))
    refused(lambda: c.dense_update_map(0, draws, T), ERR_STATE)                                 # the frame's slot has no mask
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.map_dense_counts(FID)
    c.close()


def test_three_runs_give_identical_bytes():
    sc = kitti_scene()
    draws = pm.make_draws(12)
    got = []
    for _ in range(3):
        A = context(sc)
        recs, runs, napp = A.dense_update_map(0, draws, C2W)
        got.append((recs.tobytes(), runs.tobytes(), napp, A.map_dense_get(FID).tobytes()))
        A.close()
    assert got[0] == got[1] == got[2]
