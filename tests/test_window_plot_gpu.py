"""nalo_map_window_plot: FullSystem::debugPlot (FullSystemDebugStuff.cpp:109-358) on the device, against tests/window_plot_model.py.

Every comparison is exact: np.array_equal on the images' bytes and the ring counts, bit equality on the floats. The model's inputs are the library's public
read-backs: nalo_frame_download (level 0), nalo_ba_get_points (the current inverse depths; u, v and which points are still valid are the test's own bookkeeping of
what it submitted and what nalo_ba_flag_points decided), nalo_map_get_frame, nalo_imm_resident_get / nalo_imm_resident_get_points. `literal` is the reference's
loops one to one and serves the small shapes; `fast` is its vectorised twin (tests/test_window_plot_cpu.py shows fast == literal) and serves the full-size frames.

  1  planted windows at 64x32 (W = 2), 80x48 (W = 3) and 70x33 (W = 2, a pixel count that is no multiple of the resolve pass's four pixels per lane): active and
     immature lists of 0, 1, 2, 63, 64, 65 and 257 points, centres on and around every border and either side of every edge of both kernels' work split, positions
     either side of .5, overlapping rings of one list, special inverse depths and irradiances, every mode; one context through 1, 4, 1 and 3 painted frames of
     70x50 (the key plane grows, is used below its capacity and again after that)
  2  the archive lists, planted through the chain's own calls as tests/test_map_gpu.py plants its hosts (640x480, W = 6): hosts with 0, 1, 2, 63 and 65 planted
     removals, then 64 and 257 more (which of them are marginalised and which dropped is the data's choice), a host that loses nothing and one that loses only
     points without a residual; a second issue of the window puts an active ring on top of every archived one
  3  mode 7: ties, the pair carried over three calls, NULL, an allID of out-points only, a masked-out frame that still counts
  4  three keyframes of the device chain at 1224x368, W = 8, a frame leaving in between; one keyframe at 1920x1072
  5  no side effects (a twin context that never plots; the depth image before and after), determinism, every refusal

A window frame's slot without a pyramid cannot be reached through the public calls (nalo_ba_set_window refuses such a window), so that refusal is not provoked."""
import ctypes as C

import numpy as np
import pytest

import lifecycle_model as lm
import lifecycle_scenes as sc
import test_map_gpu as tm
import window_plot_model as model
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

F = np.float32
ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -4, -5
MODES = (0, 1, 2, 3, 4, 5, 7, 8, 9)
SPECIAL = np.array([-1.5, 0.0, -0.0, np.nan, np.inf, -np.inf, 1e-42, 2147483648.0, 3e9, 2147483520.0], F)


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def same(dev, want, what=""):
    assert want is not None, what
    assert dev["bgr"].shape == want["bgr"].shape, (what, dev["bgr"].shape, want["bgr"].shape)
    bad = (dev["bgr"] != want["bgr"]).any(axis=3)
    assert not bad.any(), "%s: %d pixels differ, first at (frame, y, x) = %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    assert np.array_equal(dev["sources"], want["sources"]), (what, dev["sources"].tolist(), want["sources"].tolist())
    assert dev["n_values"] == want["n_values"], what
    for k in ("min_new", "max_new", "min_used", "max_used"):
        assert bits(dev[k]) == bits(want[k]), (what, k, dev[k], want[k])
    assert (dev["minmax"] is None) == (want["minmax"] is None)
    if want["minmax"] is not None:
        assert np.array_equal(bits(dev["minmax"]), bits(want["minmax"])), (what, dev["minmax"], want["minmax"])


def read_frames(c, slots, fids, host, u, v, valid):
    """the window as the model takes it, from the context's read-backs. host / u / v: what was submitted, valid: the points still in the window"""
    idepth = c.ba_get_points()["idepth"]
    imm = None
    if getattr(c, "_imm_n", 0):
        idmin, idmax, status, quality = c.imm_resident_get()[:4]
        p = c.imm_resident_get_points(with_type=False)
        imm = dict(u=p["u"], v=p["v"], host=p["host_idx"], idmin=idmin, idmax=idmax, status=status, quality=quality)
    frames = []
    for i, (slot, fid) in enumerate(zip(slots, fids)):
        f = dict(I=c.frame_download(slot, 0)[0][:, 0].copy())
        sel = valid & (host == i)
        f["active"] = dict(u=u[sel], v=v[sel], idepth=idepth[sel])
        try:
            rec = c.map_get_frame(fid)
        except binding.NaloError:
            rec = None                                                           # no archive, or one that has never seen the frame
        if rec is not None:
            for name, st in (("marg", 2), ("out", 3)):
                r = rec[rec["status"] == st]
                f[name] = dict(u=r["u"].copy(), v=r["v"].copy(), idepth=r["idepth"].copy())
        if imm is not None:
            s = imm["host"] == i
            f["imm"] = {k: a[s] for k, a in imm.items() if k != "host"}
        frames.append(f)
    return frames


def check(c, frames, w, h, mode, mask=0, minmax=None, rs=1.0, qs=1.0, fids=None, fn=model.fast, what=""):
    got = c.map_window_plot(mode, mask, minmax, rs, qs)
    want = fn(frames, w, h, mode, mask, minmax, rs, qs)
    same(got, want, "%s mode %d mask %x" % (what, mode, mask))
    if fids is not None:
        assert got["frame_id"] == [fids[i] for i in want["frames"]]
    return got, want


# ------------------------------------------------------------------------------------------------ 1: planted windows at the smallest shapes
def planted_image(w, h, seed):
    rng = np.random.RandomState(seed)
    I = rng.uniform(0, 255, (h, w)).astype(F)
    I[1, 1:6] = [-1.2, -40.0, 283.5, 1e12, np.nan]                               # negative (wraps), above 283 (saturates at 255), beyond int, NaN
    I[h - 2, w - 3] = -3e9
    I[rng.rand(h, w) < 0.01] = np.nan
    return I


def border_centres(w, h):
    xs = [0, 1, 2, 3] + list(range(w - 4, w))
    ys = [0, 1, 2, 3] + list(range(h - 4, h))
    uv = [(x, y) for x in xs for y in ys]
    uv += [(-4, 5), (-5, 5), (w + 2, 5), (w + 3, 5), (5, -4), (5, h + 2), (5, h + 3), (-40000.0, 3e9)]     # rings that only touch the image, or miss it
    uv += [(10.49, 10.5), (10.5, 10.49), (10.51, 11.4999), (11.4999, 10.51)]                             # either side of .5
    # either side of every edge of the resolve pass's split: four pixels per lane, 1024 per workgroup (whole rows here), a frame's last row and the next one's first
    rows = sorted({y for e in range(1024 // w, h, max(1024 // w, 1)) for y in range(e - 4, e + 4) if 0 <= y < h})
    uv += [(x, y) for y in rows for x in (5, 6, 7, 8, 9)]
    return np.array(uv, F)


def planted_window(w, h, W, sizes, seed, levels=0):
    """W frames whose active lists have `sizes` points: the border centres first, then overlapping random ones; special inverse depths among them"""
    rng = np.random.RandomState(seed)
    c = binding.Context(w, h, (0.5 * w, 0.5 * w, (w - 1) / 2.0, (h - 1) / 2.0), n_slots=W, levels=levels)
    for i in range(W):
        c.frame_upload(i, planted_image(w, h, seed + i))
    fids = [40 + 3 * i for i in range(W)]
    c.ba_set_window(list(range(W)), [np.eye(3, 4)] * W, frame_ids=fids)
    bc = border_centres(w, h)
    host, u, v = [], [], []
    for i, n in enumerate(sizes):
        uv = np.concatenate([bc, np.stack([rng.uniform(-2, w + 2, n), rng.uniform(-2, h + 2, n)], 1).astype(F)])[:n] if n > 2 else np.array([[6, 6], [8, 7]], F)[:n]
        host += [i] * n
        u += uv[:, 0].tolist(); v += uv[:, 1].tolist()
    order = rng.permutation(len(host))                                           # hosts interleaved in submission order
    host, u, v = np.array(host, np.int32)[order], np.array(u, F)[order], np.array(v, F)[order]
    P = len(host)
    idepth = rng.uniform(0.05, 6.0, P).astype(F)
    m = rng.rand(P) < 0.25
    idepth[m] = SPECIAL[rng.randint(0, len(SPECIAL), int(m.sum()))]
    near = rng.rand(P) < 0.1                                                     # values that differ in the last mantissa bits
    idepth[near] = np.where(rng.rand(int(near.sum())) < 0.5, np.nextafter(F(2.0), F(3.0)), np.nextafter(F(2.0), F(1.0))).astype(F)
    c.ba_set_points(host, u, v, idepth, np.zeros((P, 8), F), np.ones((P, 8), F))
    c.ba_set_residuals(np.zeros((P, W), np.uint8))
    return c, dict(fids=fids, host=host, u=u, v=v, valid=np.ones(P, bool), slots=list(range(W)))


def planted_immature(c, w, h, sizes, seed):
    """a resident set whose hosts have `sizes` points, hosts interleaved in storage; all six statuses and one that is none of them"""
    rng = np.random.RandomState(seed)
    bc = border_centres(w, h)
    host, uv = [], []
    for i, n in enumerate(sizes):
        host += [i] * n
        uv.append(np.concatenate([bc, np.stack([rng.uniform(-2, w + 2, n), rng.uniform(-2, h + 2, n)], 1).astype(F)])[:n])
    uv = np.concatenate(uv)
    n = len(host)
    order = rng.permutation(n)
    host, uv = np.array(host, np.int32)[order], uv[order]
    idmax = rng.uniform(0.5, 3.0, n).astype(F)
    idmax[rng.rand(n) < 0.15] = np.nan
    idmax[rng.rand(n) < 0.05] = np.inf
    idmin = rng.uniform(-0.5, 1.0, n).astype(F)
    q = rng.uniform(0.2, 6.0, n).astype(F)
    m = rng.rand(n) < 0.2
    q[m] = SPECIAL[rng.randint(0, len(SPECIAL), int(m.sum()))]
    status = rng.permutation(np.arange(n) % 7).astype(np.int32)                  # 6: no ImmaturePointStatus at all
    c.imm_resident_set(uv[:, 0].copy(), uv[:, 1].copy(), np.zeros((n, 8), F), np.ones((n, 8), F), np.ones((n, 3), F), np.full(n, 100, F), host, idmin, idmax, status, q)


@pytest.mark.parametrize("w,h,W,sizes,imm_sizes,levels", [(64, 32, 2, (257, 64), (65, 257), 0), (80, 48, 3, (63, 0, 65), (1, 64, 0), 0), (80, 48, 3, (1, 2, 257), (2, 63, 2), 0),
                                                           (70, 33, 2, (65, 130), (64, 70), 1)])
def test_planted_windows_every_mode(w, h, W, sizes, imm_sizes, levels):
    c, S = planted_window(w, h, W, sizes, seed=w + sum(sizes), levels=levels)
    planted_immature(c, w, h, imm_sizes, seed=h)
    frames = read_frames(c, S["slots"], S["fids"], S["host"], S["u"], S["v"], S["valid"])
    assert [len(f["active"]["u"]) for f in frames] == list(sizes) and [len(f["imm"]["u"]) for f in frames] == list(imm_sizes)
    st = np.concatenate([f["imm"]["status"] for f in frames])
    assert set(st.tolist()) == set(range(min(7, len(st))))
    for mode in MODES:
        got, want = check(c, frames, w, h, mode, 0, (-1.0, -1.0), fids=S["fids"], fn=model.literal, what="%dx%d" % (w, h))
        again = c.map_window_plot(mode, 0, (-1.0, -1.0))
        assert np.array_equal(got["bgr"], again["bgr"]) and np.array_equal(got["sources"], again["sources"])      # the same bytes on every run
        if mode in (2, 8, 9):
            assert not got["sources"].any()
    for mode, rs, qs in ((0, 0.37, 1.0), (1, 1e9, 1.0), (3, 2.5, 1.0), (5, 1.0, 0.3), (5, 1.0, -2.0)):
        check(c, frames, w, h, mode, 0, None, rs, qs)
    for mask in [1 << i for i in range(W)] + [(1 << W) - 1, 0b101 & ((1 << W) - 1)]:
        check(c, frames, w, h, 1, mask, fids=S["fids"])
        check(c, frames, w, h, 4, mask, fids=S["fids"])
    c.close()


def test_plane_cleans_itself():
    """ONE context paints 1, then all 4, then 1, then 3 frames of 70x50: 3500 pixels a frame are no multiple of the resolve pass's 1024, so every frame after the
    first straddles workgroups and the last workgroup has a tail. The key plane and the counters beside it grow, are used below their capacity, and are used again
    after that; every call's bytes and ring counts equal the model's."""
    w, h, W = 70, 50, 4
    c, S = planted_window(w, h, W, (65, 130, 63, 257), seed=w + h, levels=1)
    planted_immature(c, w, h, (64, 70, 1, 129), seed=h)
    frames = read_frames(c, S["slots"], S["fids"], S["host"], S["u"], S["v"], S["valid"])
    for mask in (0b0100, 0b1111, 0b0010, 0b1011):
        for mode in (1, 4):
            check(c, frames, w, h, mode, mask, fids=S["fids"], fn=model.literal, what="the plane's walk")
    c.close()


def test_overlapping_rings_of_one_list():
    """rings of the same list with different colours, centres 0..6 pixels apart in both directions and both submission orders"""
    w, h = 64, 32
    c = binding.Context(w, h, (32.0, 32.0, 31.5, 15.5), n_slots=2)
    for i in range(2):
        c.frame_upload(i, planted_image(w, h, i))
    c.ba_set_window([0, 1], [np.eye(3, 4)] * 2, frame_ids=[7, 9])
    u, v, idp, host = [], [], [], []
    for k, (dx, dy) in enumerate([(0, 0), (1, 0), (2, 1), (3, 3), (4, 2), (5, 0), (6, 6), (0, 5)]):
        x0, y0 = 6 + 14 * (k % 4), 6 + 14 * (k // 4)
        for hst, first in ((0, True), (1, False)):                                # frame 1 holds the same pairs in the other order
            pair = [(x0, y0, 0.25), (x0 + dx, y0 + dy, 1.5)]
            for (x, y, d) in (pair if first else pair[::-1]):
                u.append(x); v.append(y); idp.append(d); host.append(hst)
    host, u, v, idp = np.array(host, np.int32), np.array(u, F), np.array(v, F), np.array(idp, F)
    c.ba_set_points(host, u, v, idp, np.zeros((len(u), 8), F), np.ones((len(u), 8), F))
    c.ba_set_residuals(np.zeros((len(u), 2), np.uint8))
    frames = read_frames(c, [0, 1], [7, 9], host, u, v, np.ones(len(u), bool))
    got, _ = check(c, frames, w, h, 1, fn=model.literal)
    assert not np.array_equal((got["bgr"][0] == model.rainbow(0.25)).all(axis=2), (got["bgr"][1] == model.rainbow(0.25)).all(axis=2))   # the order shows
    check(c, frames, w, h, 0, fn=model.literal)
    c.close()


# ------------------------------------------------------------------------------------------------ 2: the archive lists, planted through the chain
def overlap_pairs(a, b):
    """pairs of centres of two lists whose rings can share a pixel (Chebyshev distance <= 6)"""
    if len(a["u"]) == 0 or len(b["u"]) == 0:
        return 0
    ax, ay, bx, by = [np.floor(np.asarray(q, np.float64) + 0.5) for q in (a["u"], a["v"], b["u"], b["v"])]
    return int(((np.abs(ax[:, None] - bx[None]) <= 6) & (np.abs(ay[:, None] - by[None]) <= 6)).sum())


def test_archive_lists_planted_through_the_chain():
    sizes = [0, 0, 1, 2, 63, 65]                                                 # host 0 loses nothing, host 1 only points without a residual (always `out`)
    S = tm.planted_scene(sizes)
    win = S["win"]
    w, h, W, P = win.w, win.h, 6, len(S["host"])
    idepth = S["idepth"].copy()
    exists = S["exists"].copy()
    rng = np.random.RandomState(3)
    odd = rng.permutation(np.nonzero(S["host"] >= 1)[0])[:len(SPECIAL) * 4]      # points without a residual and with a special inverse depth: dropped, with that value
    idepth[odd] = np.tile(SPECIAL, 4)
    exists[odd] = 0
    S = dict(S, idepth=idepth, exists=exists)
    A = tm.make_ctx(S)
    A.map_enable(chunk_points=300)
    slots = list(range(W))
    none = np.zeros(W, np.uint8)
    frames0 = read_frames(A, slots, S["fids"], S["host"], S["u"], S["v"], np.ones(P, bool))
    assert all("marg" not in f for f in frames0)
    check(A, frames0, w, h, 1, what="before any removal")                        # an enabled archive that has seen no frame: the two lists are empty
    for rnd, sz in enumerate((sizes, [0, 0, 64, 257, 0, 0])):
        if rnd:
            tm.issue(A, S)                                                       # every point active again, on top of its archived twin
        A.ba_set_point_history(*tm.plant(S, sz, 30 + rnd))
        A.ba_linearize(False)
        dec, _, _ = A.ba_flag_points(none)
        A.ba_marginalize_flagged()
        valid = dec == lm.KEEP
        frames = read_frames(A, slots, S["fids"], S["host"], S["u"], S["v"], valid)
        cls = [[len(f[k]["u"]) for k in ("active", "marg", "out")] for f in frames]
        print("WINDOW PLOT archive round %d: active / marginalised / out per frame %s" % (rnd, cls))
        for mode in (0, 1, 7):
            check(A, frames, w, h, mode, 0, (-1.0, -1.0), fids=S["fids"], what="round %d" % rnd)
        check(A, frames, w, h, 1, 0b100010, what="round %d" % rnd)
    pairs = [sum(overlap_pairs(f[a], f[b]) for f in frames) for a, b in (("active", "marg"), ("active", "out"), ("marg", "out"))]
    print("WINDOW PLOT archive: overlapping pairs active-marg / active-out / marg-out", pairs)
    assert all(p > 0 for p in pairs)
    assert any(len(f["marg"]["u"]) == 0 and len(f["out"]["u"]) > 0 for f in frames)      # a frame with only out-points
    assert any(len(f["marg"]["u"]) == 0 and len(f["out"]["u"]) == 0 for f in frames)     # and one with none
    assert np.isnan(np.concatenate([f["out"]["idepth"] for f in frames])).any()
    A.close()


# ------------------------------------------------------------------------------------------------ 3: mode 7
def mode7_ctx(idepth_by_host, w=64, h=32):
    W = len(idepth_by_host)
    c = binding.Context(w, h, (32.0, 32.0, 31.5, 15.5), n_slots=W)
    for i in range(W):
        c.frame_upload(i, planted_image(w, h, 50 + i))
    fids = [5 + i for i in range(W)]
    c.ba_set_window(list(range(W)), [np.eye(3, 4)] * W, frame_ids=fids)
    rng = np.random.RandomState(W)
    host = np.concatenate([np.full(len(d), i, np.int32) for i, d in enumerate(idepth_by_host)])
    idepth = np.concatenate([np.asarray(d, F) for d in idepth_by_host])
    P = len(host)
    u, v = rng.uniform(3, w - 4, P).astype(F), rng.uniform(3, h - 4, P).astype(F)
    c.ba_set_points(host, u, v, idepth, np.zeros((P, 8), F), np.ones((P, 8), F))
    c.ba_set_residuals(np.zeros((P, W), np.uint8))
    return c, dict(fids=fids, host=host, u=u, v=v, valid=np.ones(P, bool), slots=list(range(W)))


@pytest.mark.parametrize("values", [
    [[0.5] * 30 + [1.5] * 30, [0.5] * 41],                                         # ranks that tie
    [[-1.0, -0.0, 0.0, 2.0], [np.nan] * 5 + [-np.inf, np.inf]],                    # both signs, the zeros, NaNs left out
    [[3.0], [np.nan]],                                                             # one value
    [np.arange(1, 21, dtype=F) / 7, np.arange(1, 22, dtype=F) / -3],               # 41 values
    [np.random.RandomState(1).lognormal(0, 2, 300), np.random.RandomState(2).randn(301) * 1e-3]])
def test_mode7_range_and_smoothing(values):
    c, S = mode7_ctx(values)
    frames = read_frames(c, S["slots"], S["fids"], S["host"], S["u"], S["v"], S["valid"])
    pair_dev = pair_model = (-1.0, -1.0)
    for call in range(3):                                                        # the pair carried as FullSystem carries minIdJetVisDebug / maxIdJetVisDebug
        got, want = check(c, frames, 64, 32, 7, 0, pair_dev, fn=model.literal, what="call %d" % call)
        pair_dev, pair_model = got["minmax"], want["minmax"]
        assert np.array_equal(bits(pair_dev), bits(pair_model))
    check(c, frames, 64, 32, 7, 0, None, fn=model.literal, what="NULL")
    for pair in ((0.1, 0.2), (5.0, 1.0), (0.0, 0.0), (np.inf, np.inf), (np.nan, 1.0), (1e-3, 1e4)):
        check(c, frames, 64, 32, 7, 0, pair, fn=model.literal, what=str(pair))
    got, want = check(c, frames, 64, 32, 7, 0b10, (-1.0, -1.0), fn=model.literal, what="masked")     # frame 0 is not painted and still counts
    assert got["n_values"] == want["n_values"] == int((~np.isnan(np.concatenate([np.asarray(v, F) for v in values]))).sum())
    c.close()


def test_mode7_all_id_of_out_points_only():
    """every point of the window is dropped (no residual): allID is the archive's out lists alone, nothing is drawn in mode 7 and the range is theirs"""
    S = tm.scene(640, 480, 4, 200)
    S = dict(S, exists=np.zeros_like(S["exists"]))
    A = tm.make_ctx(S)
    A.map_enable()
    A.ba_set_point_history(*sc.plant_history(200, 4))
    A.ba_linearize(False)
    dec, _, _ = A.ba_flag_points(np.zeros(4, np.uint8))
    A.ba_marginalize_flagged()
    assert (dec != lm.KEEP).all()
    frames = read_frames(A, [0, 1, 2, 3], S["fids"], S["host"], S["u"], S["v"], dec == lm.KEEP)
    assert sum(len(f["out"]["u"]) for f in frames) == 200 and not sum(len(f["marg"]["u"]) + len(f["active"]["u"]) for f in frames)
    got, _ = check(A, frames, 640, 480, 7, 0, (-1.0, -1.0))
    assert got["n_values"] == 200 and not got["sources"].any()
    check(A, frames, 640, 480, 0)
    A.close()


# ------------------------------------------------------------------------------------------------ 4: the device chain at real shapes
def run_chain(w, h, WW, P, KF, check_kf):
    """tests/test_map_gpu.py's three keyframes of the device chain (flag -> marginalize_flagged -> marginalize_frame -> carry_window) at a size of its own;
    check_kf(A, kf, frames, fids) is called after nalo_ba_marginalize_flagged of every keyframe"""
    s = 3e-4
    win = synth.make_window(w=w, h=h, W=WW, P=P, seed=sc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    nF = WW + KF
    rng = np.random.RandomState(sc.SEED + 3)
    st6 = np.zeros((nF, 6))
    st6[1:, :3] = 0.004 * rng.randn(nF - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * rng.randn(nF - 1, 3)
    A = binding.Context(win.w, win.h, win.K, n_slots=nF)
    for i in range(nF):
        A.frame_upload(i, win.images[i])
    A.ba_set_prior_carry(True)
    fids = [200 + i for i in range(WW)]
    slots = list(range(WW))
    A.ba_set_window(slots, win.world_to_cam[:WW], state6=st6[:WW], frame_ids=fids)
    A.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    A.ba_set_residuals(win.exists)
    ng0, lt0, ls0 = lm.default_history(win.exists)
    ls0[win.host == WW - 1, 0] = lm.IN
    A.ba_set_point_history(ng0, lt0, ls0)
    A.map_enable(chunk_points=300)
    host, u, v = win.host.copy(), win.u, win.v
    for kf in range(KF):
        if kf:
            A.ba_carry_window(A.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            m = A.ba_carry_map()
            host, u, v = host[m] - 1, u[m], v[m]
            fids, slots = fids[1:] + [200 + WW - 1 + kf], slots[1:] + [WW - 1 + kf]
        A.ba_linearize(False)
        A.ba_linearize(True)
        ff = np.zeros(WW, np.uint8); ff[0] = 1
        dec, _, _ = A.ba_flag_points(ff)
        A.ba_marginalize_flagged()
        imm = tm.immature_set(1500 * WW, WW, w, h, seed=11 + kf)
        imm["status"] = np.random.RandomState(kf).randint(0, 6, len(imm["u"])).astype(np.int32)
        A.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
        frames = read_frames(A, slots, fids, host, u, v, dec == lm.KEEP)
        print("WINDOW PLOT chain %dx%d keyframe %d: active / marginalised / out / immature per frame %s" %
              (w, h, kf, [[len(f[k]["u"]) for k in ("active", "marg", "out", "imm")] for f in frames]))
        check_kf(A, kf, frames, fids)
        if kf + 1 < KF:
            A.ba_marginalize_frame(0)                                            # the frame leaves
    A.close()


def test_three_keyframes_of_the_device_chain_kitti_shape():
    w, h = 1224, 368
    pair = {"dev": (-1.0, -1.0), "model": (-1.0, -1.0)}

    def check_kf(A, kf, frames, fids):
        assert len(frames) == 8 and sum(len(f["marg"]["u"]) + len(f["out"]["u"]) for f in frames) >= 50
        got, _ = check(A, frames, w, h, 1, fids=fids, what="keyframe %d" % kf)
        assert got["bgr"].shape == (8, h, w, 3)
        check(A, frames, w, h, (0, 3, 5)[kf], what="keyframe %d" % kf)
        check(A, frames, w, h, 4, 0b10010001, what="keyframe %d" % kf)
        got, want = check(A, frames, w, h, 7, 0, pair["dev"], what="keyframe %d" % kf)
        pair["dev"], pair["model"] = got["minmax"], want["minmax"]
    run_chain(w, h, 8, 2000, 3, check_kf)


def test_one_keyframe_at_1920x1072():
    w, h = 1920, 1072

    def check_kf(A, kf, frames, fids):
        check(A, frames, w, h, 1, fids=fids)
        check(A, frames, w, h, 7, 0b101, (0.01, 0.5))
        check(A, frames, w, h, 3, 0b010)
    run_chain(w, h, 3, 3000, 1, check_kf)


# ------------------------------------------------------------------------------------------------ 5: side effects, refusals
def state_of(c, fids):
    out = []
    pts = c.ba_get_points()
    out += [pts[k] for k in sorted(pts)]
    out += list(c.ba_get_residuals()) + list(c.ba_get_prior()) + list(c.ba_get_point_history())
    out += [np.array(c.ba_counts())] + [np.array(c.map_counts(f)) for f in fids] + [c.map_get_frame(f) for f in fids]
    out += list(c.imm_resident_get()) + [c.imm_resident_get_points(with_type=False)[k] for k in ("u", "v", "host_idx")]
    di = c.trk_depth_image((0.01, 0.2))
    out += [di["bgr"], di["minmax"]]
    for l in range(c.levels):
        out += list(c.trk_get_pc(l)) + list(c.trk_get_depth(l))
    return [np.ascontiguousarray(x) for x in out]


def test_no_side_effects_against_a_twin_that_never_plots():
    S = tm.scene(640, 480, 4, 400)
    A, T = tm.make_ctx(S), tm.make_ctx(S)
    imm = tm.immature_set(500, 4, 640, 480)
    for c in (A, T):
        c.map_enable()
        c.map_graph_enable()
        c.ba_set_point_history(*sc.plant_history(400, 4))
        c.ba_linearize(False)
        c.ba_linearize(True)
        c.trk_set_ref_from_window()
        c.imm_resident_set(imm["u"], imm["v"], imm["color"], imm["weights"], imm["gradH"], imm["energyTH"], imm["host_idx"], imm["idmin"], imm["idmax"], imm["status"], imm["quality"])
        if c is A:
            c.map_window_plot(1)                                                 # the reference's place: right after the optimisation
        c.ba_flag_points(sc.flag_sets(4)[1])
        c.ba_marginalize_flagged()
    before = A.trk_depth_image((0.01, 0.2))
    pair = (-1.0, -1.0)
    for mode in MODES:
        pair = A.map_window_plot(mode, 0, pair)["minmax"]
    A.map_window_plot(1, 0b0101)
    after = A.trk_depth_image((0.01, 0.2))
    assert np.array_equal(before["bgr"], after["bgr"]) and np.array_equal(bits(before["minmax"]), bits(after["minmax"]))
    sa, st = state_of(A, S["fids"]), state_of(T, S["fids"])
    assert len(sa) == len(st)
    for k, (x, y) in enumerate(zip(sa, st)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert np.array_equal(A.map_graph(), T.map_graph())
    # and the chain goes on as the twin's does
    for c in (A, T):
        c.ba_marginalize_frame(1)
    for x, y in zip(A.ba_get_prior(), T.ba_get_prior()):
        assert x.tobytes() == y.tobytes()
    A.close()
    T.close()


def _raw(c, bgr, mm, mode=1, mask=0, rs=1.0, qs=1.0, null_args=False, null_ctx=False):
    a = binding.WindowPlotArgs()
    a.mode, a.rainbow_scale, a.quality_scale, a.frame_mask = mode, rs, qs, mask
    a.minmax_io = None if mm is None else mm.ctypes.data_as(binding.c_fp)
    a.bgr = None if bgr is None else bgr.ctypes.data_as(binding.c_u8p)
    a.n_values = -7
    rc = c.L.nalo_map_window_plot(None if null_ctx else c.h_, None if null_args else C.byref(a))
    return rc, a


def test_refusals_leave_the_outputs_untouched():
    w, h = 64, 32
    bgr = np.full((3, h, w, 3), 0xA5, np.uint8)
    mm = np.array([0.25, 0.75], F)

    def untouched(b=bgr):
        return (b == 0xA5).all() and mm.tolist() == [0.25, 0.75]
    # no window
    c0 = binding.Context(w, h, (32.0, 32.0, 31.5, 15.5), n_slots=1)
    c0.frame_upload(0, planted_image(w, h, 0))
    assert _raw(c0, bgr, mm)[0] == ERR_STATE and untouched()
    c0.close()
    c, S = mode7_ctx([[0.5, 1.0, 2.0], [np.nan, 3.0]])
    frames = read_frames(c, S["slots"], S["fids"], S["host"], S["u"], S["v"], S["valid"])
    # bad arguments
    assert _raw(c, bgr, mm, null_ctx=True)[0] == ERR_ARG and _raw(c, bgr, mm, null_args=True)[0] == ERR_ARG and _raw(c, None, mm)[0] == ERR_ARG
    assert _raw(c, bgr, mm, mode=-1)[0] == ERR_ARG and _raw(c, bgr, mm, mode=10)[0] == ERR_ARG
    assert _raw(c, bgr, mm, mask=0b100)[0] == ERR_ARG and _raw(c, bgr, mm, mask=1 << 31)[0] == ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        assert _raw(c, bgr, mm, rs=bad)[0] == ERR_ARG and _raw(c, bgr, mm, mode=7, qs=bad)[0] == ERR_ARG
    assert _raw(c, bgr, mm, mode=6)[0] == ERR_UNSUPPORTED and b"mode 6" in c.L.nalo_last_error(c.h_)
    assert untouched()
    # the call works, before and after the refusals, and writes only the frames it paints
    rc, a = _raw(c, bgr, mm, mode=7, mask=0b10)
    want = model.literal(frames, w, h, 7, 0b10, (0.25, 0.75))
    assert rc == 0 and a.n_frames == 1 and a.frame_id[0] == S["fids"][1] and np.array_equal(bgr[0], want["bgr"][0]) and (bgr[1:] == 0xA5).all()
    assert np.array_equal(bits(mm), bits(want["minmax"])) and a.n_values == 4
    bgr[:] = 0xA5
    mm[:] = [0.25, 0.75]
    # mode 7 with an empty allID: nothing painted, the pair left as it was
    e, _ = mode7_ctx([[np.nan, np.nan], [np.nan]])
    rc, a = _raw(e, bgr, mm, mode=7)
    assert rc == ERR_STATE and a.n_values == 0 and untouched() and b"mode 7" in e.L.nalo_last_error(e.h_)
    assert _raw(e, bgr, mm, mode=1)[0] == 0 and not (bgr[:2] == 0xA5).all() and mm.tolist() == [0.25, 0.75]      # the other modes do not need it
    bgr[:] = 0xA5
    e.close()
    # a sharded window
    c.ba_set_allreduce(lambda ptr, n: None)
    assert _raw(c, bgr, mm)[0] == ERR_STATE and b"sharded" in c.L.nalo_last_error(c.h_) and untouched()
    # a context whose cross-rank exchange failed
    c.ba_exchange_failed("link down (window plot test)")
    assert _raw(c, bgr, mm)[0] == ERR_HIP and untouched()
    c.close()


def test_point_arrays_unset_between_marginalize_frame_and_the_carry():
    S = tm.scene(640, 480, 4, 400)
    A = tm.make_ctx(S)
    A.map_enable()
    A.ba_set_point_history(*sc.plant_history(400, 4))
    A.ba_linearize(False)
    A.ba_linearize(True)
    dec, _, _ = A.ba_flag_points(sc.flag_sets(4)[1])
    A.ba_marginalize_flagged()
    frames = read_frames(A, [0, 1, 2, 3], S["fids"], S["host"], S["u"], S["v"], dec == lm.KEEP)
    check(A, frames, 640, 480, 1, fids=S["fids"])
    A.ba_marginalize_frame(1)
    bgr = np.full((4, 480, 640, 3), 0xA5, np.uint8)
    mm = np.array([0.25, 0.75], F)
    assert _raw(A, bgr, mm, mode=7)[0] == ERR_STATE and (bgr == 0xA5).all() and mm.tolist() == [0.25, 0.75]
    A.ba_carry_window()                                                          # carried: three frames, the archive lists of the three that stay
    m = A.ba_carry_map()
    keep = [0, 2, 3]
    host = np.array([keep.index(x) for x in S["host"][m]], np.int32)
    frames = read_frames(A, keep, [S["fids"][i] for i in keep], host, S["u"][m], S["v"][m], np.ones(len(m), bool))
    check(A, frames, 640, 480, 1, fids=[S["fids"][i] for i in keep], what="after the carry")
    A.close()
