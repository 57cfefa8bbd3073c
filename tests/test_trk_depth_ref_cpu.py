"""The definition of nalo_trk_set_ref_from_depth (include/nalo_gpu.h) on the host: tests/trk_depth_ref_model.py against itself, against a plane worked by hand
and through the fp32 oracle's orc_trk_set_ref. No device; tests/test_trk_depth_ref_gpu.py takes its planes from here."""
import numpy as np

import orc
import trk_depth_ref_model as dm

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
DENORMAL = F(1e-45)                                      # the smallest positive float: 1.0f / DENORMAL overflows to +inf


def up(x):
    return np.nextafter(F(x), INF)


def down(x):
    return np.nextafter(F(x), -INF)


def seeded_depth(w, h, seed, lo=0.8, hi=6.0):
    return np.random.RandomState(seed).uniform(lo, hi, (h, w)).astype(F)


def frame_image(w, h, seed):
    """a textured frame: seeded noise over a ramp, so that absSquaredGrad spreads over a few decades"""
    rng = np.random.RandomState(seed)
    return (40.0 + 120.0 * np.linspace(0, 1, w)[None, :] * np.ones((h, 1)) + rng.rand(h, w) * 60.0).astype(F)


def tile_edge_pixels(w, h):
    """either side of every 32-pixel tile edge, the four corners, and the 2-pixel border that step 5 drops"""
    xs = sorted({x for e in range(0, w + 1, 32) for x in (e - 1, e) if 0 <= x < w} | {0, 1, w - 2, w - 1})
    ys = sorted({y for e in range(0, h + 1, 32) for y in (e - 1, e) if 0 <= y < h} | {0, 1, h - 2, h - 1})
    return xs, ys


def planted_depth(w, h, seed, min_depth, max_depth):
    """a seeded plane in which most pixels fail (0.0, as a ray-cast's misses) and the planted ones decide: the range's ends and their neighbours, the values no
    depth may be, passing pixels at the tile edges, corners and borders, a lone pixel and two checkerboards (x + y even: the diagonal dilation of levels 0 and 1
    finds no empty pixel with a full neighbour, the axis dilation of level 2 does; x + y odd shifted: the reverse)"""
    rng = np.random.RandomState(seed)
    d = np.zeros((h, w), F)
    xs, ys = tile_edge_pixels(w, h)
    for y in ys:
        d[y, :] = rng.uniform(min_depth, max_depth, w).astype(F)
    for x in xs:
        d[:, x] = rng.uniform(min_depth, max_depth, h).astype(F)
    d[4:14, 4:16] = np.where((np.add.outer(np.arange(10), np.arange(12)) % 2) == 0, F(2.0), F(0.0))
    d[16:26, 5:17] = np.where((np.add.outer(np.arange(10), np.arange(12)) % 2) == 1, F(1.5), F(0.0))
    d[15, 20:26] = 0.0
    d[14:17, 22] = 0.0
    d[15, 22] = F(1.25)                                                        # a single passing pixel: nothing passes around it
    special = [F(min_depth), F(max_depth), down(min_depth), up(max_depth), F(0.0), F(-0.0), F(-1.5), NAN, INF, -INF]
    for k, val in enumerate(special):
        d[6 + (k // 5) * 3, 28 + (k % 5) * 2 + (k // 5)] = val
    return d


def maps_before_dilation_recognisable(idp, ws, want_id, want_ws, ok, colour, w, h):
    """The oracle's level-0 maps after steps 1-5 at the pixels that passed, where step 1's values can still be read. A pixel with weight > 0 is never dilated
    (steps 3/4 write only where the weight is <= 0). Step 5 normalises the interior only: on the 2-pixel border a passing pixel still holds (1 / D) * weight and
    weight; inside it holds ((1 / D) * weight) / weight and 1 when that is > 0 and its colour finite, and -1 with its weight unchanged otherwise."""
    idp, ws = idp.reshape(h, w), ws.reshape(h, w)
    border = np.ones((h, w), bool)
    border[2:h - 2, 2:w - 2] = False
    b = ok & border
    assert dm.bits(idp[b]) == dm.bits(want_id[b]) and dm.bits(ws[b]) == dm.bits(want_ws[b])
    assert not (idp[border & ~ok & (np.arange(h)[:, None] % (h - 1) == 0)]).any()      # first and last row are never dilated: zeros where nothing passed
    with np.errstate(all="ignore"):
        val = want_id / want_ws
    kept = ok & ~border & np.isfinite(colour) & (val > 0)
    dropped = ok & ~border & ~kept
    assert dm.bits(idp[kept]) == dm.bits(val[kept]) and (ws[kept] == 1).all()
    assert (idp[dropped] == -1).all() and dm.bits(ws[dropped]) == dm.bits(want_ws[dropped])
    return kept


# ------------------------------------------------------------------------------------------------ the model against itself
def test_vectorised_form_equals_the_literal_one():
    for seed, (w, h) in enumerate(((17, 9), (33, 35), (70, 34))):
        rng = np.random.RandomState(seed)
        depth = planted_depth(w, h, seed, 0.75, 4.0) if w >= 40 else seeded_depth(w, h, seed, 0.2, 6.0)
        absg = (rng.rand(h, w) * 100).astype(F)
        depth[h // 2, w // 3], absg[h // 3, w // 2], absg[1, 1] = NAN, NAN, F(50.0)
        depth[0, 0], depth[h - 1, w - 1], depth[0, w - 1], depth[h - 1, 0] = F(0.75), F(4.0), down(0.75), up(4.0)
        for step in (1, 2, 5, w + 1):
            for mg in (0.0, -0.0, 50.0, 1e9, -3.0):
                lit = dm.inputs_literal(depth, absg, 0.75, 4.0, 1e-4, step, mg)
                vec = dm.inputs(depth, absg, 0.75, 4.0, 1e-4, step, mg)
                assert all(dm.bits(a) == dm.bits(b) for a, b in zip(lit, vec)), (w, h, step, mg)
                idp, ws = dm.step1(depth, absg, 0.75, 4.0, 1e-4, step, mg)
                assert int((ws > 0).sum()) == len(lit[0])
                u, v = lit[0].astype(int), lit[1].astype(int)
                assert dm.bits(idp[v, u]) == dm.bits(lit[2] * dm.weight_of(1e-4)) and (ws[v, u] == dm.weight_of(1e-4)).all()
        assert len(dm.inputs(depth, absg, 0.75, 4.0, 1e-4, w + 1, 0.0)[0]) == 1            # only (0, 0) is on that grid: D == min_depth passes
    # a denormal min_depth: its reciprocal overflows, the product stays +inf
    depth = np.full((3, 4), DENORMAL, F)
    lit = dm.inputs_literal(depth, None, DENORMAL, 1.0, 0.0)
    assert len(lit[0]) == 12 and np.isposinf(lit[2]).all() and np.isposinf(dm.step1(depth, None, DENORMAL, 1.0, 0.0)[0]).all()


def test_a_6x5_plane_through_every_clause_by_hand():
    w, h = 6, 5
    depth, absg = np.full((h, w), F(2.0)), np.full((h, w), F(100.0))            # off the step grid everything would pass
    cells = {(0, 0): (2.0, 10.0),            # passes; absg == min_grad exactly
             (2, 0): (1.0, 11.0),            # passes; D == min_depth
             (4, 0): (4.0, 50.0),            # passes; D == max_depth
             (0, 2): (down(1.0), 50.0),      # one ulp below min_depth
             (2, 2): (up(4.0), 50.0),        # one ulp above max_depth
             (4, 2): (NAN, 50.0),            # a NaN fails both comparisons
             (0, 4): (2.0, down(10.0)),      # one ulp below min_grad
             (2, 4): (3.0, NAN),             # a NaN gradient fails
             (4, 4): (2.5, INF)}             # passes
    for (u, v), (D, g) in cells.items():
        depth[v, u], absg[v, u] = D, g
    for fn in (dm.inputs_literal, dm.inputs):
        Ku, Kv, nid, hd = fn(depth, absg, 1.0, 4.0, 0.25, 2, 10.0)
        assert Ku.tolist() == [0, 2, 4, 4] and Kv.tolist() == [0, 0, 0, 4]
        assert dm.bits(nid) == dm.bits(np.array([0.5, 1.0, 0.25, F(1.0) / F(2.5)], F)) and hd.tolist() == [0.25] * 4 and all(a.dtype == F for a in (Ku, Kv, nid, hd))
        Ku, Kv, nid, _ = fn(depth, absg, 1.0, 4.0, 0.25, 2, 0.0)               # the gradient test off: the two gradient failures pass, in raster order
        assert Ku.tolist() == [0, 2, 4, 0, 2, 4] and Kv.tolist() == [0, 0, 0, 4, 4, 4] and nid[3] == 0.5 and dm.bits(nid[4:5]) == dm.bits(np.array([F(1.0) / F(3.0)], F))
        assert len(fn(depth, absg, 1.0, 4.0, 0.25, 1, 0.0)[0]) == 27            # every pixel but the three depth failures
        assert len(fn(depth, absg, 1.0, 4.0, 0.25, 1, 10.0)[0]) == 25
        Ku, Kv, _, _ = fn(depth, absg, 1.0, 4.0, 0.25, 7, 0.0)                 # a step beyond both sizes: pixel (0, 0) alone
        assert Ku.tolist() == [0] and Kv.tolist() == [0]
        assert len(fn(depth, absg, 4.5, 5.0, 0.25, 1, 0.0)[0]) == 0
    assert dm.weight_of(0.25) == np.sqrt(F(1e-3 / (0.25 + 1e-12))) and dm.weight_of(0.0) == np.sqrt(F(1e9))


# ------------------------------------------------------------------------------------------------ through the oracle
def oracle_ref(img, levels, K, lists):
    h, w = img.shape
    trk = orc.Tracker(w, h, levels, K)
    dI, _ = orc.make_images(img, levels)
    trk.set_ref(dI, *lists)
    return trk


def test_through_the_oracle_at_70x34_with_three_levels():
    w, h, L = 70, 34, 3
    K = (0.52 * w, 0.52 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    img = frame_image(w, h, 3)
    img[10, 10], img[20, 40] = NAN, NAN                                        # the colour rejection of step 5, under passing pixels
    colour = img
    # 1. every pixel passes: nothing is left for the dilation to fill, and pc_n[0] is the passing interior pixels with a finite colour
    depth = seeded_depth(w, h, 1)
    trk = oracle_ref(img, L, K, dm.inputs(depth, None, 0.5, 8.0, 1e-4))
    want_id, want_ws = dm.step1(depth, None, 0.5, 8.0, 1e-4)
    ok = dm.passing(depth, None, 0.5, 8.0)
    assert ok.all()
    kept = maps_before_dilation_recognisable(*trk.get_depth(0), want_id, want_ws, ok, colour, w, h)
    pc = trk.get_pc(0)
    assert len(pc[0]) == int(kept.sum()) == (w - 4) * (h - 4) - 2
    assert np.array_equal(pc[0], np.nonzero(kept)[1].astype(F)) and np.array_equal(pc[1], np.nonzero(kept)[0].astype(F))       # raster order
    # 2. planted planes: passing pixels keep step 1's values; the cloud is those of the interior plus what the diagonal dilation fills around them
    for step, mg in ((1, 0.0), (2, 0.0), (1, None)):
        depth = planted_depth(w, h, 5, 0.75, 4.0)
        absg = orc.make_images(img, L)[1][:w * h].reshape(h, w)
        mg = float(np.median(absg)) if mg is None else mg
        lists = dm.inputs(depth, absg, 0.75, 4.0, 0.01, step, mg)
        trk = oracle_ref(img, L, K, lists)
        want_id, want_ws = dm.step1(depth, absg, 0.75, 4.0, 0.01, step, mg)
        ok = dm.passing(depth, absg, 0.75, 4.0, step, mg)
        assert 50 < ok.sum() < w * h // 2 and int(ok.sum()) == len(lists[0])
        kept = maps_before_dilation_recognisable(*trk.get_depth(0), want_id, want_ws, ok, colour, w, h)
        p = np.pad(ok, 1)
        filled = ~ok & (p[2:, 2:] | p[:-2, :-2] | p[2:, :-2] | p[:-2, 2:])    # steps 3/4 at level 0: an empty pixel with a passing diagonal neighbour
        filled[:2], filled[-2:], filled[:, :2], filled[:, -2:] = False, False, False, False
        assert len(trk.get_pc(0)[0]) == int(kept.sum()) + int((filled & np.isfinite(colour)).sum())
    # 3. nothing passes: every map is what step 5 leaves of zeros, every cloud empty
    trk = oracle_ref(img, L, K, dm.inputs(np.zeros((h, w), F), None, 0.5, 8.0, 1e-4))
    for l in range(L):
        assert len(trk.get_pc(l)[0]) == 0
