"""The front end at its tile and table edges: nalo_undist_set + nalo_frame_upload_raw[_async] (ingest_kernel<BPP, PHOTO>) and makeImages (pyramid_build:
pyr_one_pass_kernel<2 / 3 / 4> with and without its coarse workgroups, pyr_down_kernel + pyr_grad_all_kernel) at small contexts whose sizes are chosen for the
branch they reach - partial fine tiles, coarse tiles that are left, right and partial at once, levels with one or no interior row, odd parents, a last
workgroup and a last wave of the ingest that are partial - against the CPU oracle (orc_undistort, orc_resize_nearest_u8, orc_make_images with and without B;
tests/test_oracle_cpu.py pins those against a literal model and hand-worked cases at such shapes).

Every comparison is BIT FOR BIT on every level the context has: the values are compared as uint32 words, so -0.0 and +0.0 are told apart. One exception: where
the oracle's value is NaN the device's must be NaN at the same position - payload and sign of a generated NaN differ between x86 and gfx950."""
import numpy as np
import pytest

import orc
from nalo_slam_amd import binding
from test_ingest_gpu import radial_remap

pytestmark = pytest.mark.gpu

GAMMA = (255.0 * (np.arange(256) / 255.0) ** 0.8).astype(np.float32)         # the table of test_gamma_table_in_make_images
GAMMA2 = (255.0 * (np.arange(256) / 255.0) ** 1.3).astype(np.float32)        # a different one (the async entries' "a different table waits" branch)
ERR_ARG, ERR_STATE = -1, -4


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def orc_pyramid(img, levels, B=None):
    """[(dI [n_l, 3], absSquaredGrad [n_l])] per level from orc_make_images"""
    h, w = img.shape
    L = orc.lib()
    offs = [L.orc_pyr_offset(w, h, l) for l in range(levels + 1)]
    dI, ab = np.zeros((offs[-1], 3), np.float32), np.zeros(offs[-1], np.float32)
    L.orc_make_images(orc.fp(np.ascontiguousarray(img, np.float32)), w, h, levels, None if B is None else orc.fp(B), orc.fp(dI), orc.fp(ab))
    return [(dI[offs[l]:offs[l + 1]], ab[offs[l]:offs[l + 1]]) for l in range(levels)]


def gpu_pyramid(c, slot):
    return [c.frame_download(slot, l) for l in range(c.levels)]


def assert_pyramids_equal(got, want, tag):
    assert len(got) == len(want)
    for lvl, ((g_dI, g_ab), (o_dI, o_ab)) in enumerate(zip(got, want)):
        for k, name in enumerate(("I", "dx", "dy")):
            assert same_bits(g_dI[:, k], o_dI[:, k]), (tag, "level %d" % lvl, name, int((g_dI[:, k].view(np.uint32) != o_dI[:, k].view(np.uint32)).sum()))
        assert same_bits(g_ab, o_ab), (tag, "level %d" % lvl, "absSquaredGrad")


def context(w, h, levels=0, n_slots=1):
    c = binding.Context(w, h, (0.52 * w, 0.52 * w, (w - 1) / 2.0, (h - 1) / 2.0), n_slots=n_slots, levels=levels)
    assert levels == 0 or c.levels == levels
    return c


def pyramid_path(w, h, levels):
    """pyramid_build's rule: one pass for 2..5 levels over even parents (a 64x16 tile holds a whole pixel of level 4 at most), level by level otherwise"""
    fused = 2 <= levels and (1 << (levels - 1)) <= 16 and all((w >> (l - 1)) % 2 == 0 and (h >> (l - 1)) % 2 == 0 for l in range(1, levels))
    return {2: "one_pass_NL2", 3: "one_pass_NL3", 4: "one_pass_NL4", 5: "one_pass_NL3_coarse"}[levels] if fused else "level_by_level"


def make_image(w, h, seed=0):
    """seeded random, amplitude 0..255; the top-left quarter is dark (0..3) and the bottom-right one bright (252..255), so that the intensity clamps of the gamma
    factor (ci < 5, ci > 250) are reached on the upper levels too, where the box filter has averaged noise away"""
    rng = np.random.RandomState(1000 * w + h + seed)
    img = (rng.rand(h, w) * 255).astype(np.float32)
    img[:h // 2, :w // 2] = (rng.rand(h // 2, w // 2) * 3).astype(np.float32)
    img[h - h // 2:, w - w // 2:] = (252 + rng.rand(h // 2, w // 2) * 3).astype(np.float32)
    return img


def shifted(img):
    """the same image spanning -20..300: negative and > 255 intensities under the gamma table"""
    return (img * np.float32(320.0 / 255.0) - np.float32(20.0)).astype(np.float32)


# (w, h, levels, the path pyramid_build's rule selects): what each size is there for
PYR_CASES = [
    (80, 48, 5, "one_pass_NL3_coarse"),      # one coarse tile that is left, right and partial both ways (w3 = 10, h3 = 6); w4 = 5 odd; fine right column partial
    (208, 112, 5, "one_pass_NL3_coarse"),    # the second coarse tile partial and `right` (w3 = 26); h3 = 14: 3.5 coarse tile rows; w4 = 13
    (272, 80, 5, "one_pass_NL3_coarse"),     # w3 = 34: a last coarse tile of 2 columns; h4 = 5
    (48, 48, 5, "one_pass_NL3_coarse"),      # level 4 is 3x3: one interior row, both flat-index neighbours from the rebuilt edge values
    (32, 32, 5, "one_pass_NL3_coarse"),      # level 4 is 2x2: no interior
    (16, 16, 5, "one_pass_NL3_coarse"),      # level 4 is 1x1, level 3 2x2
    (72, 40, 4, "one_pass_NL4"),             # partial right and bottom fine tiles; level 3 is 9x5 (odd)
    (136, 72, 4, "one_pass_NL4"),            # three tile columns, five tile rows, both last ones partial; level 3 is 17x9
    (24, 24, 4, "one_pass_NL4"),             # level 3 is 3x3
    (64, 16, 4, "one_pass_NL4"),             # exactly one full tile
    (68, 20, 3, "one_pass_NL3"),             # 16-byte tile loads with a partial tile both ways, no coarse workgroups
    (132, 36, 3, "one_pass_NL3"),
    (66, 18, 2, "one_pass_NL2"),             # scalar tile loads, w % 4 != 0
    (70, 34, 2, "one_pass_NL2"),
    (71, 37, 1, "level_by_level"),           # odd w and h, no parent: pyr_grad_all_kernel alone
    (70, 34, 3, "level_by_level"),           # odd parents 35x17 -> 17x8: pyr_down_kernel's second 8-byte load is 4-byte aligned
    (100, 52, 4, "level_by_level"),          # odd parents 25x13 -> 12x6
    (64, 32, 6, "level_by_level"),           # six levels down to 2x1 (no interior)
    (96, 96, 6, "level_by_level"),           # six levels down to 3x3
]


@pytest.mark.parametrize("gamma", [False, True], ids=["plain", "gamma"])
@pytest.mark.parametrize("w,h,levels,path", PYR_CASES, ids=["%dx%d_L%d_%s" % c for c in PYR_CASES])
def test_pyramid_at_tile_edges(w, h, levels, path, gamma):
    assert pyramid_path(w, h, levels) == path                                # the table above states the rule's outcome, not a wish
    img = make_image(w, h)
    c = context(w, h, levels)
    try:
        for name, im in ([("shifted", shifted(img)), ("0..255", img)] if gamma else [("0..255", img)]):
            B = GAMMA if gamma else None
            want = orc_pyramid(im, levels, B)
            c.frame_upload(0, im, gammaB=B)
            assert_pyramids_equal(gpu_pyramid(c, 0), want, (w, h, levels, path, name))
            if gamma:
                plain = orc_pyramid(im, levels)
                for lvl in range(levels):
                    wl, hl = w >> lvl, h >> lvl
                    if hl >= 3:
                        assert not np.array_equal(want[lvl][1], plain[lvl][1]), lvl                  # the table changes absSquaredGrad on this level
                    if name == "shifted" and hl >= 5 and wl >= 4:                                     # ... and both clamps are reached on it, from outside 0..255
                        inner = want[lvl][0][wl:wl * (hl - 1), 0]
                        assert (inner < 0).any() and (inner > 255.5).any(), lvl
    finally:
        c.close()


def plant_non_finite(img):
    """+inf, -inf and NaN at interior pixels, in column 0 and column w-1 (each other's flat-index neighbours), either side of the fine-tile corner (64, 16) and of
    the coarse-tile corner (128, 32) where the image reaches them"""
    h, w = img.shape
    img = img.copy()
    plants = [(w // 2 + 1, h // 2, np.inf), (w // 3, h // 3 + 1, np.nan), (2 * w // 3 + 1, 2 * h // 3, -np.inf),
              (0, 5, -np.inf), (w - 1, 9, np.inf), (0, h - 3, np.nan), (w - 1, h - 6, np.nan),
              (63, 15, np.nan), (64, 16, np.inf), (127, 31, -np.inf), (128, 32, np.nan)]
    n = 0
    for x, y, v in plants:
        if x < w and 0 < y < h - 1:
            img[y, x] = v; n += 1
    assert n >= 8
    return img


@pytest.mark.parametrize("w,h,levels", [(208, 112, 5), (72, 40, 4), (70, 34, 3)], ids=["208x112_L5_coarse", "72x40_L4", "70x34_L3_level_by_level"])
def test_non_finite_pixels(w, h, levels):
    """`if (!isfinite(dx)) dx = 0` (HessianBlocks.cpp:174-175) in every kernel that states it. No gamma table: (int)(inf + 0.5f) is undefined in the reference."""
    img = plant_non_finite(make_image(w, h, seed=1))
    want = orc_pyramid(img, levels)
    for lvl, (dI, _) in enumerate(want):                                     # the input reaches the branch on every level, for dx and for dy
        wl, hl = w >> lvl, h >> lvl
        nf = ~np.isfinite(dI[:, 0])
        inner = np.zeros(wl * hl, bool); inner[wl:wl * (hl - 1)] = True
        for col, step in ((1, 1), (2, wl)):
            nb = np.zeros(wl * hl, bool); nb[step:] |= nf[:-step]; nb[:-step] |= nf[step:]
            assert (nb & inner).any() and (dI[nb & inner, col] == 0).all(), (lvl, col)
        assert np.isfinite(dI[:, 1:]).all()
    c = context(w, h, levels)
    try:
        c.frame_upload(0, img)
        assert_pyramids_equal(gpu_pyramid(c, 0), want, (w, h, levels))
    finally:
        c.close()


@pytest.mark.parametrize("w,h,levels", [(80, 48, 5), (72, 40, 4)], ids=["80x48_L5_coarse", "72x40_L4"])
def test_flat_index_wrap(w, h, levels):
    """the gradient runs over the flat index (HessianBlocks.cpp:168-181): column 0 differences against the last pixel of the row above, column w-1 against the
    first pixel of the row below. Those columns are constant and far from the rest, so a border clamp would differ on every level."""
    img = make_image(w, h, seed=2)
    img[:, 0], img[:, -1] = 1000.0, -1000.0
    want = orc_pyramid(img, levels)
    for lvl, (dI, _) in enumerate(want):
        wl, hl = w >> lvl, h >> lvl
        if hl >= 3:
            I, dx = dI[:, 0].reshape(hl, wl), dI[:, 1].reshape(hl, wl)
            assert (dx[1:-1, 0] != np.float32(0.5) * (I[1:-1, 1] - I[1:-1, 0])).all() and (dx[1:-1, -1] != np.float32(0.5) * (I[1:-1, -1] - I[1:-1, -2])).all(), lvl
    c = context(w, h, levels)
    try:
        c.frame_upload(0, img)
        assert_pyramids_equal(gpu_pyramid(c, 0), want, (w, h, levels))
    finally:
        c.close()


def test_async_uploads_with_changing_gamma_tables():
    """nalo_frame_upload_async with gammaB: the first table, a different one on the next slot (its copy waits for the main stream), the first again. Each slot
    equals its synchronous upload, and that equals the oracle."""
    w, h, levels = 208, 112, 5
    c = context(w, h, levels, n_slots=4)
    try:
        tables = [GAMMA, GAMMA2, GAMMA]
        imgs = [shifted(make_image(w, h, seed=10 + k)) for k in range(3)]
        ref = []
        for im, B in zip(imgs, tables):
            c.frame_upload(3, im, gammaB=B)
            ref.append(gpu_pyramid(c, 3))
            assert_pyramids_equal(ref[-1], orc_pyramid(im, levels, B), "sync")
        pinned = []
        for im in imgs:
            a = c.pinned_array((h, w), np.float32); a[:] = im; pinned.append(a)
        for rep in range(2):                                                 # the second round overwrites slots and changes the table while kernels may still read both
            for k in range(3):
                c.frame_upload_async(k, pinned[k], gammaB=tables[k])
            for k in (1, 2, 0):
                c.frame_wait(k)
            c.sync()
            for k in range(3):
                assert_pyramids_equal(gpu_pyramid(c, k), ref[k], ("async", rep, k))
    finally:
        c.close()


def test_raw_async_uploads_with_changing_gamma_tables():
    """the same through nalo_frame_upload_raw_async (gammaB passed through by the binding), and gammaB through the synchronous nalo_frame_upload_raw"""
    w, h, levels, wo, ho = 208, 112, 5, 230, 130
    rng = np.random.RandomState(21)
    G = np.cumsum(rng.rand(256) + 0.05).astype(np.float32); G = (255.0 * (G - G[0]) / (G[-1] - G[0])).astype(np.float32)
    rx, ry = radial_remap(w, h, wo, ho)
    c = context(w, h, levels, n_slots=4)
    try:
        c.undist_set(wo, ho, G, None, 1, rx, ry)
        tables = [GAMMA, GAMMA2, GAMMA]
        raws = [rng.randint(0, 256, (ho, wo)).astype(np.uint8) for _ in range(3)]
        ref = []
        for raw, B in zip(raws, tables):
            c.frame_upload_raw(3, raw, exposure=0.01, factor=1.0, gammaB=B)
            ref.append(gpu_pyramid(c, 3))
            assert_pyramids_equal(ref[-1], orc_pyramid(orc.undistort(raw, G, None, 1, 1.0, rx, ry, w, h), levels, B), "sync")
        pinned = []
        for raw in raws:
            a = c.pinned_array((ho, wo), np.uint8); a[:] = raw; pinned.append(a)
        for rep in range(2):
            for k in range(3):
                c.frame_upload_raw_async(k, pinned[k], exposure=0.01, factor=1.0, gammaB=tables[k])
            for k in (2, 0, 1):
                c.frame_wait(k)
            c.sync()
            for k in range(3):
                assert_pyramids_equal(gpu_pyramid(c, k), ref[k], ("raw async", rep, k))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ ingest
WO, HO = 99, 51                                                              # odd original width
INGEST_SIZES = [(72, 40, 4), (70, 34, 3)]                                    # n = 2880 = 2 * 1024 + 832: a partial last workgroup; n = 2380 = 2 * 1024 + 5 * 64 + 12: a partial last wave


def response(depth, seed=7):
    rng = np.random.RandomState(seed)
    G = np.cumsum(rng.rand(depth) + 0.05)
    return (255.0 * (G - G[0]) / (G[-1] - G[0])).astype(np.float32)


def vignette_inv(wo, ho):
    yy, xx = np.mgrid[0:ho, 0:wo]
    vmap = (1.0 - 0.4 * (((xx - wo / 2) / wo) ** 2 + ((yy - ho / 2) / ho) ** 2)).astype(np.float32)
    return (np.float32(1.0) / vmap).astype(np.float32)


def planted_remap(w, h, wo, ho):
    """the radial table with twenty planted entries, at the first pixels, either side of every 256-lane stride and workgroup border, and in the tail.
    Returns (rx, ry, taps): taps = the (xi, yi) of every planted entry that reads the image."""
    rx, ry = radial_remap(w, h, wo, ho)
    f = np.float32
    below = lambda v: np.nextafter(f(v), f(0))
    entries = [
        (below(wo - 1), below(ho - 1)),      # the last legal tap, (int)x == wOrg-2, (int)y == hOrg-2, both fractions next to 1
        (below(wo - 1), f(ho - 2)),          # ... with an integer y
        (f(wo - 2), below(ho - 1)),          # ... with an integer x
        (f(wo - 2), f(ho - 2)),              # ... both integers: weight 1 on the top-left tap, 0 on the last pixel of the image
        (f(10), f(7)),                       # exact integers: the bilinear fractions are 0
        (f(20), f(10.75)), (f(20.25), f(10)),
        (f(0), f(0)), (f(0), below(ho - 1)), (below(wo - 1), f(0)),
        (f(-0.0), f(3.5)), (f(3.5), f(-0.0)), (f(-0.0), f(-0.0)),            # -0.0 is not < 0: a tap at column / row 0 with a fraction of -0.0
        (f(-1), f(12.25)), (f(-0.5), f(3)), (f(-1e-30), f(ho - 2)),          # x < 0 with a valid y: outside, 0
        (f(0.5), f(0.5)), (f(wo - 2.5), f(ho - 2.5)), (f(47.999996), f(24.000002)), (f(1e-30), f(1e-30)),
    ]
    n = w * h
    where = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, n - 1, n - 2, n - 3, n - 4, n - 5, n // 2, n // 2 + 1, n // 3]
    assert len(where) == len(entries) == len(set(where)) == 20 and max(where) < n
    fx, fy = rx.reshape(-1), ry.reshape(-1)
    taps = []
    for i, (x, y) in zip(where, entries):
        fx[i], fy[i] = x, y
        if not x < 0:
            taps.append((int(x), int(y)))
    return rx, ry, taps


def raw_image(dtype, wo, ho, taps, seed):
    """random, with 0 and the type's maximum under the planted taps"""
    rng = np.random.RandomState(seed)
    top = np.iinfo(dtype).max
    raw = rng.randint(0, top + 1, (ho, wo)).astype(dtype)
    for k, (xi, yi) in enumerate(taps):
        raw[yi:yi + 2, xi:xi + 2] = [[[0, top], [top, 0]], [[top, top], [top, top]], [[0, 0], [0, 0]], [[top, 0], [0, top]]][k % 4]
    return raw


@pytest.mark.parametrize("remap", [True, False], ids=["remap", "passthrough"])
@pytest.mark.parametrize("photometric", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_ingest_every_instantiation(dtype, photometric, remap):
    """ingest_kernel<1 / 2, 0 / 1 / 2> with and without the remap, with a tail: level-0 irradiance and the whole pyramid against orc_undistort + orc_make_images"""
    depth = 256 if dtype == np.uint8 else 65536
    G = response(depth)
    for w, h, levels in INGEST_SIZES:
        assert (w * h) % 1024 != 0 and ((w * h) % 256 != 0)
        wo, ho = (WO, HO) if remap else (w, h)
        vinv = vignette_inv(wo, ho)
        rx, ry, taps = planted_remap(w, h, wo, ho) if remap else (None, None, [(0, 0), (wo - 2, ho - 2), (5, 5), (6, 8)])
        raw = raw_image(dtype, wo, ho, taps, seed=w + photometric)
        c = context(w, h, levels)
        try:
            c.undist_set(wo, ho, G, vinv if photometric == 2 else None, photometric, rx, ry)      # the planted table is accepted: every entry is a legal one
            for exposure in (0.02, 0.0):                                     # exposure <= 0: factor * raw for that frame
                ph = photometric if exposure > 0 else 0
                c.frame_upload_raw(0, raw, exposure=exposure, factor=0.5)
                img = orc.undistort(raw, G, vinv if ph == 2 else None, ph, 0.5, rx, ry, w, h)
                got = gpu_pyramid(c, 0)
                assert same_bits(got[0][0][:, 0], img), (w, h, exposure, "level-0 irradiance")
                assert_pyramids_equal(got, orc_pyramid(img, levels), (w, h, exposure))
                if remap:
                    assert (img == 0).sum() >= 7 and (img != 0).mean() > 0.8
        finally:
            c.close()


@pytest.mark.parametrize("wo,ho", [(105, 51), (96, 53), (48, 27)], ids=["ratio_1.5", "ratio_96_70", "upscale"])
def test_mask_and_colour_resize(wo, ho):
    """the INTER_NEAREST resizes of undistort_mask inside the ingest pass, read back at every pixel (nalo_frame_download_mask): a ratio that is exact in binary,
    one whose reciprocal is not, and an upscale"""
    w, h = 70, 34
    rng = np.random.RandomState(wo)
    raw = rng.randint(0, 256, (ho, wo)).astype(np.uint8)
    mask_o = rng.randint(0, 256, (ho, wo)).astype(np.uint8)
    mask_o[0, 0], mask_o[-1, -1], mask_o[0, -1] = 0, 255, 254
    bgr_o = rng.randint(0, 256, (ho, wo, 3)).astype(np.uint8)
    rx, ry = radial_remap(w, h, wo, ho)
    c = context(w, h, n_slots=2)
    try:
        c.undist_set(wo, ho, None, None, 0, rx, ry)
        c.frame_upload_raw(1, raw)                                           # a frame without mask and colour: the slot holds neither
        with pytest.raises(binding.NaloError, match="error %d" % ERR_STATE):
            c.frame_download_mask(1)
        c.frame_upload_raw(0, raw, mask_org=mask_o, bgr_org=bgr_o)
        m, b = c.frame_download_mask(0)
        want_m, want_b = orc.resize_nearest_u8(mask_o, w, h), orc.resize_nearest_u8(bgr_o, w, h)
        assert m.dtype == np.float32 and np.array_equal(m, want_m.astype(np.float32))
        assert np.array_equal(b, want_b)
        assert len(np.unique(want_m)) > 100
        assert np.array_equal(c.frame_download_mask(0, bgr=False)[0], m) and np.array_equal(c.frame_download_mask(0, mask=False)[1], b)
        assert same_bits(c.frame_download(0, 0)[0][:, 0], orc.undistort(raw, None, None, 0, 1.0, rx, ry, w, h))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ refusals (none is followed by an upload that would use the refused table)
@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("bad", [3e9, np.inf, np.nan], ids=["3e9", "inf", "nan"])
def test_undist_set_refuses_entries_no_int_holds(bad, axis):
    """(int) of 3e9f or of an infinity is INT_MIN on the host: the former test `(int)x + 1 < wOrg` let such an entry through to the kernel's index arithmetic"""
    w, h = 72, 40
    rx, ry = radial_remap(w, h, WO, HO)
    (rx if axis == "x" else ry)[5, 5] = bad
    assert rx[5, 5] >= 0 or axis == "x"                                      # in y: under a valid x
    c = context(w, h)
    try:
        with pytest.raises(binding.NaloError, match="remap entry outside"):
            c.undist_set(WO, HO, None, None, 0, rx, ry)
        with pytest.raises(binding.NaloError, match="has not run"):         # and nothing was set
            c.frame_upload_raw(0, np.zeros((HO, WO), np.uint8))
    finally:
        c.close()


def test_undist_set_refuses_the_last_column_and_row():
    w, h = 72, 40
    c = context(w, h)
    try:
        for axis, v in (("x", WO - 1), ("x", WO - 0.5), ("y", HO - 1), ("y", 1e6), ("y", -1.0)):
            rx, ry = radial_remap(w, h, WO, HO)
            (rx if axis == "x" else ry)[h - 1, w - 1] = v
            with pytest.raises(binding.NaloError, match="remap entry outside"):
                c.undist_set(WO, HO, None, None, 0, rx, ry)
    finally:
        c.close()


def test_16_bit_frame_needs_a_16_bit_response():
    w, h = 72, 40
    rx, ry = radial_remap(w, h, WO, HO)
    raw = np.random.RandomState(3).randint(0, 65536, (HO, WO)).astype(np.uint16)
    c = context(w, h)
    try:
        c.undist_set(WO, HO, response(256), None, 1, rx, ry)
        with pytest.raises(binding.NaloError, match="error %d.*16-bit" % ERR_ARG):
            c.frame_upload_raw(0, raw, exposure=0.02)
        c.frame_upload_raw(0, raw, exposure=0.0, factor=0.25)                # without the photometric part the response is not indexed
        assert same_bits(c.frame_download(0, 0)[0][:, 0], orc.undistort(raw, None, None, 0, 0.25, rx, ry, w, h))
    finally:
        c.close()


def test_refused_undist_set_has_no_side_effects():
    """a refused call leaves the tables of the last accepted one: the next frame gives the same pyramid bit for bit. The bad entry is a finite one that every
    version of the check refuses, so that this test is about the order of check and copy alone."""
    w, h, levels = 72, 40, 4
    rx, ry, taps = planted_remap(w, h, WO, HO)
    G, vinv = response(256), vignette_inv(WO, HO)
    raw = raw_image(np.uint8, WO, HO, taps, seed=5)
    c = context(w, h, levels)
    try:
        c.undist_set(WO, HO, G, vinv, 2, rx, ry)
        c.frame_upload_raw(0, raw, exposure=0.02)
        before = gpu_pyramid(c, 0)
        assert_pyramids_equal(before, orc_pyramid(orc.undistort(raw, G, vinv, 2, 1.0, rx, ry, w, h), levels), "before")
        bad = rx.copy(); bad[20, 30] = 400.0
        with pytest.raises(binding.NaloError, match="remap entry outside"):
            c.undist_set(WO, HO, response(256, seed=8), (vinv * np.float32(1.5)).astype(np.float32), 2, bad, ry)
        c.frame_upload_raw(0, raw, exposure=0.02)                            # uses the first call's tables, all of them
        assert_pyramids_equal(gpu_pyramid(c, 0), before, "after the refused call")
    finally:
        c.close()
