"""Scenes, random tables, masks and draws for the pixel-selection edge tests (test_pixsel_cpu.py, test_pixsel_edges_gpu.py). numpy + the CPU oracle; no GPU.

The scene has four bands, left to right by quarter of the width: uniform noise 80..120 | vertical stripes (dy == 0 exactly, whole rows tie, a cell whose
drawn direction is (0,1) sees no gradient) | a triangle wave in y of slope 6 (too flat for level 0, steep enough at level 1: level-2 selections) | a
triangle wave of slope 3 in x plus slope 3 in y (level-3 selections, and identical gradients all over: exact ties across cells and 2pot blocks)."""
import functools

import numpy as np

import orc
import pixsel_model as model

F = np.float32
SHAPES = [(104, 72), (96, 64), (264, 168)]
POTS = {(104, 72): [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 40], (96, 64): [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 40], (264, 168): [8, 9, 12, 16, 17, 23]}
THFACTORS = [1.0, 2.0]
TABLES = ["libc", "zero", "alt_0_14", "third_16", "mod256"]
MASKS = ["zero", "single", "const37", "random", "top_bins", "fractions"]
WIDE = (3232, 48)                                          # w/32 > 100 and h % 32 != 0: select() indexes past the reference's (w/32)*(h/32) + 100 thresholds
RESIDUES = [0, 9, 10, 11, 499, 500, 501, 599, 600, 601, 999]


def _tri(t, period, slope):
    return slope * np.abs(t % (2 * period) - period)


@functools.lru_cache(maxsize=None)
def scene(w, h):
    if (w, h) == WIDE:                                     # noise, the four bands at both ends: a stripe band a quarter of this width costs > 2000 rounds
        img = np.random.RandomState(12).randint(80, 121, size=(h, w)).astype(F)
        img[:, :256] = scene(256, h)
        img[:, -256:] = scene(256, h)
        img.setflags(write=False)
        return img
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    q = w // 4
    img = np.random.RandomState(11).randint(80, 121, size=(h, w)).astype(F)
    img[:, q:2 * q] = (100 + 60 * ((x[:, q:2 * q] // 3) % 2)) + 0 * y
    img[:, 2 * q:3 * q] = 60 + _tri(y, 12, 6) + 0 * x[:, 2 * q:3 * q]
    img[:, 3 * q:] = 40 + _tri(x[:, 3 * q:], 16, 3) + _tri(y, 16, 3)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def images(w, h):
    """(dI0 [w*h,3], absSquaredGrad of levels 0, 1, 2) of the scene, from the oracle's pyramid"""
    dI, ab = orc.make_images(scene(w, h), 3)
    o1, o2 = w * h, w * h + (w // 2) * (h // 2)
    return dI[:o1], ab[:o1], ab[o1:o2], ab[o2:o2 + (w // 4) * (h // 4)]


@functools.lru_cache(maxsize=None)
def thresholds(w, h):
    return orc.pixsel_make_hists(images(w, h)[1], w, h)[1]


@functools.lru_cache(maxsize=None)
def table(name, n):
    """randomPattern[n]"""
    i = np.arange(n)
    if name == "libc":
        rp = orc.pixsel_libc_tables(n)[0]
    elif name == "zero":
        rp = np.zeros(n, np.uint8)
    elif name == "alt_0_14":                               # directions (0,1) and (1,0) alternating with the running count
        rp = np.where(i % 2 == 0, 0, 14).astype(np.uint8)
    elif name == "third_16":                               # 16 & 15 = 0: the high bits are not part of the direction
        rp = np.where(i % 3 == 0, 16, 14).astype(np.uint8)
    else:
        assert name == "mod256"
        rp = (i % 256).astype(np.uint8)
    rp.setflags(write=False)
    return rp


@functools.lru_cache(maxsize=None)
def mask(name, w, h):
    rng = np.random.RandomState(5)
    m = np.zeros((h, w), F)
    if name == "single":
        m[h // 2, w // 2] = 90
    elif name == "const37":
        m[:] = 37
    elif name == "random":                                 # test_pixsel_gpu.py's: 0 = no lidar return
        m[h // 3:, :] = rng.randint(0, 200, size=(h - h // 3, w))
        m[:, :w // 5] = 0
    elif name == "top_bins":                               # 255, and 256 = the clamp bin the quantile loop reads as 0
        m[:] = rng.randint(0, 257, size=(h, w))
        m[::7, ::5] = 255
        m[3::7, 2::5] = 256
    elif name == "fractions":                              # (int)0.5 = 0: counted twice in bin 0
        m[:] = rng.randint(0, 200, size=(h, w))
        m[::3, ::4] = 0.5
        m[1::3, 1::4] = 199.75
    else:
        assert name == "zero"
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def draws(name, n):
    """the rand() stream of FusedWithMask: libc's, or every residue mod 1000 that sits on or next to a comparison of the fuse kernel, under varying high parts"""
    if name == "libc":
        return orc.pixsel_libc_tables(n)[1]
    i = np.arange(n, dtype=np.int64)
    d = (np.array(RESIDUES)[(i + i // len(RESIDUES)) % len(RESIDUES)] + 1000 * ((i * 7919) % 2000003)).astype(np.int32)
    d.setflags(write=False)
    return d


def select_cases():
    """(w, h, pot, thFactor, table) of every selection the GPU test runs"""
    return [(w, h, pot, thf, t) for (w, h) in SHAPES for pot in POTS[(w, h)] for thf in THFACTORS for t in TABLES] + [WIDE + (3, 1.0, "alt_0_14")]


@functools.lru_cache(maxsize=None)
def model_tables(w, h, pot, thf):
    return model.Tables(*images(w, h), w, h, thresholds(w, h), pot, thf)


@functools.lru_cache(maxsize=None)
def oracle_select(w, h, pot, thf, t):
    return orc.pixsel_select(*images(w, h), w, h, thresholds(w, h), table(t, w * h), pot, thf)


FUSE_SELECTIONS = [(104, 72, 1, "mod256"), (264, 168, 8, "libc")]          # (w, h, pot, table) of the selections the fusion runs on, thFactor 1


def fuse_cases():
    """(w, h, pot, table, mask, draws): every mask under the crafted draws, and libc's draws on the two masks with the widest histograms"""
    return [s + (m, "crafted") for s in FUSE_SELECTIONS for m in MASKS] + [s + (m, "libc") for s in FUSE_SELECTIONS for m in ("random", "top_bins")]


def make_maps_cases():
    """(w, h, table, density, entry potential, recursionsLeft, thFactor) of nalo_pixsel_make_maps: densities that drive the potential up from 3 into the
    16-lane class and down from 9 (and from 40, in two steps) into the 1-lane class, every recursion budget, and quotia on either side of 0.95"""
    out = []
    for (w, h) in [(104, 72), (264, 168)]:
        n3, n9, n40 = (int(oracle_select(w, h, p, 1.0, "mod256")[1].sum()) for p in (3, 9, 40))
        n3f2 = int(oracle_select(w, h, 3, 2.0, "libc")[1].sum())
        down = 30.0 if w * h < 10000 else 6.0              # 9 -> 1 on the small frame, 9 -> 3 on the large one (its potential 1 needs ~4000 rounds)
        for rec in (0, 1, 2, 3):
            out += [(w, h, "mod256", 0.04 * n3, 3, rec, 1.0), (w, h, "mod256", down * n9, 9, rec, 1.0), (w, h, "mod256", 30.0 * n40, 40, rec, 1.0),
                    (w, h, "libc", 0.5 * n3f2, 3, rec, 2.0)]
        out += [(w, h, "mod256", density_at_quotia(n3, True), 3, 0, 1.0), (w, h, "mod256", density_at_quotia(n3, False), 3, 0, 1.0)]
    return [(w, h, t, float(F(d)), p, r, f) for (w, h, t, d, p, r, f) in out]


def make_maps_trace(w, h, t, density, pot, rec, thf):
    """makeMaps' potential adaptation (PixelSelector2.cpp:180-228) on the oracle's counts -> (potentials selected at, quotia of the last, its count)"""
    density, cur, visited = F(density), pot, []
    while True:
        visited.append(cur)
        n = F(oracle_select(w, h, cur, thf, t)[1].sum())
        quotia = F(density / n)
        ideal = max(int(np.sqrt(F(F(n * F(cur + 1)) * F(cur + 1)) / density, dtype=F) - F(1)), 1)
        if rec > 0 and quotia > 1.25 and cur > 1:
            cur, rec = min(ideal, cur - 1), rec - 1
        elif rec > 0 and quotia < 0.25:
            cur, rec = max(ideal, cur + 1), rec - 1
        else:
            return visited, float(quotia), int(n)


def density_at_quotia(n, above):
    """the float32 density next to 0.95 * n on either side of makeMaps' `quotia < 0.95` (float quotient, double literal)"""
    d = F(0.95 * n)
    while float(F(d / F(n))) < 0.95:
        d = np.nextafter(d, F(np.inf))
    while float(F(d / F(n))) >= 0.95:
        d = np.nextafter(d, F(-np.inf))
    return float(np.nextafter(d, F(np.inf)) if above else d)
