"""Host model of the DEVICE SCHEME of the candidate-pixel selection (kernels_pixsel.hip), numpy only. It does not walk the image like PixelSelector::select
(oracle/orc_pixsel.c does): it restates what the kernels do, so that the scheme itself - not only its result - can be questioned on the CPU:

  slot    one cell of potential `pot`; slots are numbered in scan order: 16 per 4pot block (2pot block b3 = c >> 2, cell c2 = c & 3, both row-major inside
          their parent), 4pot blocks row-major over the image
  has     the cell holds a pixel above its block threshold (the speculative "this cell selects")
  sel[d]  ... and one of them has a non-zero |gx*dx + gy*dy| along direction d (float32, one rounding per operation, no contraction)
  rounds  flags = has; repeat { pre = exclusive scan(flags); new = sel[slot][rp[pre] & 15]; stop when new == flags; flags = new }: one round per pass of
          the selection kernel, the confirming one included
  levels  at the fixed point: the cell's pixel = first strict maximum of the projected gradient in raster order (L lanes walk runs of per = ceil(tot / L)
          pixels and are combined in lane order); a 2pot block selects its level-2 pixel iff none of its cells selected, a 4pot block its level-3 pixel
          iff nothing below it selected, directions drawn with the count at the block's first slot

Besides the map it counts what the lane merges exist for: maxima attained in two lanes' runs (level 1), in two cells of a 2pot block (level 2), in two cells
and in two 2pot blocks (the four waves of the 16-lane class) of a 4pot block (level 3)."""
import numpy as np

F = np.float32
DIRS = np.array([[0, 1.0000], [0.3827, 0.9239], [0.1951, 0.9808], [0.9239, 0.3827], [0.7071, 0.7071], [0.3827, -0.9239], [0.8315, 0.5556], [0.8315, -0.5556],
                 [0.5556, -0.8315], [0.9808, 0.1951], [0.9239, -0.3827], [0.7071, -0.7071], [0.5556, 0.8315], [0.9808, -0.1951], [1.0000, 0.0000],
                 [0.1951, -0.9808]], F)                    # PixelSelector2.cpp:581-597
DW1 = F(0.75)                                              # setting_gradDownweightPerLevel
DW2 = F(DW1 * DW1)


def lanes(pot):
    """lanes that share a cell"""
    return 1 if pot <= 3 else (4 if pot <= 7 else 16)


def ths_len(w, h):
    """floats of one threshold buffer: the reference's (w/32)*(h/32) + 100, or what the largest index select() forms needs, (h/32)*(w/32) + ((w-1) >> 5)"""
    return (w // 32) * (h // 32) + max(100, w // 32 + 1)


class Tables:
    """everything that does not depend on randomPattern: the per-pixel geometry in (slot, raster position) order, candidates, has and sel"""

    def __init__(self, dI, ag0, ag1, ag2, w, h, thsSmoothed, pot, thFactor):
        self.w, self.h, self.pot, self.L = w, h, pot, lanes(pot)
        tf = F(thFactor)
        ths = np.zeros(ths_len(w, h), F)
        ths[:len(thsSmoothed)] = thsSmoothed
        ys, xs = np.mgrid[0:h, 0:w]
        nb4x, nb4y = -(-w // (4 * pot)), -(-h // (4 * pot))
        self.nslots = nb4x * nb4y * 16
        rx, ry = xs % (4 * pot), ys % (4 * pot)
        b3 = (ry // (2 * pot)) * 2 + rx // (2 * pot)
        c2 = ((ry % (2 * pot)) // pot) * 2 + (rx % (2 * pot)) // pot
        slot = ((ys // (4 * pot)) * nb4x + xs // (4 * pot)) * 16 + b3 * 4 + c2
        px, py = xs % pot, ys % pot
        mx, my = np.minimum(pot, w - (xs - px)), np.minimum(pot, h - (ys - py))
        p = py * mx + px
        per = -(-(mx * my) // self.L)
        valid = ~((xs < 4) | (xs >= w - 5) | (ys < 4) | (ys > h - 4))
        th0 = ths[(xs >> 5) + (ys >> 5) * (w // 32)]
        th1 = th0 * DW1
        th2 = th1 * DW2
        a0 = np.asarray(ag0, F).reshape(h, w)
        a1 = np.asarray(ag1, F).reshape(h // 2, w // 2)[np.minimum(ys // 2, h // 2 - 1), np.minimum(xs // 2, w // 2 - 1)]
        a2 = np.asarray(ag2, F).reshape(h // 4, w // 4)[np.minimum(ys // 4, h // 4 - 1), np.minimum(xs // 4, w // 4 - 1)]
        order = np.lexsort((p.reshape(-1), slot.reshape(-1)))
        g = lambda a: a.reshape(-1)[order]
        dI = np.asarray(dI, F).reshape(h * w, -1)
        self.pix, self.slot, self.lane = order, g(slot), g(p // per)
        self.gx, self.gy = dI[order, 1], dI[order, 2]
        self.c = [g(valid & (a0 > th0 * tf)), g(valid & (a1 > th1 * tf)), g(valid & (a2 > th2 * tf))]
        self.has = np.bincount(self.slot[self.c[0]], minlength=self.nslots) > 0
        self.sel = np.zeros((self.nslots, 16), bool)
        for d in range(16):
            nz = self.c[0] & (self.proj(np.full(len(order), d)) != 0)
            self.sel[:, d] = np.bincount(self.slot[nz], minlength=self.nslots) > 0

    def proj(self, d):
        return np.abs(self.gx * DIRS[d, 0] + self.gy * DIRS[d, 1])


def _first_max(group, ngroups, v, key):
    """per group of the (slot, raster)-ordered pixels: the maximum of v, the position of its first occurrence (-1 without a positive value) and whether
    the maximum is attained under two different keys"""
    top = np.zeros(ngroups, F)
    np.maximum.at(top, group, v)
    at = np.flatnonzero((v == top[group]) & (v > 0))
    first = np.full(ngroups, -1, np.int64)
    gs, i = np.unique(group[at], return_index=True)
    first[gs] = at[i]
    lo, hi = np.full(ngroups, np.iinfo(np.int64).max), np.full(ngroups, -1, np.int64)
    np.minimum.at(lo, group[at], key[at])
    np.maximum.at(hi, group[at], key[at])
    return first, hi > lo


def run(T, rp):
    """-> dict(map [h,w] float32 0/1/2/4, n [3], flags, rounds, span_lanes, span_cells2, span_cells3, span_blocks3)"""
    rp = np.asarray(rp, np.uint8)
    idx = np.arange(T.nslots)
    flags, rounds = T.has.copy(), 0
    while True:
        pre = np.cumsum(flags) - flags
        new = T.sel[idx, rp[pre] & 15]
        rounds += 1
        if np.array_equal(new, flags):
            break
        flags = new
    m = np.zeros(T.w * T.h, F)
    # level 1
    v = np.where(T.c[0], T.proj(rp[pre[T.slot]] & 15), F(0))
    k2, span1 = _first_max(T.slot, T.nslots, v, T.lane)
    s2 = k2 >= 0
    assert np.array_equal(s2, flags)
    m[T.pix[k2[s2]]] = 1
    # level 2: the 2pot blocks none of whose cells selected
    g2, n2 = T.slot >> 2, T.nslots // 4
    v = np.where(T.c[1], T.proj(rp[pre[T.slot & ~3]] & 15), F(0))
    k3, span2 = _first_max(g2, n2, v, T.slot)
    s3 = (k3 >= 0) & ~s2.reshape(n2, 4).any(1)
    m[T.pix[k3[s3]]] = 2
    # level 3: the 4pot blocks with nothing below
    g4, n4 = T.slot >> 4, T.nslots // 16
    v = np.where(T.c[2], T.proj(rp[pre[T.slot & ~15]] & 15), F(0))
    k4, span3 = _first_max(g4, n4, v, T.slot)
    _, span3b = _first_max(g4, n4, v, g2)
    s4 = (k4 >= 0) & ~s2.reshape(n4, 16).any(1) & ~s3.reshape(n4, 4).any(1)
    m[T.pix[k4[s4]]] = 4
    return dict(map=m.reshape(T.h, T.w), n=np.array([s2.sum(), s3.sum(), s4.sum()], np.int32), flags=flags, rounds=rounds,
                span_lanes=int((span1 & s2).sum()), span_cells2=int((span2 & s3).sum()), span_cells3=int((span3 & s4).sum()),
                span_blocks3=int((span3b & s4).sum()))
