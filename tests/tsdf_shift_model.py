"""The literal model of nalo_tsdf_shift and its host helpers (include/nalo_gpu.h, "A volume that follows the camera"): the shift as a triple loop and as array
slices, both on uint32 views so that bits are compared; the origin formula in float32; nalo_tsdf_shift_for in float64; nalo_tsdf_shift_boxes, and the brute-force
sets of cells its property is stated on. No device."""
import numpy as np

F = np.float32
U = np.uint32
ONE, ZERO = U(0x3F800000), U(0)                        # the initial words: tsdf 1.0f, weight and colour 0.0f
MAX_BASE = 1 << 24


def words(a):
    """the uint32 view of a float32 array: a copy, contiguous, the same bits"""
    return np.ascontiguousarray(a, F).view(U).copy()


def shift_literal(src, s, init):
    """src: uint32 [nz][ny][nx]; out[k][j][i] = src[k + s2][j + s1][i + s0] where that lies in the grid, else init"""
    nz, ny, nx = src.shape
    out = np.empty_like(src)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                a, b, c = i + int(s[0]), j + int(s[1]), k + int(s[2])
                out[k, j, i] = src[c, b, a] if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz else init
    return out


def shift_words(src, s, init):
    """the same on slices: per axis the kept destination range [max(-s, 0), n - max(s, 0)) takes the source range moved by s"""
    out = np.full_like(src, init)
    dst_sl, src_sl = [], []
    for ax, sa in zip((2, 1, 0), (int(s[0]), int(s[1]), int(s[2]))):            # array axis 2 is x
        n = src.shape[ax]
        lo, hi = max(-sa, 0), n - max(sa, 0)
        if lo >= hi:
            return out
        dst_sl.append((ax, slice(lo, hi)))
        src_sl.append((ax, slice(lo + sa, hi + sa)))
    d, r = [None] * 3, [None] * 3
    for (ax, a), (_, b) in zip(dst_sl, src_sl):
        d[ax], r[ax] = a, b
    out[tuple(d)] = src[tuple(r)]
    return out


def shift_volume(vol, s, fn=shift_words):
    """nalo_tsdf_shift on a model volume (tests/tsdf_model.py's dict; 'colour': float32 [3][nz][ny][nx] when coloured, 'origin0' and 'base' are added on the first
    call): the arrays, base and origin in place"""
    if "origin0" not in vol:
        vol["origin0"], vol["base"] = vol["origin"].astype(F).copy(), np.zeros(3, np.int64)
    vol["tsdf"] = fn(words(vol["tsdf"]), s, ONE).view(F)
    vol["weight"] = fn(words(vol["weight"]), s, ZERO).view(F)
    if vol.get("colour") is not None:
        vol["colour"] = np.stack([fn(words(vol["colour"][X]), s, ZERO) for X in range(3)]).view(F)
    vol["base"] = vol["base"] + np.asarray(s, np.int64)
    vol["origin"] = origin(vol["origin0"], vol["base"], vol["vs"])
    return vol


def origin(origin0, base, vs):
    """origin0[a] + (float)base[a] * voxel_size in float32: the product rounded, then the sum"""
    o0 = np.asarray(origin0, F)
    step = np.asarray(base, np.int64).astype(F) * F(vs)
    assert step.dtype == F
    out = o0 + step
    assert out.dtype == F
    return out


def shift_refusal(origin0, base, s, vs):
    """True where nalo_tsdf_shift refuses: |base + s| beyond 2^24 or an origin that is not finite"""
    b = np.asarray(base, np.int64) + np.asarray(s, np.int64)
    if (np.abs(b) > MAX_BASE).any():
        return True
    with np.errstate(all="ignore"):
        return not np.isfinite(origin(origin0, b, vs)).all()


def shift_for(origin_now, vs, dims, centre, margin):
    """nalo_tsdf_shift_for in float64; None where it refuses for the centre, the margin or the distance (the descriptor is the caller's to check)"""
    out = []
    with np.errstate(all="ignore"):
        for a in range(3):
            c = np.float64(centre[a])
            if not np.isfinite(c) or int(margin[a]) < 0:
                return None
            q = np.floor((c - np.float64(F(origin_now[a]))) / np.float64(F(vs)))
            d = q - np.float64(int(dims[a]) // 2)
            if not abs(d) <= MAX_BASE:
                return None
            out.append(int(d) if abs(d) > int(margin[a]) else 0)
    return tuple(out)


def shift_boxes(dims, s):
    """nalo_tsdf_shift_boxes: dict(boxes=[(lo, size)], kept_lo, kept_size), voxel indices in (x, y, z) order"""
    n, s = [int(v) for v in dims], [int(v) for v in s]
    if any(abs(s[a]) >= n[a] for a in range(3)):
        return dict(boxes=[((0, 0, 0), tuple(n))], kept_lo=(0, 0, 0), kept_size=(0, 0, 0))
    kept = [(s[a], n[a] - s[a]) if s[a] > 0 else (0, n[a] + s[a]) for a in range(3)]                   # (lo, size)
    leave = [(0, min(s[a] + 1, n[a])) if s[a] > 0 else (max(n[a] + s[a] - 1, 0), n[a] - max(n[a] + s[a] - 1, 0)) if s[a] < 0 else None for a in range(3)]
    boxes = []
    for b in range(3):
        if leave[b] is None:
            continue
        rng = [kept[a] if a < b else leave[a] if a == b else (0, n[a]) for a in range(3)]
        if all(r[1] >= 1 for r in rng):
            boxes.append((tuple(r[0] for r in rng), tuple(r[1] for r in rng)))
    return dict(boxes=boxes, kept_lo=tuple(k[0] for k in kept), kept_size=tuple(k[1] for k in kept))


def cells_of_box(lo, size):
    """the cells (by their lowest corner) whose eight corners lie in the sub-box of voxels [lo, lo + size)"""
    return {(i, j, k) for i in range(lo[0], lo[0] + size[0] - 1) for j in range(lo[1], lo[1] + size[1] - 1) for k in range(lo[2], lo[2] + size[2] - 1)}


def lost_cells(dims, s):
    """by brute force: the cells of the grid with a corner voxel that is not kept"""
    n = [int(v) for v in dims]
    keep = [set(range(max(int(s[a]), 0), n[a] + min(int(s[a]), 0))) for a in range(3)]
    out = set()
    for c in cells_of_box((0, 0, 0), n):
        if not all(c[a] in keep[a] and c[a] + 1 in keep[a] for a in range(3)):
            out.add(c)
    return out


def random_words(rng, shape):
    """seeded words of every kind: any bit pattern, with NaN payloads (quiet and signalling), infinities, -0.0f and denormals planted among them"""
    w = rng.randint(0, 2 ** 32, shape, dtype=np.uint64).astype(U)
    flat = w.reshape(-1)
    special = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x3F800000, 0x00000000], U)
    at = rng.randint(0, flat.size, min(flat.size, 2 * len(special)))
    flat[at] = special[np.arange(len(at)) % len(special)]
    return w
