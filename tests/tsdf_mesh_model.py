"""The literal model of nalo_tsdf_mesh (include/nalo_gpu.h, "The mesh"): marching tetrahedra on the Kuhn split of every cell, one voxel and one cell at a time
in the defined order, in float32; the triangle table built from the header's winding rule on real midpoints (never copied from the library's); a vectorised
form of the same operations for the larger grids; the checks a closed oriented surface passes; a PLY writer. Volumes are tests/tsdf_model.py's. No device."""
import struct

import numpy as np

import tsdf_model as tm

F = np.float32
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))


def bits(b):
    return np.array([b & 1, (b >> 1) & 1, (b >> 2) & 1])


def tet_polygons(mask):
    """the triangles of one tetrahedron as edges (r, r') between corner positions r = 0..3, before the winding test"""
    ins = [r for r in range(4) if (mask >> r) & 1]
    outs = [r for r in range(4) if not (mask >> r) & 1]
    if not ins or not outs:
        return []
    if len(ins) == 1 or len(outs) == 1:
        lone, others = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
        return [[(lone, o) for o in others]]
    q = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


def build_table():
    """int8 [6][16][6]: per tetrahedron and mask up to two triangles, a vertex coded 8 p + (q ^ p), -1 padding. The winding is decided on the midpoints of the
    edges in the unit cube, in float64: kept when the normal looks from the inside corners' mean to the outside corners' mean"""
    tab = np.full((6, 16, 6), -1, np.int8)
    for t, tet in enumerate(TETS):
        corner = [bits(b).astype(np.float64) for b in tet]
        for mask in range(16):
            ins = [corner[r] for r in range(4) if (mask >> r) & 1]
            outs = [corner[r] for r in range(4) if not (mask >> r) & 1]
            for s, poly in enumerate(tet_polygons(mask)):
                mid = [0.5 * (corner[a] + corner[b]) for a, b in poly]
                code = []
                for a, b in poly:
                    p, q = sorted((tet[a], tet[b]))
                    assert p & q == p
                    code.append(8 * p + (q ^ p))
                d = float(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), np.mean(outs, 0) - np.mean(ins, 0)))
                assert abs(d) > 1e-9
                if d < 0:
                    code[1], code[2] = code[2], code[1]
                tab[t, mask, 3 * s:3 * s + 3] = code
    return tab


TABLE = build_table()


def _box(vol, lo, size):
    nx, ny, nz = vol["dims"]
    lo = (0, 0, 0) if lo is None else tuple(int(v) for v in lo)
    size = (nx, ny, nz) if size is None else tuple(int(v) for v in size)
    return lo, size


def mesh_literal(vol, min_weight, lo=None, size=None):
    """(xyz float32 [nv][3], tri int32 [nt][3], owner [nv] = (i, j, k, m) of every vertex): every voxel, then every cell, in the defined order"""
    lo, size = _box(vol, lo, size)
    cs, T, W, mw, vs = tm.centres(vol), vol["tsdf"], vol["weight"], F(min_weight), vol["vs"]
    hi = tuple(lo[a] + size[a] for a in range(3))

    def valid(i, j, k):
        return bool(W[k, j, i] >= mw) and not np.isnan(T[k, j, i])

    def inside(i, j, k):
        return bool(T[k, j, i] < 0)

    index, xyz, owner = {}, [], []
    with np.errstate(all="ignore"):
        for k in range(lo[2], hi[2]):
            for j in range(lo[1], hi[1]):
                for i in range(lo[0], hi[0]):
                    if not valid(i, j, k):
                        continue
                    for m in range(1, 8):
                        d = bits(m)
                        n = (i + d[0], j + d[1], k + d[2])
                        if n[0] >= hi[0] or n[1] >= hi[1] or n[2] >= hi[2] or not valid(*n) or inside(i, j, k) == inside(*n):
                            continue
                        t0, t1 = T[k, j, i], T[n[2], n[1], n[0]]
                        s = t0 / (t0 - t1)
                        prod = vs * s
                        p = [cs[0][i], cs[1][j], cs[2][k]]
                        for a in range(3):
                            if d[a]:
                                p[a] = p[a] + prod
                        index[(i, j, k, m)] = len(xyz)
                        xyz.append(p)
                        owner.append((i, j, k, m))
    tri = []
    for k in range(lo[2], hi[2] - 1):
        for j in range(lo[1], hi[1] - 1):
            for i in range(lo[0], hi[0] - 1):
                corner = [(i + (b & 1), j + ((b >> 1) & 1), k + ((b >> 2) & 1)) for b in range(8)]
                if not all(valid(*c) for c in corner):
                    continue
                for t, tet in enumerate(TETS):
                    mask = sum(1 << r for r in range(4) if inside(*corner[tet[r]]))
                    row = TABLE[t, mask]
                    for s in (0, 3):
                        if row[s] < 0:
                            break
                        tri.append([index[corner[int(c) >> 3] + (int(c) & 7,)] for c in row[s:s + 3]])
    return np.array(xyz, F).reshape(-1, 3), np.array(tri, np.int32).reshape(-1, 3), owner


def mesh(vol, min_weight, lo=None, size=None, with_axis=False):
    """the same operations on whole arrays: (xyz, tri), with_axis: also the edge m of every vertex"""
    lo, size = _box(vol, lo, size)
    sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
    T, W, mw, vs = vol["tsdf"][sl], vol["weight"][sl], F(min_weight), vol["vs"]
    cs = tm.centres(vol)
    sz, sy, sx = T.shape
    cen = [cs[0][lo[0]:lo[0] + sx][None, None, :], cs[1][lo[1]:lo[1] + sy][None, :, None], cs[2][lo[2]:lo[2] + sz][:, None, None]]
    with np.errstate(all="ignore"):
        valid = (W >= mw) & ~np.isnan(T)
        inside = T < 0
        keys, parts = [], []                                                    # per edge m: 8 * (the voxel's position in the sub-box) + m, and the positions
        for m in range(1, 8):
            d = bits(m)
            if sx - d[0] < 1 or sy - d[1] < 1 or sz - d[2] < 1:
                continue
            s0 = (slice(0, sz - d[2]), slice(0, sy - d[1]), slice(0, sx - d[0]))
            s1 = (slice(d[2], sz), slice(d[1], sy), slice(d[0], sx))
            z, y, x = np.nonzero(valid[s0] & valid[s1] & (inside[s0] != inside[s1]))
            if len(z) == 0:
                continue
            t0, t1 = T[z, y, x], T[z + d[2], y + d[1], x + d[0]]
            prod = vs * (t0 / (t0 - t1))
            p = np.stack([cen[0][0, 0, x], cen[1][0, y, 0], cen[2][z, 0, 0]], 1)
            for a in range(3):
                if d[a]:
                    p[:, a] = p[:, a] + prod
            assert p.dtype == F
            keys.append(((z.astype(np.int64) * sy + y) * sx + x) * 8 + m)
            parts.append(p)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    order = np.argsort(keys, kind="stable")                                     # ascending (k, j, i) of the voxel, then m
    keys = keys[order]
    xyz = (np.concatenate(parts)[order] if parts else np.zeros((0, 3), F)).reshape(-1, 3)
    tri = np.zeros((0, 3), np.int32)
    if min(sx, sy, sz) >= 2:
        cz, cy, cx = sz - 1, sy - 1, sx - 1
        live = np.ones((cz, cy, cx), bool)
        ins8 = np.zeros((cz, cy, cx), np.int32)
        for b in range(8):
            d = bits(b)
            s = (slice(d[2], d[2] + cz), slice(d[1], d[1] + cy), slice(d[0], d[0] + cx))
            live &= valid[s]
            ins8 |= inside[s].astype(np.int32) << b
        z, y, x = np.nonzero(live & (ins8 != 0) & (ins8 != 255))               # C order: ascending (k, j, i)
        ins = ins8[z, y, x]
        out = np.full((len(z), 6, 2, 3), -1, np.int64)
        for t, tet in enumerate(TETS):
            mask = sum(((ins >> tet[r]) & 1) << r for r in range(4))
            for s in range(2):
                codes = TABLE[t][mask][:, 3 * s:3 * s + 3].astype(np.int64)     # [cells][3]
                ok = codes[:, 0] >= 0
                for k in range(3):
                    p, m = codes[ok, k] >> 3, codes[ok, k] & 7
                    want = (((z[ok] + ((p >> 2) & 1)) * sy + y[ok] + ((p >> 1) & 1)) * sx + x[ok] + (p & 1)) * 8 + m
                    at = np.searchsorted(keys, want)
                    assert (keys[at] == want).all()                             # the vertex a triangle names exists
                    out[ok, t, s, k] = at
        out = out.reshape(-1, 3)
        tri = out[out[:, 0] >= 0].astype(np.int32)
    if with_axis:
        return xyz, tri, (keys & 7)
    return xyz, tri


# ------------------------------------------------------------------------------------------------ what a closed, oriented surface passes
def directed_edges(tri):
    t = np.asarray(tri, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_and_oriented(tri):
    """every directed edge occurs exactly once and its reverse exactly once"""
    e = directed_edges(tri)
    if len(e) == 0:
        return False
    n = int(e.max()) + 1
    fwd, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    u, cnt = np.unique(fwd, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(u, np.unique(rev)))


def signed_volume(xyz, tri):
    p = np.asarray(xyz, np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def sphere(n=12, radius=3.6, vs=0.25, complement=False):
    """a volume of n^3 voxels holding the signed distance to a sphere around its centre (negative inside), every voxel valid"""
    vol = tm.volume((-0.5 * n * vs,) * 3, vs, (n, n, n), 1.0, 4.0)
    c = tm.centres(vol)
    r = np.sqrt(c[0][None, None, :].astype(np.float64) ** 2 + c[1][None, :, None].astype(np.float64) ** 2 + c[2][:, None, None].astype(np.float64) ** 2)
    sd = (r - radius * vs).astype(F)
    vol["tsdf"][:] = -sd if complement else sd
    vol["weight"][:] = 1.0
    return vol


def write_ply(path, xyz, tri):
    """binary_little_endian 1.0, float x y z, list uchar int vertex_indices"""
    x, t = np.asarray(xyz, "<f4").reshape(-1, 3), np.asarray(tri, "<i4").reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(x), len(t)))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(x.tobytes())
        for row in t:
            f.write(struct.pack("<Biii", 3, int(row[0]), int(row[1]), int(row[2])))


def same_floats(a, b):
    """bit for bit, except that a NaN equals a NaN whatever its payload"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
