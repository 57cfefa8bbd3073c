"""The literal model of the mesh archive (include/nalo_gpu.h, "The mesh archive"): a Python dict from key to index and the lists of positions, colours, keys
and triangles, fed with pieces that tests/tsdf_mesh_model.py (and tests/tsdf_color_model.py) evaluate on a model volume with its current origin; the key of every
vertex recomputed from the mesh definition; a vectorised archive with the same interface for the larger grids; the loop nalo_tsdf_follow is defined as. No device."""
import numpy as np

import tsdf_color_model as cm
import tsdf_mesh_model as mm

F = np.float32


def base_of(vol):
    return np.asarray(vol.get("base", np.zeros(3, np.int64)), np.int64)


def owners(vol, min_weight, lo=None, size=None):
    """int64 [nv][4] = (i, j, k, m) of every vertex of the sub-box's mesh, in the mesh's order: ascending (k, j, i) of the owning voxel (grid indices), then m.
    Written from the definition: (v, m) carries a vertex iff the far end lies inside the sub-box, both ends are valid and exactly one is inside"""
    lo, size = mm._box(vol, lo, size)
    sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
    T, W = vol["tsdf"][sl], vol["weight"][sl]
    with np.errstate(all="ignore"):
        valid, inside = (W >= F(min_weight)) & ~np.isnan(T), T < 0
    sz, sy, sx = T.shape
    rows = []
    for m in range(1, 8):
        d = mm.bits(m)
        if sx - d[0] < 1 or sy - d[1] < 1 or sz - d[2] < 1:
            continue
        s0 = (slice(0, sz - d[2]), slice(0, sy - d[1]), slice(0, sx - d[0]))
        s1 = (slice(d[2], sz), slice(d[1], sy), slice(d[0], sx))
        z, y, x = np.nonzero(valid[s0] & valid[s1] & (inside[s0] != inside[s1]))
        rows.append(np.stack([x + lo[0], y + lo[1], z + lo[2], np.full(len(z), m)], 1).astype(np.int64))
    out = np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)
    order = np.lexsort((out[:, 3], out[:, 0], out[:, 1], out[:, 2]))
    return out[order]


def keys_of(vol, min_weight, lo=None, size=None):
    """int32 [nv][4] = (gx, gy, gz, m): the owner's grid index plus the volume's base"""
    k = owners(vol, min_weight, lo, size)
    k[:, :3] += base_of(vol)[None, :]
    return k.astype(np.int32)


def piece(vol, min_weight, lo=None, size=None, colour=False):
    """what nalo_tsdf_archive_mesh appends: (xyz, tri, key, rgba or None) of the sub-box's mesh at the volume's current origin"""
    xyz, tri = mm.mesh(vol, min_weight, lo, size)
    key = keys_of(vol, min_weight, lo, size)
    assert len(key) == len(xyz)
    rgba = cm.mesh_colours(vol, min_weight, lo, size) if colour else None
    return xyz, tri, key, rgba


class Archive:
    """the definition, one vertex at a time: a dict from key to index and the lists"""

    def __init__(self, coloured=False):
        self.coloured, self.index, self.xyz, self.rgba, self.key, self.tri = coloured, {}, [], [], [], []

    def append(self, xyz, tri, key, rgba=None):
        """-> (vertices added, vertices welded, triangles added)"""
        assert (rgba is not None) == self.coloured and len(xyz) == len(key)
        remap, added = [], 0
        for v in range(len(xyz)):
            k = tuple(int(x) for x in key[v])
            at = self.index.get(k)
            if at is None:                                                      # new: at the end, words copied
                at = self.index[k] = len(self.xyz)
                self.xyz.append(np.array(xyz[v], F))
                self.key.append(k)
                if self.coloured:
                    self.rgba.append(np.array(rgba[v], np.uint8))
                added += 1
            remap.append(at)                                                    # held: the first occurrence wins
        for t in tri:
            self.tri.append([remap[int(i)] for i in t])
        return added, len(xyz) - added, len(tri)

    def arrays(self):
        return (np.array(self.xyz, F).reshape(-1, 3), np.array(self.tri, np.int32).reshape(-1, 3),
                np.array(self.rgba, np.uint8).reshape(-1, 4) if self.coloured else None, np.array(self.key, np.int32).reshape(-1, 4))


SPAN = 1 << 19                                                                  # the vectorised archive packs a key into one int64: |g| below 2^19 on every axis


def pack(key):
    k = np.asarray(key, np.int64).reshape(-1, 4)
    assert (np.abs(k[:, :3]) < SPAN).all() and ((k[:, 3] >= 1) & (k[:, 3] <= 7)).all()
    return (((k[:, 0] + SPAN) * (2 * SPAN) + (k[:, 1] + SPAN)) * (2 * SPAN) + (k[:, 2] + SPAN)) * 8 + k[:, 3]


class FastArchive:
    """the same archive on whole arrays: a sorted table of packed keys instead of the dict"""

    def __init__(self, coloured=False):
        self.coloured = coloured
        self.sorted, self.where = np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.xyz, self.rgba, self.key, self.tri = [np.zeros((0, 3), F)], [np.zeros((0, 4), np.uint8)], [np.zeros((0, 4), np.int32)], [np.zeros((0, 3), np.int32)]
        self.nv = 0

    def append(self, xyz, tri, key, rgba=None):
        assert (rgba is not None) == self.coloured and len(xyz) == len(key)
        p = pack(key)
        assert len(np.unique(p)) == len(p)                                      # within one mesh all keys are distinct
        at = np.minimum(np.searchsorted(self.sorted, p), max(len(self.sorted) - 1, 0))
        held = (self.sorted[at] == p) if len(self.sorted) else np.zeros(len(p), bool)
        remap = np.where(held, self.where[at] if len(self.sorted) else 0, self.nv + np.cumsum(~held) - 1)
        new = ~held
        self.xyz.append(np.asarray(xyz, F)[new])
        self.key.append(np.asarray(key, np.int32)[new])
        if self.coloured:
            self.rgba.append(np.asarray(rgba, np.uint8)[new])
        self.tri.append(remap[np.asarray(tri, np.int64)].astype(np.int32).reshape(-1, 3))
        allp, allw = np.concatenate([self.sorted, p[new]]), np.concatenate([self.where, remap[new]])
        order = np.argsort(allp, kind="stable")
        self.sorted, self.where = allp[order], allw[order]
        added = int(new.sum())
        self.nv += added
        return added, len(p) - added, len(tri)

    def arrays(self):
        return np.concatenate(self.xyz), np.concatenate(self.tri), np.concatenate(self.rgba) if self.coloured else None, np.concatenate(self.key)


def key_triples(tri, key):
    """the triangles as rows of twelve ints, the keys of their three vertices in order, sorted: a multiset that does not depend on how vertices are numbered"""
    rows = np.asarray(key, np.int64)[np.asarray(tri, np.int64).reshape(-1, 3)].reshape(-1, 12)
    return rows[np.lexsort(rows.T[::-1])]


def seam_keys(a, b):
    """the keys two pieces share"""
    sa = {tuple(int(x) for x in k) for k in a}
    return {tuple(int(x) for x in k) for k in b} & sa


def follow(ops, centre, margin, min_weight):
    """nalo_tsdf_follow as the header defines it, on an object that offers the calls it is made of: geometry() -> dict(origin, vs, dims), shift_for, shift_boxes,
    archive_mesh(min_weight, (lo, size)), shift(s). Returns the shift"""
    g = ops.geometry()
    s = ops.shift_for(g, centre, margin)
    if any(s):
        for lo, size in ops.shift_boxes(g["dims"], s)["boxes"]:
            ops.archive_mesh(min_weight, (lo, size))
    ops.shift(s)
    return tuple(int(v) for v in s)
