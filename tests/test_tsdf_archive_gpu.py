"""nalo_tsdf_archive_* and nalo_tsdf_follow on the device (include/nalo_gpu.h, "The mesh archive") against tests/tsdf_archive_model.py, which is fed pieces that
tests/tsdf_mesh_model.py evaluates on a model volume with its current origin. Everything is equality: positions bit for bit (a NaN as a NaN), indices, colours,
keys and every count exactly; the one tolerance is the signed volume of the sphere that was cut, shifted and welded. Volumes are planted through nalo_tsdf_set."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import tsdf_archive_model as am
import tsdf_color_model as cm
import tsdf_mesh_model as mm
import tsdf_model as tm
import tsdf_shift_model as sm
from nalo_slam_amd import binding
from test_tsdf_color_gpu import random_colour
from test_tsdf_gpu import bits_eq, ctx
from test_tsdf_mesh_gpu import device_mesh, grid, random_field

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4
SMALL_GRIDS = [(1, 1, 1), (2, 2, 2), (5, 3, 2), (33, 17, 5), (32, 24, 40)]


def create(c, g, colour, archive=True):
    """a volume (with colour) on the device and in the model, and the archive, which takes its colour state from the volume as it is then"""
    c.tsdf_create(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    if colour:
        c.tsdf_color_enable()
    if archive:
        c.tsdf_archive_enable()
    return (cm.volume if colour else tm.volume)(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])


def plant(c, vol):
    c.tsdf_set((0, 0, 0), vol["tsdf"], vol["weight"])
    if vol.get("colour") is not None:
        c.tsdf_color_set((0, 0, 0), vol["colour"])


def planted(c, g, colour, seed, archive=True):
    vol = random_field(create(c, g, colour, archive), seed)
    if colour:
        random_colour(vol, seed + 100)
    plant(c, vol)
    return vol


def archive_of(c):
    """(xyz, tri, rgba or None, key) as nalo_tsdf_archive_get gives them"""
    got = c.tsdf_archive_get(keys=True)
    return (got[0], got[1], got[2], got[3]) if len(got) == 4 else (got[0], got[1], None, got[2])


def same(got, want, tag=""):
    assert got[0].shape == want[0].shape and mm.same_floats(got[0], want[0]), (tag, "xyz", got[0].shape, want[0].shape)
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), (tag, "tri")
    assert (got[2] is None) == (want[2] is None) and (got[2] is None or (got[2].dtype == np.uint8 and np.array_equal(got[2], want[2]))), (tag, "rgba")
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]), (tag, "key")
    return True


def append_both(c, ar, vol, box, colour, mw=1.0, tag=""):
    """nalo_tsdf_archive_mesh of the box and the model's append of the model's piece: the three counts and the totals agree"""
    st = c.tsdf_archive_mesh(mw, box)
    p = am.piece(vol, mw, *(box or (None, None)), colour=colour)
    n = ar.append(*p)
    assert c.tsdf_mesh_counts == (len(p[0]), len(p[1])), (tag, c.tsdf_mesh_counts)
    assert (st["added_vertices"], st["welded_vertices"], st["added_triangles"]) == n, (tag, st, n)
    return st, p


def cut(dims, a, at):
    """two boxes that share the layer `at` of axis a, as nalo_tsdf_shift_boxes cuts a leaving box from the rest: [0, at] and [at, n)"""
    lo_b, size_a, size_b = [0, 0, 0], list(dims), list(dims)
    size_a[a], lo_b[a], size_b[a] = at + 1, at, dims[a] - at
    return ((0, 0, 0), tuple(size_a)), (tuple(lo_b), tuple(size_b))


# ------------------------------------------------------------------------------------------------ 1. one piece
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("dims", SMALL_GRIDS)
def test_one_piece_into_an_empty_archive_is_the_mesh_of_the_box(dims, colour):
    c, t = ctx(), ctx()
    g = grid(dims)
    vol = planted(c, g, colour, 3 + sum(dims))
    planted(t, g, colour, 3 + sum(dims), archive=False)
    boxes = [None] + ([((1, 0, 0), (dims[0] - 1, dims[1], max(dims[2] - 1, 1)))] if dims[0] > 1 else [])
    for box in boxes:
        c.tsdf_archive_reset()
        st, p = append_both(c, am.FastArchive(colour), vol, box, colour)
        got = archive_of(c)
        assert st["n_vertices"] == len(got[0]) == st["added_vertices"] and st["n_triangles"] == len(got[1]) and st["welded_vertices"] == 0 and st["coloured"] == colour
        mesh = c.tsdf_mesh(1.0, *(box or (None, None)), colour=colour)          # nalo_tsdf_mesh_color of the same box, array for array
        assert got[0].tobytes() == mesh[0].tobytes() and np.array_equal(got[1], mesh[1]) and (not colour or np.array_equal(got[2], mesh[2]))
        same(got, (p[0], p[1], p[3], p[2]), (dims, box))                                               # and the model's, keys included
        # the device mesh behind the call is what a mesh call alone leaves
        c.tsdf_archive_mesh(1.0, box)
        t.tsdf_mesh(1.0, *(box or (None, None)), download=False, colour=colour)
        assert [m[1:] for m in device_mesh(c, colour)] == [m[1:] for m in device_mesh(t, colour)]
    c.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 2. two pieces and their seam
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("dims", [(5, 3, 2), (33, 17, 5)])
def test_two_boxes_that_share_a_seam_layer_in_both_orders(dims, colour):
    c = ctx()
    vol = planted(c, grid(dims), colour, 17)
    whole = am.piece(vol, 1.0, colour=colour)
    want = am.key_triples(whole[1], whole[2])
    if dims == (5, 3, 2):
        cuts = [(a, at) for a in range(3) for at in range(dims[a])]             # every cut position
    else:
        cuts = sorted({(0, at) for m in range(4, 33, 4) for at in (m - 1, m, m + 1) if at < 33})      # either side of every multiple of four in x
    n_welded = 0
    for a, at in cuts:
        A, B = cut(dims, a, at)
        for first, second in ((A, B), (B, A)):
            c.tsdf_archive_reset()
            ar = am.FastArchive(colour)
            _, p1 = append_both(c, ar, vol, first, colour, tag=(a, at))
            st, p2 = append_both(c, ar, vol, second, colour, tag=(a, at))
            seam = am.seam_keys(p1[2], p2[2])
            assert all(k[a] == at and not (k[3] >> a) & 1 for k in seam)        # the vertices on the shared layer's edges
            assert st["welded_vertices"] == len(seam) and st["n_vertices"] == len(whole[0]) and st["n_triangles"] == len(whole[1]), (a, at, st)
            got = archive_of(c)
            same(got, ar.arrays(), (a, at))
            assert np.array_equal(am.key_triples(got[1], got[3]), want), (a, at)
            n_welded += len(seam)
    assert n_welded > (20 if dims == (5, 3, 2) else 2000)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. the first occurrence wins; a sphere stays closed
def sphere_volume(g, colour, radius=9.3):
    """the signed distance to a sphere around the middle of the grid, every voxel valid, with seeded colours"""
    vol = (cm.volume if colour else tm.volume)(g["origin"], g["vs"], g["dims"], g["trunc"], g["mw"])
    cs = tm.centres(vol)
    mid = [np.float64(cs[a][len(cs[a]) // 2]) for a in range(3)]
    r = np.sqrt((cs[0][None, None, :].astype(np.float64) - mid[0]) ** 2 + (cs[1][None, :, None].astype(np.float64) - mid[1]) ** 2 +
                (cs[2][:, None, None].astype(np.float64) - mid[2]) ** 2)
    vol["tsdf"][:] = (r - radius * np.float64(vol["vs"])).astype(F)
    vol["weight"][:] = 1.0
    if colour:
        vol["colour"][:] = np.random.RandomState(5).uniform(0, 255, vol["colour"].shape).astype(F)
    return vol


def test_first_occurrence_wins_and_a_cut_sphere_stays_watertight():
    g = grid((32, 24, 40))
    c = ctx()
    create(c, g, True)
    vol = sphere_volume(g, True)
    plant(c, vol)
    whole = am.piece(vol, 1.0, colour=True)
    assert len(whole[1]) > 2000 and mm.is_closed_and_oriented(whole[1])
    A, B = cut(g["dims"], 0, 16)
    ar = am.FastArchive(True)
    _, pa = append_both(c, ar, vol, A, True)
    # the seam voxels keep integrating: other magnitudes and other colours on the layer, no sign changed
    vol["tsdf"][:, :, 16] *= F(0.5)
    vol["colour"][:, :, :, 16] = 255.0 - vol["colour"][:, :, :, 16]
    plant(c, vol)
    st, pb = append_both(c, ar, vol, B, True)
    got = archive_of(c)
    same(got, ar.arrays())
    seam = am.seam_keys(pa[2], pb[2])
    assert st["welded_vertices"] == len(seam) > 100
    # a seam vertex keeps the first position and colour bit for bit, B's copy differs, and B's triangles name the archived one
    a_at = {tuple(k): v for v, k in enumerate(pa[2].tolist())}
    b_at = {tuple(k): v for v, k in enumerate(pb[2].tolist())}
    moved = recoloured = 0
    named = set(got[1][len(pa[1]):].reshape(-1).tolist())
    for k in seam:
        va, vb = a_at[k], b_at[k]
        assert got[0][va].tobytes() == pa[0][va].tobytes() and got[2][va].tobytes() == pa[3][va].tobytes() and got[3][va].tolist() == list(k)
        moved += pa[0][va].tobytes() != pb[0][vb].tobytes()
        recoloured += pa[3][va].tobytes() != pb[3][vb].tobytes()
    assert moved == 0 and recoloured > len(seam) // 2                           # both ends of a seam edge were scaled alike: s is unchanged, the colour is not
    assert len(named & set(a_at[k] for k in seam)) > len(seam) // 2
    assert mm.is_closed_and_oriented(got[1])                                    # every undirected edge in exactly two triangles, once in each direction
    # the same two pieces concatenated on the host, as a caller would without the weld: the test can see a crack
    x1, t1 = c.tsdf_mesh(1.0, *A)
    x2, t2 = c.tsdf_mesh(1.0, *B)
    assert not mm.is_closed_and_oriented(np.concatenate([t1, t2 + len(x1)]))
    c.close()


def test_a_sphere_cut_by_a_shift_keeps_its_signed_volume():
    """box X of the shift (16, 0, 0) is archived, the volume shifts - its origin is recomputed, so the seam vertices' later copies differ in their last bits - and
    the rest is archived from the shifted volume. The surface is closed, and its signed volume is the unshifted whole-grid mesh's up to what the positions differ
    by. The voxel size 0.1 is no power of two, so that the two origins do give other last bits. The bound on the spread: a coordinate is
    (origin + ((float)i + 0.5f) * vs) + prod with the same prod at both origins: three roundings at the first origin, five at the second (the product and the
    sum of the shifted origin come on top), each at most half an ulp of the largest coordinate: spread <= 4 ulp. Moving every vertex by at most d changes
    the volume by at most d times the surface area (the gradient of the volume at a vertex is a third of the summed area normals of its triangles); the
    tolerance is twice that, for the second-order terms. Measured: spread 2.4e-7 (half an ulp of 4.8e-7), |dV| 1.2e-7 against 2 * area * spread = 5.2e-6,
    V = 3.35."""
    g = grid((32, 24, 40), vs=0.1)
    c = ctx()
    create(c, g, False)
    vol = sphere_volume(g, False)
    plant(c, vol)
    whole = am.piece(vol, 1.0)
    s = (16, 0, 0)
    ar = am.FastArchive()
    boxes = binding.tsdf_shift_boxes(g["dims"], s)["boxes"]
    assert boxes == [((0, 0, 0), (17, 24, 40))]
    append_both(c, ar, vol, boxes[0], False)
    c.tsdf_shift(s)
    sm.shift_volume(vol, s)
    assert not bits_eq(vol["origin"], vol["origin0"])
    st, _ = append_both(c, ar, vol, None, False)
    got = archive_of(c)
    same(got, ar.arrays())
    assert st["welded_vertices"] > 100 and st["n_vertices"] == len(whole[0]) and mm.is_closed_and_oriented(got[1])
    assert np.array_equal(am.key_triples(got[1], got[3]), am.key_triples(whole[1], whole[2]))
    at = {tuple(k): v for v, k in enumerate(whole[2].tolist())}
    order = np.array([at[tuple(k)] for k in got[3].tolist()])
    spread = float(np.abs(got[0].astype(np.float64) - whole[0][order].astype(np.float64)).max())
    ulp = float(np.spacing(F(np.abs(whole[0]).max())))
    p = whole[0].astype(np.float64)
    area = float(0.5 * np.linalg.norm(np.cross(p[whole[1][:, 1]] - p[whole[1][:, 0]], p[whole[1][:, 2]] - p[whole[1][:, 0]]), axis=1).sum())
    v0, v1 = mm.signed_volume(*whole[:2]), mm.signed_volume(got[0], got[1])
    print("sphere: spread %.3g (ulp %.3g), area %.4g, V %.6g, |dV| %.3g, tolerance %.3g" % (spread, ulp, area, v0, abs(v1 - v0), 2 * area * spread))
    assert 0 < spread <= 4.0 * ulp
    assert v0 > 0 and abs(v1 - v0) <= 2.0 * area * spread
    c.close()


# ------------------------------------------------------------------------------------------------ 4. a walk through nalo_tsdf_follow
class LoopOps:
    """the loop of INTEGRATION.md call by call on a context, and on the model next to it"""

    def __init__(self, c, vol, ar, colour):
        self.c, self.vol, self.ar, self.colour = c, vol, ar, colour

    def geometry(self):
        return self.c.tsdf_geometry()

    def shift_for(self, g, centre, margin):
        return binding.tsdf_shift_for(g["desc"], centre, margin)

    def shift_boxes(self, dims, s):
        return binding.tsdf_shift_boxes(dims, s)

    def archive_mesh(self, mw, box):
        append_both(self.c, self.ar, self.vol, box, self.colour, mw)

    def shift(self, s):
        self.c.tsdf_shift(s)
        sm.shift_volume(self.vol, s)


@pytest.mark.parametrize("colour", [False, True])
def test_a_walk_of_twelve_shifts_through_follow(colour):
    g = grid((32, 24, 40))
    c, t = ctx(), ctx()
    vol = planted(c, g, colour, 41)
    planted(t, g, colour, 41)
    whole = am.piece(vol, 1.0, colour=colour)
    ar = am.FastArchive(colour)
    ops = LoopOps(t, vol, ar, colour)
    rng = np.random.RandomState(8)
    n_boxes = n_welded = 0
    for step in range(12):
        s = [int(v) for v in rng.randint(-3, 4, 3)]
        if step == 5:
            s = [0, 0, 0]                                                       # a step inside the dead band: nothing is archived, nothing shifts
        geo = c.tsdf_geometry()
        centre = [float(np.float64(geo["origin"][a]) + (g["dims"][a] // 2 + s[a] + 0.5) * np.float64(geo["voxel_size"])) for a in range(3)]
        out = c.tsdf_follow(centre, (0, 0, 0), 1.0)
        assert out["shift"].tolist() == s, (step, out, s)
        assert am.follow(ops, centre, (0, 0, 0), 1.0) == tuple(s)
        assert out["n_boxes"] == len(sm.shift_boxes(g["dims"], s)["boxes"]) * bool(any(s)) and out["n_vertices"] == ar.nv
        n_boxes += out["n_boxes"]
        n_welded += out["welded_vertices"]
        assert bits_eq(c.tsdf_geometry()["origin"], np.asarray(vol["origin"], F)) and c.tsdf_geometry()["base"].tolist() == [int(v) for v in vol["base"]]
    c.tsdf_archive_mesh(1.0)                                                    # what is still in the volume
    append_both(t, ar, vol, None, colour)
    got = archive_of(c)
    same(got, archive_of(t), "the loop call by call")
    same(got, ar.arrays(), "the model")
    assert n_boxes >= 20 and n_welded > 1000
    # every cell of the planted grid was archived exactly once, when it left or at the end (the refilled slabs carry weight 0: no cell of theirs is live)
    assert np.array_equal(am.key_triples(got[1], got[3]), am.key_triples(whole[1], whole[2]))
    assert all(bits_eq(x, y) for x, y in zip(c.tsdf_get(), t.tsdf_get()))
    c.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 5. the same box twice, and the smallest pieces
def test_the_same_box_twice_an_empty_piece_the_smallest_piece_and_one_voxel():
    """a corner other than 0 and 7 lies in two tetrahedra of its cell, and 0 and 7 in all six: a piece of ONE triangle does not exist; the smallest has two"""
    c = ctx()
    vol = planted(c, grid((5, 3, 2)), True, 9)
    ar = am.FastArchive(True)
    box = ((1, 0, 0), (4, 3, 2))
    st1, p = append_both(c, ar, vol, box, True)
    st2, _ = append_both(c, ar, vol, box, True)
    assert st1["added_vertices"] == len(p[0]) > 0 and len(p[1]) > 0
    assert st2["added_vertices"] == 0 and st2["welded_vertices"] == len(p[0]) and st2["n_vertices"] == len(p[0]) and st2["n_triangles"] == 2 * len(p[1])
    got = archive_of(c)
    same(got, ar.arrays())
    assert np.array_equal(got[1][:len(p[1])], got[1][len(p[1]):])
    # an empty piece: a box of one voxel has no edge
    st3, p3 = append_both(c, ar, vol, ((2, 1, 0), (1, 1, 1)), True)
    assert len(p3[0]) == 0 and (st3["added_vertices"], st3["welded_vertices"], st3["added_triangles"]) == (0, 0, 0) and st3["n_triangles"] == 2 * len(p[1])
    same(archive_of(c), ar.arrays())
    c.close()
    # one cell, corner 1 alone inside: two triangles, three vertices each on their own edges
    c = ctx()
    vol = create(c, grid((2, 2, 2)), False)
    vol["weight"][:] = 1.0
    vol["tsdf"][:] = 0.5
    vol["tsdf"][0, 0, 1] = -0.25
    plant(c, vol)
    ar = am.Archive()
    st, p = append_both(c, ar, vol, None, False)
    assert len(p[1]) == 2 and st["n_triangles"] == 2 and st["n_vertices"] == len(p[0]) == 4
    same(archive_of(c), ar.arrays())
    c.close()
    # a grid of one voxel
    c = ctx()
    vol = create(c, grid((1, 1, 1)), False)
    vol["weight"][:], vol["tsdf"][:] = 1.0, -0.5
    plant(c, vol)
    st = c.tsdf_archive_mesh(1.0)
    assert (st["n_vertices"], st["n_triangles"], st["have_lattice"]) == (0, 0, True) and [len(a) for a in c.tsdf_archive_get(keys=True)] == [0, 0, 0]
    c.close()


# ------------------------------------------------------------------------------------------------ 6. growth, reset, the caps of nalo_tsdf_archive_get
def get_once(c, capv, capt, capc, capk, fill=7):
    """ONE nalo_tsdf_archive_get with arrays of the given caps (None: no array), filled with a sentinel: (rc, xyz, tri, rgba, key, n_vertices, n_triangles)"""
    a = binding.TsdfArchiveGetArgs()
    xyz = None if capv is None else np.full((max(capv, 1), 3), fill, F)
    tri = None if capt is None else np.full((max(capt, 1), 3), fill, np.int32)
    rgba = None if capc is None else np.full((max(capc, 1), 4), fill, np.uint8)
    key = None if capk is None else np.full((max(capk, 1), 4), fill, np.int32)
    a.cap_vertices, a.cap_triangles, a.cap_rgba, a.cap_key = capv or 0, capt or 0, capc or 0, capk or 0
    a.xyz, a.tri, a.rgba, a.key = binding._f(xyz), binding._i(tri), binding._u8(rgba), binding._i(key)
    rc = c.L.nalo_tsdf_archive_get(c.h_, C.byref(a))
    return rc, xyz, tri, rgba, key, int(a.n_vertices), int(a.n_triangles)


def test_growth_reset_and_the_caps_of_get():
    g = grid((32, 24, 40))
    c = ctx()
    vol = planted(c, g, True, 21)
    slabs = [((0, 0, z), (32, 24, min(5, 40 - z))) for z in range(0, 39, 4)]     # ten slabs of five layers, neighbours share one
    runs = []
    for run in range(2):
        ar = am.FastArchive(True)
        st0 = c.tsdf_archive_stats()
        caps, grown = [(st0["cap_vertices"], st0["cap_triangles"], st0["table_slots"])], [0, 0, 0]
        if run == 0:
            assert caps[0] == (4096, 8192, 8192) and (st0["n_vertices"], st0["n_triangles"], st0["have_lattice"]) == (0, 0, False)
        ptr = c.tsdf_archive_view()["xyz"].ptr
        moved = 0
        for box in slabs:
            st, _ = append_both(c, ar, vol, box, True)
            now = (st["cap_vertices"], st["cap_triangles"], st["table_slots"])
            for k in range(3):
                grown[k] += now[k] > caps[-1][k]
            assert now[0] >= st["n_vertices"] and now[1] >= st["n_triangles"] and now[2] >= 2 * st["n_vertices"] and now[2] & (now[2] - 1) == 0      # load <= 1/2
            moved += c.tsdf_archive_view()["xyz"].ptr != ptr
            ptr = c.tsdf_archive_view()["xyz"].ptr
            caps.append(now)
        if run == 0:
            assert min(grown) >= 3 and moved >= 3, (grown, caps)                # every buffer and the table passed its first capacity at least three times
        else:
            assert grown == [0, 0, 0] and moved == 0                            # nalo_tsdf_archive_reset kept the buffers
        got = archive_of(c)
        same(got, ar.arrays(), run)
        runs.append([a.tobytes() for a in got])
        if run == 0:
            c.tsdf_archive_reset()
            st = c.tsdf_archive_stats()
            assert (st["n_vertices"], st["n_triangles"], st["have_lattice"], st["coloured"]) == (0, 0, False, True) and st["cap_vertices"] == caps[-1][0]
    assert runs[0] == runs[1]
    nv, nt = len(got[0]), len(got[1])
    assert nv > 4 * 4096 and nt > 4 * 8192
    # caps one below each count, one array at a time: NALO_ERR_ARG, the counts set, no array touched
    for short in range(4):
        caps = [nv, nt, nv, nv]
        caps[short] -= 1
        rc, xyz, tri, rgba, key, n1, n2 = get_once(c, *caps)
        assert rc == ERR_ARG and (n1, n2) == (nv, nt), short
        assert (xyz == 7).all() and (tri == 7).all() and (rgba == 7).all() and (key == 7).all(), short
    # cap = 0 with arrays: refused for a non-empty archive, the counts come back; NULL arrays with cap 0: the counts only
    rc, xyz, tri, rgba, key, n1, n2 = get_once(c, 0, 0, 0, 0)
    assert rc == ERR_ARG and (n1, n2) == (nv, nt) and (xyz == 7).all() and (tri == 7).all() and (rgba == 7).all() and (key == 7).all()
    rc, _, _, _, _, n1, n2 = get_once(c, None, None, None, None)
    assert rc == 0 and (n1, n2) == (nv, nt)
    # a single array asked for, with room to spare: the rows behind the count keep the sentinel
    rc, xyz, _, _, _, _, _ = get_once(c, nv + 3, None, None, None)
    assert rc == 0 and mm.same_floats(xyz[:nv], got[0]) and (xyz[nv:] == 7).all()
    rc, _, tri, _, _, _, _ = get_once(c, None, nt, None, None)
    assert rc == 0 and np.array_equal(tri, got[1])
    rc, _, _, rgba, _, _, _ = get_once(c, None, None, nv, None)
    assert rc == 0 and np.array_equal(rgba, got[2])
    rc, _, _, _, key, _, _ = get_once(c, None, None, None, nv + 1)
    assert rc == 0 and np.array_equal(key[:nv], got[3]) and (key[nv:] == 7).all()
    for bad in ((-1, None, None, None), (None, -1, None, None), (None, None, -1, None), (None, None, None, -1)):
        a = binding.TsdfArchiveGetArgs()
        a.cap_vertices, a.cap_triangles, a.cap_rgba, a.cap_key = [v or 0 for v in bad]
        assert c.L.nalo_tsdf_archive_get(c.h_, C.byref(a)) == ERR_ARG
    a = binding.TsdfArchiveGetArgs()
    a.cap_key = nv                                                              # a cap > 0 with a NULL array
    assert c.L.nalo_tsdf_archive_get(c.h_, C.byref(a)) == ERR_ARG and c.L.nalo_tsdf_archive_get(c.h_, None) == ERR_ARG
    c.close()


# ------------------------------------------------------------------------------------------------ 7. the view
def test_the_view_against_get_and_on_a_second_stream_without_a_host_wait():
    g = grid((32, 24, 40))
    c = ctx()
    vol = planted(c, g, True, 33)
    A, B = cut(g["dims"], 2, 20)
    for box in (A, B, B):                                                       # the steady state: every buffer, the mesh's too, has its size
        c.tsdf_archive_mesh(1.0, box)
    c.tsdf_archive_reset()
    c.tsdf_archive_mesh(1.0, A)
    before = c.tsdf_archive_view()
    a = torch.randn(4096, 4096, device="cuda")
    out = torch.empty_like(a)
    S, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        with torch.cuda.stream(S):
            torch.mm(a, a, out=out)
            S.synchronize()
            t0 = time.perf_counter()
            torch.mm(a, a, out=out)
            S.synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
            for _ in range(min(int(math.ceil(0.25 / one)) + 1, 20000)):
                torch.mm(a, a, out=out)
            behind = torch.cuda.Event()
            behind.record(S)
        st = c.tsdf_archive_mesh(1.0, B)                                        # waits for its own stream only
        v = c.tsdf_archive_view()
        with torch.cuda.stream(S2):
            S2.wait_stream(torch.cuda.ExternalStream(v["xyz"].stream))          # on the device: the producing stream
            copies = {k: torch.as_tensor(v[k], device="cuda").clone() for k in ("xyz", "tri", "rgba", "key")}
        returned_early = not behind.query()
        assert returned_early, "nalo_tsdf_archive_mesh and the view's consumer waited for another stream's work"
        S2.synchronize()
        assert st["welded_vertices"] > 100 and v["xyz"].ptr == before["xyz"].ptr and v["tri"].ptr == before["tri"].ptr      # nothing grew: the earlier view is still good
        assert v["xyz"].shape == (st["n_vertices"], 3) and v["tri"].shape == (st["n_triangles"], 3) and v["rgba"].shape == (st["n_vertices"], 4)
        assert v["key"].shape == (st["n_vertices"], 4) and v["xyz"].stream == c.L.nalo_stream(c.h_)
        t = torch.as_tensor(v["xyz"], device="cuda")
        assert t.data_ptr() == v["xyz"].ptr and t.dtype == torch.float32 and copies["tri"].dtype == torch.int32 and copies["rgba"].dtype == torch.uint8
        got = archive_of(c)
        same((copies["xyz"].cpu().numpy(), copies["tri"].cpu().numpy(), copies["rgba"].cpu().numpy(), copies["key"].cpu().numpy()), got)
        ar = am.FastArchive(True)
        for box in (A, B):
            ar.append(*am.piece(vol, 1.0, *box, colour=True))
        same(got, ar.arrays())
    finally:
        S.synchronize()
        c.close()
        torch.cuda.synchronize()
    # an uncoloured archive has no rgba view, and write_ply_mesh takes the arrays as they come
    c = ctx()
    planted(c, grid((5, 3, 2)), False, 2)
    c.tsdf_archive_mesh(1.0)
    assert c.tsdf_archive_view()["rgba"] is None and len(c.tsdf_archive_get()) == 2
    c.close()


def test_write_ply_mesh_takes_the_archives_arrays(tmp_path):
    for colour in (False, True):
        c = ctx()
        planted(c, grid((5, 3, 2)), colour, 2)
        c.tsdf_archive_mesh(1.0, ((0, 0, 0), (3, 3, 2)))
        c.tsdf_archive_mesh(1.0, ((2, 0, 0), (3, 3, 2)))
        arrays = c.tsdf_archive_get()
        path = tmp_path / ("a%d.ply" % colour)
        binding.write_ply_mesh(str(path), *arrays)
        head = path.read_bytes().split(b"end_header\n")[0].decode()
        assert "element vertex %d\n" % len(arrays[0]) in head and "element face %d\n" % len(arrays[1]) in head and ("red" in head) == colour
        c.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def mesh_args(mw=1.0, box=None, capv=0, xyz=None):
    a = binding.TsdfMeshArgs()
    if box is not None:
        a.use_box = 1
        a.lo[:], a.size[:] = box[0], box[1]
    a.min_weight = mw
    a.cap_vertices, a.xyz = capv, binding._f(xyz)
    return a


def archive_rc(c, a, st=None):
    return c.L.nalo_tsdf_archive_mesh(c.h_, None if a is None else C.byref(a), None if st is None else C.byref(st))


def snapshot(c, colour):
    """what a refused call must leave: the archive's arrays, its stats and view pointers, the volume's bits, the colour and the geometry"""
    v = c.tsdf_archive_view()
    geo = c.tsdf_geometry()
    out = [a.tobytes() for a in c.tsdf_archive_get(keys=True)] + [repr(sorted((k, str(x)) for k, x in c.tsdf_archive_stats().items())), (v["xyz"].ptr, v["tri"].ptr, v["key"].ptr)]
    out += [a.tobytes() for a in c.tsdf_get()] + [geo["origin"].tobytes(), geo["base"].tobytes()]
    if colour:
        out.append(c.tsdf_color_get().tobytes())
    return out


def test_refusals_leave_archive_volume_and_device_mesh_as_stated():
    c, t = ctx(), ctx()
    st, gargs, dv = binding.TsdfArchiveStats(), binding.TsdfArchiveGetArgs(), binding.TsdfArchiveDev()
    # before nalo_tsdf_archive_enable
    assert archive_rc(c, mesh_args()) == ERR_STATE and c.L.nalo_tsdf_archive_stats(c.h_, C.byref(st)) == ERR_STATE
    assert c.L.nalo_tsdf_archive_get(c.h_, C.byref(gargs)) == ERR_STATE and c.L.nalo_tsdf_archive_view(c.h_, C.byref(dv)) == ERR_STATE
    assert c.L.nalo_tsdf_archive_reset(c.h_) == ERR_STATE and c.L.nalo_tsdf_archive_disable(c.h_) == 0
    ce, mg, sh, fs = np.zeros(3), np.zeros(3, np.int32), np.zeros(3, np.int32), binding.TsdfFollowStats()
    follow = lambda x: x.L.nalo_tsdf_follow(x.h_, binding._d(ce), binding._i(mg), 1.0, binding._i(sh), C.byref(fs))
    assert follow(c) == ERR_STATE
    g = grid((33, 17, 5))
    vol = planted(c, g, True, 13, archive=False)
    assert archive_rc(c, mesh_args()) == ERR_STATE and follow(c) == ERR_STATE   # a volume, no archive
    # an archive without a volume: uncoloured, and every append is refused
    t.tsdf_archive_enable()
    t.tsdf_archive_enable()                                                     # already enabled: nothing changes
    assert archive_rc(t, mesh_args()) == ERR_STATE and follow(t) == ERR_STATE and t.tsdf_archive_stats()["coloured"] is False
    assert (t.tsdf_archive_stats()["n_vertices"], len(t.tsdf_archive_get()[0])) == (0, 0)
    t.tsdf_archive_disable()
    planted(t, g, True, 13, archive=False)                                      # the twin that only meshes
    # a coloured archive with two pieces in it
    c.tsdf_archive_enable()
    A, B = cut(g["dims"], 0, 12)
    c.tsdf_archive_mesh(1.0, A)
    c.tsdf_mesh(1.0, (3, 2, 1), (6, 5, 4), download=False, colour=True)         # the device mesh a refused call has to leave
    before, mesh_before = snapshot(c, True), device_mesh(c, True)
    nv_b = am.piece(vol, 1.0, *B)[0].shape[0]
    # every refusal of nalo_tsdf_mesh, unchanged: nothing is queued, the counts are zero
    bad = [None, mesh_args(float("nan")), mesh_args(1.0, ((0, 0, 0), (34, 17, 5))), mesh_args(1.0, ((0, 0, 0), (0, 17, 5))), mesh_args(1.0, ((-1, 0, 0), (2, 2, 2))),
           mesh_args(1.0, None, -1), mesh_args(1.0, None, 5, None)]
    for a in bad:
        assert archive_rc(c, a, st) == ERR_ARG and (a is None or (a.n_vertices, a.n_triangles) == (0, 0))
        assert (st.added_vertices, st.welded_vertices, st.added_triangles) == (0, 0, 0)
        assert snapshot(c, True) == before and device_mesh(c, True) == mesh_before
    # a host array with a cap below the count: the device mesh IS built, nothing is appended, the array is not touched
    xyz = np.full((nv_b - 1, 3), 7.0, F)
    a = mesh_args(1.0, B, nv_b - 1, xyz)
    assert archive_rc(c, a, st) == ERR_ARG and a.n_vertices == nv_b and (xyz == 7.0).all() and snapshot(c, True) == before
    t.tsdf_mesh(1.0, *B, download=False, colour=True)
    assert [m[1:] for m in device_mesh(c, True)] == [m[1:] for m in device_mesh(t, True)]
    # host arrays that suffice are filled as nalo_tsdf_mesh fills them, and the piece is appended
    xyz = np.full((nv_b + 2, 3), 7.0, F)
    a = mesh_args(1.0, B, nv_b + 2, xyz)
    assert archive_rc(c, a, st) == 0 and st.welded_vertices > 0 and mm.same_floats(xyz[:nv_b], am.piece(vol, 1.0, *B)[0]) and (xyz[nv_b:] == 7.0).all()
    before = snapshot(c, True)
    # an uncoloured volume into the coloured archive: refused, with the plain mesh of the box built
    c.tsdf_color_disable()
    t.tsdf_color_disable()
    a = mesh_args(1.0, A)
    assert archive_rc(c, a, st) == ERR_STATE and a.n_vertices > 0 and snapshot(c, False) == before[:len(snapshot(c, False))]
    t.tsdf_mesh(1.0, *A, download=False)
    assert [m[1:] for m in device_mesh(c)] == [m[1:] for m in device_mesh(t)]
    with pytest.raises(binding.NaloError):
        c.tsdf_mesh_color_view()
    # and the reverse: a coloured volume into an uncoloured archive
    c.tsdf_archive_disable()
    c.tsdf_archive_enable()
    assert c.tsdf_archive_stats()["coloured"] is False
    c.tsdf_archive_mesh(1.0, A)
    before = snapshot(c, False)
    c.tsdf_color_enable()
    a = mesh_args(1.0, B)
    assert archive_rc(c, a, st) == ERR_STATE and a.n_vertices == nv_b and snapshot(c, False) == before
    rgba = np.zeros((10, 4), np.uint8)
    gargs = binding.TsdfArchiveGetArgs()
    gargs.cap_rgba, gargs.rgba = 10, binding._u8(rgba)
    assert c.L.nalo_tsdf_archive_get(c.h_, C.byref(gargs)) == ERR_STATE         # no colour in this archive
    c.tsdf_color_disable()
    # the lattice: a second volume with another voxel_size or origin0 is refused, the same lattice re-created is accepted; nalo_tsdf_reset and
    # nalo_tsdf_destroy leave the archive alone
    c.tsdf_reset()
    assert snapshot(c, False)[:5] == before[:5]
    c.tsdf_destroy()
    assert [x.tobytes() for x in c.tsdf_archive_get(keys=True)] == before[:3]
    for other in (dict(g, vs=0.25), dict(g, origin=(-0.7, 0.3, 1.125))):
        create(c, other, False, archive=False)
        a = mesh_args(1.0)
        assert archive_rc(c, a, st) == ERR_STATE and [x.tobytes() for x in c.tsdf_archive_get(keys=True)] == before[:3]
    create(c, g, False, archive=False)
    plant(c, dict(vol, colour=None))
    st_ok = c.tsdf_archive_mesh(1.0, B)
    assert st_ok["welded_vertices"] > 0 and st_ok["n_vertices"] == len(am.piece(vol, 1.0)[0])
    # nalo_tsdf_follow refuses what nalo_tsdf_shift_for refuses, before anything is archived or shifted
    before = snapshot(c, False)
    ce[0] = np.nan
    assert follow(c) == ERR_ARG and snapshot(c, False) == before
    ce[0], mg[1] = 0.0, -1
    assert follow(c) == ERR_ARG and snapshot(c, False) == before
    c.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 9. a context that never enables the archive
def test_a_twin_without_the_archive_gives_the_same_bits_and_two_runs_the_same_bytes():
    g = grid((33, 17, 5))

    def run(archive):
        c = ctx()
        planted(c, g, True, 29, archive=archive)
        out = []
        for s in ((4, 0, 0), (-3, 2, 1), (0, -5, 0)):
            for lo, size in binding.tsdf_shift_boxes(g["dims"], s)["boxes"]:
                if archive:
                    c.tsdf_archive_mesh(1.0, (lo, size))
                else:
                    c.tsdf_mesh(1.0, lo, size, download=False, colour=True)
                out += [m[1:] for m in device_mesh(c, True)]
            c.tsdf_shift(s)
            out += [a.tobytes() for a in c.tsdf_get()] + [c.tsdf_color_get().tobytes(), c.tsdf_geometry()["origin"].tobytes()]
            out.append(c.tsdf_surface_points(1.0).tobytes())
        arch = [a.tobytes() for a in c.tsdf_archive_get(keys=True)] if archive else None
        c.close()
        return out, arch
    a, arch_a = run(True)
    b, _ = run(False)
    a2, arch_a2 = run(True)
    assert a == b and a == a2 and arch_a == arch_a2 and len(arch_a[0]) > 1000


# ------------------------------------------------------------------------------------------------ 10. the chain
def planted_shift(c, dims):
    """a shift whose x and z seam planes cut the fused surface: the median voxel index of the surface points on those axes (five voxels back in y)"""
    geo = c.tsdf_geometry()
    idx = np.floor((c.tsdf_surface_points(1.0).astype(np.float64) - geo["origin"].astype(np.float64)) / np.float64(geo["voxel_size"]))
    med = np.median(idx, axis=0)
    return (int(min(max(med[0], 1), dims[0] - 2)), -5, int(min(max(med[2], 1), dims[2] - 2)))


def run_chain():
    """tests/test_tsdf_shift_gpu.py's chain at 1224x368, W = 8, three keyframes into a coloured 256x64x256 volume; before each integration nalo_tsdf_follow with
    the camera position, and behind the last keyframe once more with a planted centre, planted_shift() voxels off the middle (the chain's camera moves less
    than a voxel; the planted seams cut the fused surface); then the whole grid is archived. Before every nalo_tsdf_follow the volume is read back, so that the model can be fed what was archived.
    Returns the archive's arrays, the shifts and the volumes read back."""
    import lifecycle_model as lm
    import lifecycle_scenes as lsc
    import plane_cases as pc
    import plane_model as pm
    from nalo_slam_amd import synth
    WW, KF, w, h, s = 8, 3, 1224, 368, 3e-4
    DIMS = (256, 64, 256)
    win = synth.make_window(w=w, h=h, W=WW, P=8000, seed=lsc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    nF = WW + KF
    srng = np.random.RandomState(lsc.SEED + 3)
    st6 = np.zeros((nF, 6))
    st6[1:, :3] = 0.004 * srng.randn(nF - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * srng.randn(nF - 1, 3)
    mask = pc.block_mask(w, h, 2, 1, [2.0, 0.0])
    mask[2 * h // 3:, :w // 2] = 6.0
    mask[2 * h // 3:, w // 2:] = 8.0
    bgr = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    c = binding.Context(w, h, win.K, n_slots=nF)
    fids = [200 + i for i in range(WW)]
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
    c.map_dense_enable(True, 65536)
    cur, shifts, volumes = list(fids), [], []

    def read_back():
        geo = c.tsdf_geometry()
        vol = cm.volume(geo["origin0"], geo["voxel_size"], DIMS, 1.0, 16.0)
        vol["tsdf"], vol["weight"] = c.tsdf_get()
        vol["colour"] = c.tsdf_color_get()
        vol["origin0"], vol["base"], vol["origin"] = geo["origin0"].copy(), geo["base"].astype(np.int64), geo["origin"].copy()
        return vol

    def follow(centre):
        volumes.append(read_back())
        out = c.tsdf_follow(centre, (0, 0, 0), 1.0)
        shifts.append(tuple(int(v) for v in out["shift"]))

    for kf in range(KF):
        if kf:
            c.ba_marginalize_frame(0)
            c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            cur = cur[1:] + [200 + WW - 1 + kf]
        c.ba_linearize(False)
        c.ba_linearize(True)
        hf, slot = WW - 3, WW - 3 + kf
        T = synth.se3_inv(win.world_to_cam[slot])
        c.dense_update_map(hf, pm.make_draws(60 + kf), T)
        if kf == 0:
            xyz = c.map_dense_world_points(cur[hf], T)
            ok = np.isfinite(xyz).all(1)
            reach = np.maximum(np.abs(np.percentile(xyz[ok], 2, axis=0) - T[:, 3]), np.abs(np.percentile(xyz[ok], 98, axis=0) - T[:, 3]))
            vs = float(max(2.0 * reach / np.array(DIMS)) * 1.05)
            origin = T[:, 3] - 0.5 * vs * np.array(DIMS) + vs * np.array([7.3, -4.6, 9.2])     # off centre: the first follow has something to do
            dep = 1.0 / c.map_dense_get(cur[hf])["idepth"].astype(np.float64)
            dep = dep[np.isfinite(dep) & (dep > 0)]
            rng_d = (float(np.percentile(dep, 2)) * 0.5, float(np.percentile(dep, 98)) * 2.0)
            c.tsdf_create(origin, vs, DIMS, 4 * vs, 16.0)
            c.tsdf_color_enable()
            c.tsdf_archive_enable()
        follow(T[:, 3])
        c.tsdf_integrate_frame(cur[hf], T, win.K, rng_d[0], rng_d[1])
        ff = np.zeros(WW, np.uint8)
        ff[0] = 1
        c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
    geo, last = c.tsdf_geometry(), planted_shift(c, DIMS)
    follow([float(np.float64(geo["origin"][a]) + (DIMS[a] // 2 + last[a] + 0.5) * np.float64(geo["voxel_size"])) for a in range(3)])
    assert shifts[-1] == last
    volumes.append(read_back())
    st = c.tsdf_archive_mesh(1.0)
    got = archive_of(c)
    c.close()
    return got, shifts, volumes, st


def test_three_keyframes_of_the_device_chain_followed_and_archived():
    got, shifts, volumes, st = run_chain()
    print("TSDF archive chain 1224x368 into 256x64x256: shifts", shifts, "stats", st)
    assert any(shifts[0]) and len(shifts) == 4 and shifts[3][1] == -5 and st["n_vertices"] == len(got[0]) > 1000 and st["n_triangles"] == len(got[1]) > 1000
    ar = am.FastArchive(True)
    welded = 0
    for vol, s in zip(volumes, shifts + [None]):
        boxes = [(None, None)] if s is None else sm.shift_boxes(vol["dims"], s)["boxes"] if any(s) else []
        for lo, size in boxes:
            welded += ar.append(*am.piece(vol, 1.0, lo, size, colour=True))[1]
    same(got, ar.arrays(), "the vectorised model")
    print("TSDF archive chain: welded", welded, "of", len(got[0]), "vertices")
    assert welded > 0
    again = run_chain()[0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
