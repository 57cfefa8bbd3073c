"""tests/tsdf_archive_model.py against a volume worked by hand, against the mesh definition and against the whole-grid mesh (include/nalo_gpu.h, "The mesh
archive"), and the entry points of the library. No device. nalo_tsdf_follow itself is a composition of calls that need a device (geometry, mesh, shift): its
call sequence cannot be observed here, only the model's follow() that the device tests run call by call next to it (tests/test_tsdf_archive_gpu.py, the walk)."""
import ctypes as C

import numpy as np

import tsdf_archive_model as am
import tsdf_color_model as cm
import tsdf_mesh_model as mm
import tsdf_model as tm
import tsdf_shift_model as sm
from nalo_slam_amd import binding

F = np.float32
ERR_ARG = -1


def test_exports_and_entry_points():
    names = ("nalo_tsdf_archive_enable", "nalo_tsdf_archive_disable", "nalo_tsdf_archive_reset", "nalo_tsdf_archive_mesh", "nalo_tsdf_archive_stats",
             "nalo_tsdf_archive_get", "nalo_tsdf_archive_view", "nalo_tsdf_follow")
    L = binding.host_lib()
    for s in names:
        assert s in binding.EXPORTS and hasattr(L, s)
    for m in ("tsdf_archive_enable", "tsdf_archive_disable", "tsdf_archive_reset", "tsdf_archive_stats", "tsdf_archive_mesh", "tsdf_archive_get", "tsdf_archive_view",
              "tsdf_follow"):
        assert callable(getattr(binding.Context, m))
    # without a context every call refuses before it touches a device
    for s in names[:3]:
        f = getattr(L, s)
        f.argtypes = [C.c_void_p]
        assert f(None) == ERR_ARG
    for s in names[3:7]:
        f = getattr(L, s)
        f.argtypes = [C.c_void_p, C.c_void_p] + ([C.c_void_p] if s == "nalo_tsdf_archive_mesh" else [])
        assert f(*([None] * len(f.argtypes))) == ERR_ARG
    L.nalo_tsdf_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    assert L.nalo_tsdf_follow(None, None, None, 1.0, None, None) == ERR_ARG
    # the structs the binding passes have the header's sizes
    assert C.sizeof(binding.TsdfArchiveStats) == 8 * 8 + 2 * 4 + 4 * 4 and C.sizeof(binding.TsdfArchiveGetArgs) == 10 * 8
    assert C.sizeof(binding.TsdfArchiveDev) == 7 * 8 and C.sizeof(binding.TsdfFollowStats) == 8 + 5 * 8


def hand_volume():
    """3x2x2 voxels, every one valid, inside iff j == 0: every crossing lies on an edge with d_y = 1 (m = 2, 3, 6, 7) owned by a voxel with j = 0"""
    vol = tm.volume((-1.0, 0.5, 2.0), 0.25, (3, 2, 2), 1.0, 4.0)
    vol["weight"][:] = 1.0
    vol["tsdf"][:, 0, :], vol["tsdf"][:, 1, :] = -0.5, 0.5
    return vol


def test_the_model_by_hand_on_a_3x2x2_volume_cut_in_two():
    vol = hand_volume()
    whole = am.piece(vol, 1.0)
    # by hand: voxel (i, 0, k) owns m = 2 always, 3 iff i < 2, 6 iff k == 0, 7 iff i < 2 and k == 0
    assert whole[2].tolist() == [[0, 0, 0, 2], [0, 0, 0, 3], [0, 0, 0, 6], [0, 0, 0, 7], [1, 0, 0, 2], [1, 0, 0, 3], [1, 0, 0, 6], [1, 0, 0, 7], [2, 0, 0, 2], [2, 0, 0, 6],
                                 [0, 0, 1, 2], [0, 0, 1, 3], [1, 0, 1, 2], [1, 0, 1, 3], [2, 0, 1, 2]]
    A = am.piece(vol, 1.0, (0, 0, 0), (2, 2, 2))                                # x in [0, 2): the seam layer i = 1 is its high face
    assert A[2].tolist() == [[0, 0, 0, 2], [0, 0, 0, 3], [0, 0, 0, 6], [0, 0, 0, 7], [1, 0, 0, 2], [1, 0, 0, 6], [0, 0, 1, 2], [0, 0, 1, 3], [1, 0, 1, 2]]
    # the seam voxels keep integrating: other magnitudes on layer i = 1, no sign changed; the second piece sees them
    vol["tsdf"][:, :, 1] *= F(0.5)
    B = am.piece(vol, 1.0, (1, 0, 0), (2, 2, 2))                                # x in [1, 3): the seam layer is its low face
    assert B[2].tolist() == [[1, 0, 0, 2], [1, 0, 0, 3], [1, 0, 0, 6], [1, 0, 0, 7], [2, 0, 0, 2], [2, 0, 0, 6], [1, 0, 1, 2], [1, 0, 1, 3], [2, 0, 1, 2]]
    assert am.seam_keys(A[2], B[2]) == {(1, 0, 0, 2), (1, 0, 0, 6), (1, 0, 1, 2)}  # the edges that lie inside the layer: d_x = 0
    for cls in (am.Archive, am.FastArchive):
        ar = cls()
        assert ar.append(*A[:3]) == (9, 0, len(A[1])) and ar.append(*B[:3]) == (6, 3, len(B[1]))
        xyz, tri, rgba, key = ar.arrays()
        assert rgba is None and len(xyz) == 15 == len(whole[0]) and len(tri) == len(A[1]) + len(B[1]) == len(whole[1])
        assert key.tolist() == A[2].tolist() + [[1, 0, 0, 3], [1, 0, 0, 7], [2, 0, 0, 2], [2, 0, 0, 6], [1, 0, 1, 3], [2, 0, 1, 2]]
        # the first occurrence wins: the seam vertices 4, 5 and 8 keep A's positions, and B's triangles name them
        assert xyz[:9].tobytes() == A[0].tobytes()
        held = {0: 4, 2: 5, 6: 8}
        assert tri[:len(A[1])].tolist() == A[1].tolist()
        remap = np.array([held.get(v, -1) for v in range(9)])
        remap[remap < 0] = np.arange(9, 15)
        assert tri[len(A[1]):].tolist() == remap[B[1]].tolist()
        assert np.array_equal(am.key_triples(tri, key), am.key_triples(whole[1], whole[2]))
        # the same box twice: no vertex, every triangle again
        assert ar.append(*B[:3]) == (0, 9, len(B[1])) and len(ar.arrays()[0]) == 15 and len(ar.arrays()[1]) == len(whole[1]) + len(B[1])
    # a changed magnitude with an unchanged sign moves a vertex whose two ends changed differently: edge 3 of voxel (0, 0, 0) ends in the layer
    assert not mm.same_floats(am.piece(vol, 1.0)[0], whole[0])


def seeded(dims, seed, colour=False, valid=0.85, shift=None):
    rng = np.random.RandomState(seed)
    g = dict(origin=(-1.0, 0.5, 2.0), vs=0.125, trunc=0.25, mw=4.0)
    vol = (cm.volume if colour else tm.volume)(g["origin"], g["vs"], dims, g["trunc"], g["mw"])
    shape = vol["tsdf"].shape
    vol["tsdf"] = ((rng.rand(*shape) + 0.05) * np.where(rng.rand(*shape) < 0.5, -1, 1)).astype(F)
    vol["weight"] = (2.0 * (rng.rand(*shape) < valid)).astype(F)
    if colour:
        vol["colour"] = (rng.rand(3, *shape) * 255).astype(F)
    if shift is not None:                                                       # a base that is not zero: roll by s and back in the arrays, keep the base
        sm.shift_volume(vol, (0, 0, 0))
        vol["base"] = vol["base"] + np.asarray(shift, np.int64)
        vol["origin"] = sm.origin(vol["origin0"], vol["base"], vol["vs"])
    return vol


def test_keys_of_a_5x3x2_mesh_against_the_mesh_definition():
    for seed, shift, box in ((1, None, None), (2, (7, -3, 100), None), (3, (-(1 << 24), 1 << 24, 5), ((1, 0, 0), (4, 3, 2))), (4, None, ((0, 1, 0), (5, 2, 1)))):
        vol = seeded((5, 3, 2), seed, shift=shift)
        lo, size = box if box else (None, None)
        xyz, tri, owner = mm.mesh_literal(vol, 1.0, lo, size)
        key = am.keys_of(vol, 1.0, lo, size)
        assert len(owner) >= 3 and key.dtype == np.int32
        base = am.base_of(vol)
        assert key.tolist() == [[i + int(base[0]), j + int(base[1]), k + int(base[2]), m] for i, j, k, m in owner], (seed, shift, box)
        assert len({tuple(r) for r in key.tolist()}) == len(key)                # within one mesh all keys are distinct
        p = am.piece(vol, 1.0, lo, size)
        assert mm.same_floats(p[0], xyz) and np.array_equal(p[1], tri)


def test_a_welded_two_piece_archive_is_the_whole_grid_mesh_at_every_cut():
    dims = (33, 17, 5)
    vol = seeded(dims, 11, colour=True)
    whole = am.piece(vol, 1.0, colour=True)
    want = am.key_triples(whole[1], whole[2])
    whole_by_key = {tuple(k): (whole[0][v].tobytes(), whole[3][v].tobytes()) for v, k in enumerate(whole[2].tolist())}
    assert len(whole[0]) > 2000 and len(want) > 2000
    n_cuts = 0
    for a in range(3):
        for cut in range(dims[a]):                                              # the shared layer: [0, cut] and [cut, n)
            lo_b = [0, 0, 0]
            size_a, size_b = list(dims), list(dims)
            size_a[a], lo_b[a], size_b[a] = cut + 1, cut, dims[a] - cut
            A, B = am.piece(vol, 1.0, (0, 0, 0), size_a, True), am.piece(vol, 1.0, lo_b, size_b, True)
            seam = am.seam_keys(A[2], B[2])
            assert all(k[a] == cut and not (k[3] >> a) & 1 for k in seam)       # the edges inside the layer
            for first, second in ((A, B), (B, A)):
                ar = am.FastArchive(True)
                n1, n2 = ar.append(*first), ar.append(*second)
                assert n1[1] == 0 and n2[1] == len(seam) and n1[0] + n2[0] == len(whole[0]), (a, cut)
                xyz, tri, rgba, key = ar.arrays()
                assert np.array_equal(am.key_triples(tri, key), want), (a, cut)
                # unchanged data: every vertex is the whole-grid mesh's, bit for bit, whichever piece brought it
                assert all(whole_by_key[tuple(k)] == (xyz[v].tobytes(), rgba[v].tobytes()) for v, k in enumerate(key.tolist()))
            n_cuts += 1
    assert n_cuts == 55
    # the literal archive and the vectorised one agree on a cut in the middle
    A, B = am.piece(vol, 1.0, (0, 0, 0), (17, 17, 5), True), am.piece(vol, 1.0, (16, 0, 0), (17, 17, 5), True)
    lit, fast = am.Archive(True), am.FastArchive(True)
    for ar in (lit, fast):
        ar.append(*A)
        ar.append(*B)
    for x, y in zip(lit.arrays(), fast.arrays()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


class ScriptedOps:
    """the calls nalo_tsdf_follow is made of, recorded"""

    def __init__(self, dims, origin, vs):
        self.g, self.log = dict(origin=np.asarray(origin, F), vs=F(vs), dims=tuple(dims)), []

    def geometry(self):
        self.log.append(("geometry",))
        return self.g

    def shift_for(self, g, centre, margin):
        self.log.append(("shift_for", tuple(centre), tuple(margin)))
        return sm.shift_for(g["origin"], g["vs"], g["dims"], centre, margin)

    def shift_boxes(self, dims, s):
        self.log.append(("shift_boxes", tuple(dims), tuple(s)))
        return sm.shift_boxes(dims, s)

    def archive_mesh(self, min_weight, box):
        self.log.append(("archive_mesh", min_weight, box))

    def shift(self, s):
        self.log.append(("shift", tuple(s)))


def test_the_call_sequence_of_the_models_follow_on_a_scripted_stub():
    """the model's follow(), which the device tests run next to nalo_tsdf_follow; the library's own sequence is not observable without a device"""
    ops = ScriptedOps((8, 6, 4), (0.0, 0.0, 0.0), 1.0)
    assert am.follow(ops, (4.5, 3.5, 2.5), (0, 0, 0), 1.0) == (0, 0, 0)         # the centre voxel is already at dims / 2
    assert ops.log == [("geometry",), ("shift_for", (4.5, 3.5, 2.5), (0, 0, 0)), ("shift", (0, 0, 0))]
    ops.log.clear()
    assert am.follow(ops, (6.5, 3.5, 0.5), (0, 0, 0), 2.0) == (2, 0, -2)
    boxes = sm.shift_boxes((8, 6, 4), (2, 0, -2))["boxes"]
    assert len(boxes) == 2 and boxes[0] == ((0, 0, 0), (3, 6, 4)) and boxes[1] == ((2, 0, 1), (6, 6, 3))
    assert ops.log == [("geometry",), ("shift_for", (6.5, 3.5, 0.5), (0, 0, 0)), ("shift_boxes", (8, 6, 4), (2, 0, -2)), ("archive_mesh", 2.0, boxes[0]),
                       ("archive_mesh", 2.0, boxes[1]), ("shift", (2, 0, -2))]
    ops.log.clear()
    assert am.follow(ops, (6.5, 3.5, 0.5), (2, 0, 1), 2.0) == (0, 0, -2)        # the dead band holds x
    assert [e[0] for e in ops.log] == ["geometry", "shift_for", "shift_boxes", "archive_mesh", "shift"]
