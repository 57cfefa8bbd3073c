"""The hand-off's Python layer without a GPU: binding.DeviceView (what frame_plane and trk_ref_export return) is built from hand-written descriptors, and
binding.trk_ref_view marshals per-level device arrays into nalo_trk_ref_view from `data`, `shape`, `typestr` and `strides` of __cuda_array_interface__ alone, so
stand-in objects exercise all of it (as tests/test_device_ingest_cpu.py does for dev_plane). That the library exports the five new symbols is test_abi_cpu.py's
test_library_exports_every_declared_symbol."""
import ctypes as C

import numpy as np
import pytest

from nalo_slam_amd import binding
from test_device_ingest_cpu import Fake, fields

P0 = 0x7F0000002000


def test_view_of_an_f32_plane():
    d = binding.DevPlane(P0, binding.DT_F32, 70, 34, 1, 280, 4, 0)
    v = binding.DeviceView.of_plane(d, stream=0x55AA, owner="ctx")
    cai = v.__cuda_array_interface__
    assert cai["shape"] == (34, 70) and cai["typestr"] == "<f4" and cai["strides"] is None and cai["data"] == (P0, False) and cai["version"] == 2
    assert v.stream == 0x55AA and v.owner == "ctx"
    assert fields(binding.dev_plane(v)) == fields(d)                         # and back: frame_ingest accepts it as any device array
    pitched = binding.DeviceView.of_plane(binding.DevPlane(P0, binding.DT_F32, 70, 34, 1, 512, 4, 0))
    assert pitched.__cuda_array_interface__["strides"] == (512, 4)
    assert fields(binding.dev_plane(pitched))[5:7] == (512, 4)


def test_view_of_the_interleaved_colour_plane():
    d = binding.DevPlane(P0, binding.DT_U8, 70, 34, 3, 210, 3, 1)
    v = binding.DeviceView.of_plane(d)
    cai = v.__cuda_array_interface__
    assert cai["shape"] == (34, 70, 3) and cai["typestr"] == "|u1" and cai["strides"] is None and cai["data"] == (P0, False)
    assert fields(binding.dev_plane(v, "hwc")) == fields(d)
    assert v.stream == 0


def test_view_of_an_empty_cloud():
    for ptr in (P0, 0, None):
        v = binding.DeviceView(ptr, (0,), "<f4")
        cai = v.__cuda_array_interface__
        assert cai["shape"] == (0,) and cai["typestr"] == "<f4" and cai["strides"] is None and cai["data"] == (ptr or 0, False)
    v = binding.DeviceView(P0, (595,), "<f4")
    assert v.__cuda_array_interface__["shape"] == (595,)


def test_struct_matches_the_header():
    names = [f[0] for f in binding.TrkRefView._fields_]
    assert names == ["w", "h", "levels", "slot_ref", "n", "u", "v", "idepth", "color", "idepth_map", "weight_sums", "fx", "fy", "cx", "cy", "stream"]
    assert binding.MAX_LEVELS == 6 and C.sizeof(binding.TrkRefView) == 16 + 24 + 6 * 48 + 4 * 24 + 8
    assert binding.TrkRefView.u.offset == 40 and binding.TrkRefView.fx.offset == 328 and binding.TrkRefView.stream.offset == 424
    assert (binding.PLANE_IRRADIANCE, binding.PLANE_MASK, binding.PLANE_COLOUR) == (0, 1, 2)
    for name in ("nalo_frame_plane", "nalo_trk_ref_export", "nalo_trk_ref_import", "nalo_trk_ref_release"):
        assert name in binding.EXPORTS


def test_intrinsics_follow_make_k():
    K = (72.8, 71.5, 69.5, 33.5)
    got = binding.pyr_intrinsics(K, 3)
    assert got.dtype == np.float32 and got.shape == (4, 3)
    assert got[:, 0].tolist() == [np.float32(k) for k in K]
    assert got[0, 2] == np.float32(np.float32(np.float32(72.8) * 0.5) * 0.5) and got[3, 1] == np.float32((float(np.float32(33.5)) + 0.5) / 2 - 0.5)
    assert got[2, 2] == np.float32((float(np.float32(69.5)) + 0.5) / 4 - 0.5)


def levels_140x68():
    """three levels of a 140x68 context: a cloud with maps, a cloud 4 bytes off a 16-byte boundary without maps, an empty level with flat maps"""
    return [dict(u=Fake((255,), "<f4", ptr=P0), v=Fake((255,), "<f4", ptr=P0 + 0x1000), idepth=Fake((255,), "<f4", ptr=P0 + 0x2000), color=Fake((255,), "<f4", ptr=P0 + 0x3000),
                 idepth_map=Fake((68, 140), "<f4", ptr=P0 + 0x10000), weight_sums=Fake((68, 140), "<f4", strides=(560, 4), ptr=P0 + 0x20000)),
            dict(u=Fake((5,), "<f4", strides=(4,), ptr=P0 + 0x4004), v=Fake((5,), "<f4", ptr=P0 + 0x5008), idepth=Fake((5,), "<f4", ptr=P0 + 0x600C), color=Fake((5,), "<f4", ptr=P0 + 0x7000)),
            dict(idepth_map=Fake((17 * 35,), "<f4", ptr=P0 + 0x30000), weight_sums=Fake((17 * 35,), "<f4", ptr=P0 + 0x31000), u=None, v=None, idepth=None, color=None)]


def test_marshalling_of_per_level_arrays():
    intr = binding.pyr_intrinsics((72.8, 72.8, 69.5, 33.5), 3)
    V = binding.trk_ref_view(140, 68, 3, levels_140x68(), intr, stream=0x1234, slot_ref=2)
    assert (V.w, V.h, V.levels, V.slot_ref, V.stream) == (140, 68, 3, 2, 0x1234)
    assert list(V.n) == [255, 5, 0, 0, 0, 0]
    assert [V.u[0], V.v[0], V.idepth[0], V.color[0]] == [P0, P0 + 0x1000, P0 + 0x2000, P0 + 0x3000]
    assert [V.u[1], V.v[1], V.idepth[1], V.color[1]] == [P0 + 0x4004, P0 + 0x5008, P0 + 0x600C, P0 + 0x7000]
    assert [V.u[2], V.v[2], V.idepth[2], V.color[2]] == [None] * 4
    assert [V.idepth_map[l] for l in range(6)] == [P0 + 0x10000, None, P0 + 0x30000, None, None, None]
    assert [V.weight_sums[l] for l in range(6)] == [P0 + 0x20000, None, P0 + 0x31000, None, None, None]
    for k, name in enumerate(("fx", "fy", "cx", "cy")):
        assert [np.float32(getattr(V, name)[l]) for l in range(3)] == intr[k].tolist()
    assert binding.trk_ref_view(140, 68, 3, levels_140x68(), intr).stream is None             # 0 / None: the null stream
    # an empty cloud given as arrays of length 0: n = 0 and no pointer is passed on
    lv = levels_140x68()
    lv[1] = dict(u=Fake((0,), "<f4", ptr=0), v=Fake((0,), "<f4", ptr=0), idepth=Fake((0,), "<f4", ptr=0), color=Fake((0,), "<f4", ptr=0))
    V = binding.trk_ref_view(140, 68, 3, lv, intr)
    assert V.n[1] == 0 and V.u[1] is None and V.color[1] is None


def test_the_view_keeps_its_arrays_alive():
    import gc
    import weakref
    lv = levels_140x68()
    r = weakref.ref(lv[0]["idepth_map"])
    V = binding.trk_ref_view(140, 68, 3, lv, binding.pyr_intrinsics((72.8, 72.8, 69.5, 33.5), 3))
    del lv
    gc.collect()
    assert r() is not None
    del V
    gc.collect()
    assert r() is None


def test_marshalling_refusals():
    intr = binding.pyr_intrinsics((72.8, 72.8, 69.5, 33.5), 3)
    def refused(match, mutate, exc=binding.NaloError, **kw):
        lv = levels_140x68()
        mutate(lv)
        with pytest.raises(exc, match=match):
            binding.trk_ref_view(140, 68, kw.get("levels", 3), lv, kw.get("intr", intr))
    refused("come together", lambda lv: lv[0].update(color=None))
    refused("equal length", lambda lv: lv[0].update(v=Fake((254,), "<f4")))
    refused("1-D arrays", lambda lv: lv[1].update({k: Fake((5, 1), "<f4") for k in ("u", "v", "idepth", "color")}))
    refused("together or not at all", lambda lv: lv[0].update(weight_sums=None))
    refused("expected one of", lambda lv: lv[0].update(idepth_map=Fake((140, 68), "<f4")))
    refused("expected one of", lambda lv: lv[2].update(idepth_map=Fake((34, 70), "<f4")))
    refused("float32", lambda lv: lv[0].update(u=Fake((255,), "<f8")))
    refused("float32", lambda lv: lv[0].update(idepth_map=Fake((68, 140), "<i4")))
    refused("not dense", lambda lv: lv[0].update(u=Fake((255,), "<f4", strides=(8,))))
    refused("not dense", lambda lv: lv[0].update(idepth_map=Fake((68, 140), "<f4", strides=(1024, 4))))
    refused("__cuda_array_interface__", lambda lv: lv[0].update(u=np.zeros(255, np.float32)), exc=TypeError)
    refused("levels described", lambda lv: lv.pop())
    refused("levels described", lambda lv: None, levels=4)
    refused("intrinsics", lambda lv: None, intr=intr[:, :2])
