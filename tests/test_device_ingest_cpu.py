"""binding.dev_plane without a GPU: the descriptor of nalo_frame_ingest_device is built from `data`, `shape`, `typestr` and `strides` of
__cuda_array_interface__ alone, so stand-in objects with a hand-written interface exercise all of it. (That the library exports the new symbols is
test_abi_cpu.py's test_library_exports_every_declared_symbol.)"""
import numpy as np
import pytest

from nalo_slam_amd import binding


class Fake:
    def __init__(self, shape, typestr, strides=None, ptr=0x7F0000001000):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, strides=strides, data=(ptr, False), version=2)


def fields(d):
    return (d.ptr, d.dtype, d.w, d.h, d.channels, d.stride_y, d.stride_x, d.stride_c)


@pytest.mark.parametrize("typestr,dt,item", [("<u1", binding.DT_U8, 1), ("|u1", binding.DT_U8, 1), ("<u2", binding.DT_U16, 2), ("<i4", binding.DT_I32, 4), ("<f4", binding.DT_F32, 4)])
def test_contiguous_plane_and_dtype_table(typestr, dt, item):
    d = binding.dev_plane(Fake((51, 99), typestr))                           # strides None: C-contiguous
    assert fields(d) == (0x7F0000001000, dt, 99, 51, 1, 99 * item, item, 0)
    assert (binding.DT_U8, binding.DT_U16, binding.DT_I32, binding.DT_F32) == (1, 2, 3, 4)


def test_strided_planes():
    # a pitched region of a 2-byte tensor 120 wide, and an x-strided view of it
    assert fields(binding.dev_plane(Fake((51, 99), "<u2", strides=(240, 2), ptr=4096 + 3 * 240 + 10)))[1:] == (binding.DT_U16, 99, 51, 1, 240, 2, 0)
    assert fields(binding.dev_plane(Fake((51, 60), "<u2", strides=(240, 4))))[1:] == (binding.DT_U16, 60, 51, 1, 240, 4, 0)
    assert fields(binding.dev_plane(Fake((51, 99), "<f4", strides=(0, 4))))[5:7] == (0, 4)      # a zero row stride is the library's to judge, not the builder's


def test_hwc_against_chw():
    hwc = binding.dev_plane(Fake((34, 70, 3), "|u1"), "hwc")
    chw = binding.dev_plane(Fake((3, 34, 70), "|u1"), "chw")
    assert fields(hwc)[1:] == (binding.DT_U8, 70, 34, 3, 210, 3, 1)
    assert fields(chw)[1:] == (binding.DT_U8, 70, 34, 3, 70, 1, 34 * 70)
    pitched = binding.dev_plane(Fake((34, 70, 3), "|u1", strides=(256, 3, 1)), "hwc")
    assert fields(pitched)[5:] == (256, 3, 1)
    planar_pitched = binding.dev_plane(Fake((3, 34, 70), "|u1", strides=(34 * 128, 128, 1)), "chw")
    assert fields(planar_pitched)[5:] == (128, 1, 34 * 128)
    single = binding.dev_plane(Fake((34, 70, 1), "<f4"), "hwc")              # one channel through a 3-D shape
    assert fields(single)[1:5] == (binding.DT_F32, 70, 34, 1)


def test_the_plane_keeps_its_array_alive():
    import gc
    import weakref
    f = Fake((4, 4), "|u1")
    r = weakref.ref(f)
    d = binding.dev_plane(f)
    del f
    gc.collect()
    assert r() is not None
    del d
    gc.collect()
    assert r() is None


@pytest.mark.parametrize("typestr", ["<f8", ">u2", ">f4", "<i2", "<i8", "|b1", "<f2"])
def test_dtypes_outside_the_table_are_refused(typestr):
    with pytest.raises(binding.NaloError, match="outside the table"):
        binding.dev_plane(Fake((8, 8), typestr))


def test_negative_strides_are_refused():
    with pytest.raises(binding.NaloError, match="negative strides"):
        binding.dev_plane(Fake((8, 8), "|u1", strides=(-8, 1)))
    with pytest.raises(binding.NaloError, match="negative strides"):
        binding.dev_plane(Fake((8, 8, 3), "|u1", strides=(24, 3, -1)), "hwc")


def test_shapes_that_do_not_fit_are_refused():
    with pytest.raises(binding.NaloError, match="does not fit"):
        binding.dev_plane(Fake((8, 8, 3), "|u1"))                            # three dimensions need a layout
    with pytest.raises(binding.NaloError, match="does not fit"):
        binding.dev_plane(Fake((8, 8), "|u1"), "hwc")
    with pytest.raises(binding.NaloError, match="2 channels"):
        binding.dev_plane(Fake((8, 8, 2), "|u1"), "hwc")
    with pytest.raises(binding.NaloError, match="channels_layout"):
        binding.dev_plane(Fake((8, 8, 3), "|u1"), "cwh")
    with pytest.raises(binding.NaloError, match="strides"):
        binding.dev_plane(Fake((8, 8), "|u1", strides=(8,)))


def test_a_numpy_array_is_refused():
    """host memory never becomes a descriptor: no silent copy to the device"""
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        binding.dev_plane(np.zeros((8, 8), np.uint8))
    with pytest.raises(TypeError):
        binding.dev_plane([[0, 1], [2, 3]])


def test_structs_match_the_header():
    """the ctypes mirrors against the C declaration: field order and, on the LP64 hosts the library builds for, the sizes"""
    import ctypes as C
    assert [f[0] for f in binding.DevPlane._fields_] == ["ptr", "dtype", "w", "h", "channels", "stride_y", "stride_x", "stride_c"]
    assert C.sizeof(binding.DevPlane) == 48
    assert [f[0] for f in binding.FrameIngestArgs._fields_] == ["image", "exposure_time", "factor", "mask", "colour", "colour_is_rgb", "gammaB", "producer_stream"]
    assert C.sizeof(binding.FrameIngestArgs) == 56
    for name in ("nalo_frame_ingest_device", "nalo_frame_release", "nalo_dev_plane_check", "nalo_frame_attach"):
        assert name in binding.EXPORTS
