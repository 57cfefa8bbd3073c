"""Frames, masks and colour that already live on the device: nalo_frame_ingest_device / nalo_frame_release / nalo_dev_plane_check / nalo_frame_attach
(ingest_dev_kernel<DT, PHOTO, ROWCONTIG>, ingest_f32_kernel, attach_kernel<MDT>; kernels_ingest_dev.hip) against the host routes - nalo_frame_upload_raw and
nalo_frame_upload, which test_frontend_edges_gpu.py pins against the CPU oracle at the same shapes - and against the oracle itself (orc_undistort,
orc_resize_nearest_u8). The planes are torch tensors; every comparison is bit for bit (same_bits: uint32 words, NaN by position; `bits` where the payload counts).

Shapes, tables and images are test_frontend_edges_gpu.py's: 72x40 and 70x34 from 99x51 give the ingest a partial last workgroup and a partial last wave, over
the planted remap table (first pixels, both sides of every 256-lane stride and workgroup border, the last legal taps)."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import orc
from nalo_slam_amd import binding
from test_frontend_edges_gpu import (ERR_ARG, ERR_STATE, GAMMA, HO, INGEST_SIZES, WO, assert_pyramids_equal, context, gpu_pyramid, make_image, planted_remap,
                                     raw_image, response, same_bits, vignette_inv)
from test_ingest_gpu import radial_remap

pytestmark = pytest.mark.gpu


def dev(a):
    """a host array as a torch tensor on the device (uint16 included)"""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def ingest_case(dtype, photometric, remap, w, h):
    """(wo, ho, G, vinv, rx, ry, raw) of test_ingest_every_instantiation"""
    G = response(256 if dtype == np.uint8 else 65536)
    wo, ho = (WO, HO) if remap else (w, h)
    rx, ry, taps = planted_remap(w, h, wo, ho) if remap else (None, None, [(0, 0), (wo - 2, ho - 2), (5, 5), (6, 8)])
    return wo, ho, G, vignette_inv(wo, ho), rx, ry, raw_image(dtype, wo, ho, taps, seed=w + photometric)


# ------------------------------------------------------------------------------------------------ 1. every instantiation
@pytest.mark.parametrize("remap", [True, False], ids=["remap", "passthrough"])
@pytest.mark.parametrize("photometric", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_device_ingest_every_instantiation(dtype, photometric, remap):
    """ingest_dev_kernel<1 / 2, 0 / 1 / 2, row-contiguous> with and without the remap: slot 0 from a torch tensor, slot 1 through nalo_frame_upload_raw"""
    for w, h, levels in INGEST_SIZES:
        wo, ho, G, vinv, rx, ry, raw = ingest_case(dtype, photometric, remap, w, h)
        t = dev(raw)
        c = context(w, h, levels, n_slots=2)
        try:
            c.undist_set(wo, ho, G, vinv if photometric == 2 else None, photometric, rx, ry)
            for exposure in (0.02, 0.0):
                ph = photometric if exposure > 0 else 0
                c.frame_ingest(0, image=t, exposure=exposure, factor=0.5)
                c.frame_upload_raw(1, raw, exposure=exposure, factor=0.5)
                got, host = gpu_pyramid(c, 0), gpu_pyramid(c, 1)
                assert_pyramids_equal(got, host, (w, h, exposure, "device route against host route"))
                assert same_bits(got[0][0][:, 0], orc.undistort(raw, G, vinv if ph == 2 else None, ph, 0.5, rx, ry, w, h)), (w, h, exposure, "level-0 irradiance")
        finally:
            c.close()
            torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. strides
@pytest.mark.parametrize("remap", [True, False], ids=["remap", "passthrough"])
@pytest.mark.parametrize("photometric", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_strided_sensor_frames(dtype, photometric, remap):
    """the same frames as a pitched region of a larger tensor (row-contiguous kernel with a row pitch) and as an x-strided view (one load per tap). Outside the
    described plane the larger tensors hold the type's maximum or 0 - raw_image puts 0 and the maximum under the planted taps, so a tap read one pixel or one
    row off changes the result"""
    top = int(np.iinfo(dtype).max)
    for w, h, levels in INGEST_SIZES:
        wo, ho, G, vinv, rx, ry, raw = ingest_case(dtype, photometric, remap, w, h)
        c = context(w, h, levels, n_slots=2)
        try:
            c.undist_set(wo, ho, G, vinv if photometric == 2 else None, photometric, rx, ry)
            c.frame_ingest(1, image=dev(raw), exposure=0.02, factor=0.5)
            want = gpu_pyramid(c, 1)
            for fill in (top, 0):
                big = np.full((ho + 7, wo + 11), fill, dtype)
                big[3:3 + ho, 5:5 + wo] = raw
                roi = dev(big)[3:3 + ho, 5:5 + wo]
                assert not roi.is_contiguous() and roi.stride(1) == 1
                c.frame_ingest(0, image=roi, exposure=0.02, factor=0.5)
                assert_pyramids_equal(gpu_pyramid(c, 0), want, (w, h, "pitched", fill))
                wide = np.full((ho, 2 * wo), fill, dtype)
                wide[:, ::2] = raw
                view = dev(wide)[:, ::2]
                assert view.stride(1) == 2 and tuple(view.shape) == (ho, wo)
                c.frame_ingest(0, image=view, exposure=0.02, factor=0.5)
                assert_pyramids_equal(gpu_pyramid(c, 0), want, (w, h, "x-strided", fill))
        finally:
            c.close()
            torch.cuda.synchronize()


def special_image(w, h, seed):
    """make_image with +inf, -inf, two quiet NaNs that carry a payload and -0.0 at interior pixels, at the image's corners and in the tail"""
    img = make_image(w, h, seed=seed)
    b = img.view(np.uint32)
    img[h // 2, w // 2], img[h // 3, w // 3], img[h - 1, w - 1], img[0, 0] = np.inf, -np.inf, -0.0, -0.0
    b[h // 2 + 1, w // 3], b[h - 2, w - 2], b[h - 1, w - 3] = 0x7FC12345, 0xFFC00001, 0x7FC00042
    return img


# ------------------------------------------------------------------------------------------------ 3. rectified F32 image
@pytest.mark.parametrize("w,h,levels", INGEST_SIZES, ids=["72x40", "70x34"])
def test_f32_image(w, h, levels):
    """a rectified irradiance image: contiguous and as a pitched view, with and without gammaB, equal to nalo_frame_upload; level 0 carries the input's words"""
    img = special_image(w, h, seed=3)
    c = context(w, h, levels, n_slots=2)
    try:
        big = np.full((h + 5, w + 9), np.float32(1e30), np.float32)
        big[2:2 + h, 6:6 + w] = img
        planes = {"contiguous": dev(img), "pitched": dev(big)[2:2 + h, 6:6 + w], "x-strided": dev(np.repeat(img, 2, axis=1))[:, ::2]}
        for B in (None, GAMMA):
            c.frame_upload(1, img, gammaB=B)
            want = gpu_pyramid(c, 1)
            for name, t in planes.items():
                c.frame_ingest(0, image=t, gammaB=B)
                got = gpu_pyramid(c, 0)
                assert_pyramids_equal(got, want, (w, h, name, B is not None))
                assert np.array_equal(bits(got[0][0][:, 0]), bits(want[0][0][:, 0])), (name, "level 0 against the host route, NaN payloads included")
                assert np.array_equal(bits(got[0][0][:, 0]), bits(img)), (name, "level 0 against the input's words")
    finally:
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. mask and colour
def resize_words(src, w, h):
    """cv::resize(INTER_NEAREST) of a plane of 4-byte elements through the oracle's byte resize (four channels)"""
    ho, wo = src.shape
    return orc.resize_nearest_u8(np.ascontiguousarray(src).view(np.uint8).reshape(ho, wo, 4), w, h).reshape(h, w * 4).view(src.dtype)


def sampled(dst, n, nOrg):
    """the source index cv::resize(INTER_NEAREST) reads for destination index dst: where a planted value has to sit to arrive (the expected planes themselves
    come from the oracle)"""
    return min(int(math.floor(dst * (1.0 / (n / nOrg)))), nOrg - 1)


MASK_CASES = [(70, 34, 105, 51), (70, 34, 96, 53), (70, 34, 48, 27), (70, 34, 70, 34), (70, 33, 105, 51), (70, 33, 70, 33)]


@pytest.mark.parametrize("w,h,wo,ho", MASK_CASES, ids=["%dx%d_from_%dx%d" % m for m in MASK_CASES])
def test_mask_and_colour(w, h, wo, ho):
    """attach_kernel<U8 / I32 / F32> with colour in every layout; 70x33 = 2310 pixels is no multiple of four and its rows split a lane's four pixels"""
    rng = np.random.RandomState(wo + h)
    raw = rng.randint(0, 256, (ho, wo)).astype(np.uint8)
    mask_o = rng.randint(0, 256, (ho, wo)).astype(np.uint8)
    mask_o[0, 0], mask_o[-1, -1], mask_o[0, -1], mask_o[-1, 0] = 0, 255, 254, 253
    bgr_o = rng.randint(0, 256, (ho, wo, 3)).astype(np.uint8)
    rx, ry = radial_remap(w, h, wo, ho)
    want_m, want_b = orc.resize_nearest_u8(mask_o, w, h).astype(np.float32), orc.resize_nearest_u8(bgr_o, w, h)
    if (wo, ho) == (w, h):
        assert np.array_equal(want_m, mask_o.astype(np.float32)) and np.array_equal(want_b, bgr_o)      # the formula is the identity at equal size
    c = context(w, h, n_slots=2)
    try:
        c.undist_set(wo, ho, None, None, 0, rx, ry)
        c.frame_upload_raw(1, raw, mask_org=mask_o, bgr_org=bgr_o)                                      # the host route
        host_m, host_b = c.frame_download_mask(1)
        assert np.array_equal(host_m, want_m) and np.array_equal(host_b, want_b)
        t_raw = dev(raw)
        # U8 mask, colour in every layout and order
        pitched = np.full((ho, wo + 9, 3), 255, np.uint8)
        pitched[:, 4:4 + wo] = bgr_o
        rgb_o = np.ascontiguousarray(bgr_o[:, :, ::-1])
        colours = [("hwc-bgr", dev(bgr_o), "hwc", "bgr"), ("hwc-rgb", dev(rgb_o), "hwc", "rgb"),
                   ("chw-bgr", dev(bgr_o.transpose(2, 0, 1)), "chw", "bgr"), ("chw-rgb", dev(rgb_o.transpose(2, 0, 1)), "chw", "rgb"),
                   ("hwc-bgr pitched view", dev(pitched)[:, 4:4 + wo], "hwc", "bgr"), ("chw view of hwc memory", dev(bgr_o).permute(2, 0, 1), "chw", "bgr")]
        t_mask = dev(mask_o)
        for name, t, layout, order in colours:
            c.frame_ingest(0, image=t_raw, mask=t_mask, colour=t, colour_layout=layout, colour_order=order)
            m, b = c.frame_download_mask(0)
            assert m.dtype == np.float32 and np.array_equal(bits(m), bits(want_m)), name
            assert np.array_equal(b, want_b), name
        assert_pyramids_equal(gpu_pyramid(c, 0), gpu_pyramid(c, 1), "the image under mask and colour")
        # I32 mask: (float)v, round to nearest even
        mi = rng.randint(-2 ** 31, 2 ** 31, (ho, wo), dtype=np.int64).astype(np.int32)
        at = lambda y, x: (sampled(y, h, ho), sampled(x, w, wo))             # destination pixel -> its source pixel
        mi[at(0, 0)], mi[at(h - 1, w - 1)], mi[at(h // 2, w // 2)], mi[at(0, w - 1)], mi[at(h - 1, 0)] = -2 ** 31, 2 ** 24 + 1, -1, 2 ** 31 - 1, 2 ** 24 + 3
        want_i = resize_words(mi, w, h)
        assert {-2 ** 31, 2 ** 24 + 1, -1, 2 ** 31 - 1, 2 ** 24 + 3} <= set(want_i.reshape(-1).tolist())
        c.frame_ingest(0, image=None, mask=dev(mi))
        assert np.array_equal(bits(c.frame_download_mask(0, bgr=False)[0]), bits(want_i.astype(np.float32)))
        assert np.float32(2 ** 24 + 1) == 2 ** 24 and np.float32(2 ** 24 + 3) == 2 ** 24 + 4              # what "nearest even" means at these values
        # F32 mask: the words as they are
        mf = (rng.rand(ho, wo) * 255).astype(np.float32)
        fb = mf.view(np.uint32)
        mf[at(h - 1, w - 1)], mf[at(h // 2, w // 2)], mf[at(0, w - 1)] = -0.0, np.inf, -np.inf
        fb[at(0, 0)], fb[at(h - 1, 0)], fb[at(h // 2, 0)], fb[at(h // 2, w // 3)] = 0x7FC54321, 0xFFC00007, 0x00000001, 0x807FFFFF     # NaN payloads, the smallest and a negative denormal
        want_f = resize_words(mf, w, h)
        assert {0x7FC54321, 0xFFC00007, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF} <= set(bits(want_f).tolist())
        wide = np.zeros((ho, 2 * wo), np.float32)
        wide[:, ::2] = mf
        for name, t in (("contiguous", dev(mf)), ("x-strided", dev(wide)[:, ::2])):
            c.frame_ingest(0, image=None, mask=t)
            assert np.array_equal(bits(c.frame_download_mask(0, bgr=False)[0]), bits(want_f)), name
        assert np.array_equal(c.frame_download_mask(0, mask=False)[1], want_b)                           # the colour of the last full ingest stayed
    finally:
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. attach to a tracked frame
def test_attach_to_a_tracked_frame():
    """nalo_frame_upload_raw_async brings the frame in, tracking makes it a keyframe, mask and colour follow: from the host (nalo_frame_attach) on one context,
    from the device (image = NULL) on its twin. Both equal the slot that nalo_frame_upload_raw filled with everything at once, and the pyramid stays."""
    w, h, levels = 72, 40, 4
    rx, ry, taps = planted_remap(w, h, WO, HO)
    G, vinv = response(256), vignette_inv(WO, HO)
    raw = raw_image(np.uint8, WO, HO, taps, seed=9)
    rng = np.random.RandomState(17)
    mask_o = rng.randint(0, 200, (HO, WO)).astype(np.uint8)
    mask_o[:, :WO // 5] = 0
    bgr_o = rng.randint(0, 256, (HO, WO, 3)).astype(np.uint8)
    rp, draws = rng.randint(0, 256, w * h).astype(np.uint8), rng.randint(0, 2 ** 31 - 1, w * h).astype(np.int32)
    ctxs = [context(w, h, levels, n_slots=3), context(w, h, levels, n_slots=3)]
    try:
        before = []
        for c in ctxs:
            c.undist_set(WO, HO, G, vinv, 2, rx, ry)
            c.pixsel_set_random(rp, draws)
            pinned = c.pinned_array((HO, WO), np.uint8)
            pinned[:] = raw
            c.frame_upload_raw_async(0, pinned, exposure=0.02)
            c.frame_wait(0)
            before.append(gpu_pyramid(c, 0))
            with pytest.raises(binding.NaloError, match="error %d" % ERR_STATE):
                c.frame_download_mask(0)                                                                 # a tracked frame: neither mask nor colour
        host, devc = ctxs
        host.frame_upload_raw(1, raw, exposure=0.02, mask_org=mask_o, bgr_org=bgr_o)                    # everything at once
        want_m, want_b = host.frame_download_mask(1)
        want_map, want_num = host.pixsel_make_maps_lidar(1, 3)
        assert want_num > 0 and (want_m > 0).any()
        host.frame_attach(0, mask_org=mask_o, bgr_org=bgr_o)
        devc.frame_ingest(0, image=None, mask=dev(mask_o), colour=dev(bgr_o))
        for c, k, name in ((host, 0, "host attach"), (devc, 1, "device attach")):
            m, b = c.frame_download_mask(0)
            assert np.array_equal(bits(m), bits(want_m)) and np.array_equal(b, want_b), name
            assert_pyramids_equal(gpu_pyramid(c, 0), before[k], name + ": the pyramid stays")
            assert_pyramids_equal(before[k], gpu_pyramid(host, 1), name)
            got_map, got_num = c.pixsel_make_maps_lidar(0, 3)                                            # one consumer of the mask sees the attached plane
            assert got_num == want_num and np.array_equal(got_map, want_map), name
        # one plane at a time: the other stays
        host.frame_attach(0, mask_org=np.zeros((HO, WO), np.uint8))
        m, b = host.frame_download_mask(0)
        assert not m.any() and np.array_equal(b, want_b)
        # a slot without a pyramid
        with pytest.raises(binding.NaloError, match="error %d" % ERR_STATE):
            host.frame_attach(2, mask_org=mask_o)
        with pytest.raises(binding.NaloError, match="error %d" % ERR_STATE):
            devc.frame_ingest(2, image=None, mask=dev(mask_o))
        with pytest.raises(binding.NaloError, match="error %d" % ERR_STATE):
            devc.frame_download_mask(2)
    finally:
        for c in ctxs:
            c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. stream order
def test_stream_order_without_a_host_wait():
    """the planes are produced by work queued on a non-default torch stream: wrong data, a chain of matmuls of at least 0.2 s, then the right data. The call
    returns while the chain is still running (it made no host wait) and the pyramid is the right data's; with release=True the tensor may be overwritten on
    that stream at once"""
    w, h, levels = 72, 40, 4
    wo, ho, G, vinv, rx, ry, raw = ingest_case(np.uint8, 2, True, w, h)
    c = context(w, h, levels, n_slots=2)
    try:
        c.undist_set(wo, ho, G, vinv, 2, rx, ry)
        c.frame_upload_raw(1, raw, exposure=0.02)
        want = gpu_pyramid(c, 1)
        right, wrong = dev(raw), dev(255 - raw)
        t = torch.empty_like(right)
        c.frame_ingest(0, image=wrong, exposure=0.02)                       # steady state: buffers and events exist, and the slot holds the wrong data's pyramid
        c.sync()
        a = torch.randn(4096, 4096, device="cuda")
        out = torch.empty_like(a)
        S = torch.cuda.Stream()
        with torch.cuda.stream(S):
            torch.mm(a, a, out=out)                                          # warm-up: the library's first call
            S.synchronize()
            t0 = time.perf_counter()
            torch.mm(a, a, out=out)
            S.synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
            reps = min(int(math.ceil(0.25 / one)) + 1, 20000)                # 0.2 s and a quarter more
            for release in (False, True):
                t.copy_(wrong)
                for _ in range(reps):
                    torch.mm(a, a, out=out)
                t.copy_(right)
                behind = torch.cuda.Event()
                behind.record(S)
                c.frame_ingest(0, image=t, exposure=0.02, release=release)  # stream=None: torch's current stream, S
                returned_early = not behind.query()
                if release:
                    t.fill_(77)                                              # garbage, on S, directly after the call
                else:
                    c.frame_wait(0)                                          # the host form of the same wait
                    t.fill_(78)
                assert returned_early, "nalo_frame_ingest_device waited for the producer stream (release=%s, %d matmuls of %.2e s)" % (release, reps, one)
                assert_pyramids_equal(gpu_pyramid(c, 0), want, ("stream order", release))
                S.synchronize()
    finally:
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. refusals
def plane(ptr, dtype=binding.DT_U8, w=64, h=64, channels=1, sy=64, sx=1, sc=0):
    return binding.DevPlane(ptr, dtype, w, h, channels, sy, sx, sc)


def ingest_rc(c, slot, image=None, mask=None, colour=None, exposure=0.02):
    """nalo_frame_ingest_device with hand-made descriptors, past the checks of the Python layer -> return code"""
    p = lambda d: None if d is None else C.pointer(d)
    a = binding.FrameIngestArgs(p(image), exposure, 1.0, p(mask), p(colour), 0, None, None)
    return c.L.nalo_frame_ingest_device(c.h_, slot, C.byref(a))


def slot_state(c, slot):
    m, b = c.frame_download_mask(slot)
    return gpu_pyramid(c, slot), m, b


def assert_slot_unchanged(c, slot, state, tag):
    pyr, m, b = slot_state(c, slot)
    assert_pyramids_equal(pyr, state[0], tag)
    assert np.array_equal(bits(m), bits(state[1])) and np.array_equal(b, state[2]), tag


def test_plane_check_refusals():
    """every memory-related refusal on nalo_dev_plane_check, which launches nothing; a good descriptor passes before, between and after (no sticky error)"""
    w, h = 72, 40
    c = context(w, h, 4)
    try:
        rng = np.random.RandomState(1)
        c.frame_upload(0, make_image(w, h), mask=rng.rand(h, w).astype(np.float32), bgr=rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        state = slot_state(c, 0)
        t = torch.zeros(64, 64, dtype=torch.uint8, device="cuda")           # 4 KB
        t16 = torch.zeros(64, 64, dtype=torch.int32, device="cuda").view(torch.uint8)
        good = binding.dev_plane(t)
        c.dev_plane_check(good)
        host_arr = np.zeros((64, 64), np.uint8)
        pinned = c.pinned_array((64, 64), np.uint8)
        p = t.data_ptr()
        bad = {
            "a numpy array's address": plane(host_arr.ctypes.data),
            "a pinned host array": plane(pinned.ctypes.data),
            "a null pointer": plane(None),
            "a dtype outside the table": plane(p, dtype=9),
            "dtype 0": plane(p, dtype=0),
            "two channels": plane(p, channels=2, sx=2, sc=1, w=32),
            "w = 0": plane(p, w=0),
            "h = 0": plane(p, h=0),
            "a negative row stride": plane(p + 63 * 64, sy=-64),
            "a negative pixel stride": plane(p + 63, sx=-1),
            "1 GiB of rows over a 4 KB tensor": plane(p, h=1 << 20, sy=1024),
            "a pixel stride of 0": plane(p, sx=0),
            "16-bit elements one byte apart": plane(t16.data_ptr(), dtype=binding.DT_U16, w=32, sx=1),
            "16-bit elements at an odd address": plane(t16.data_ptr() + 1, dtype=binding.DT_U16, w=16, h=16, sx=2),
            "channels that overlap inside a row": plane(p, channels=3, w=16, sx=2, sc=1),
            "planar channels inside the row": plane(p, channels=3, w=16, sx=1, sc=8, h=1),
        }
        for name, d in bad.items():
            assert c.L.nalo_dev_plane_check(c.h_, C.byref(d)) == ERR_ARG, name
            with pytest.raises(binding.NaloError, match="error %d" % ERR_ARG):
                c.dev_plane_check(d)
            c.dev_plane_check(good)
        assert c.L.nalo_dev_plane_check(c.h_, None) == ERR_ARG
        # descriptors at the limits that ARE the tensor's: accepted
        c.dev_plane_check(plane(p, channels=3, w=21, sx=3, sc=1))
        c.dev_plane_check(plane(p, channels=3, w=64, h=21, sx=1, sc=21 * 64))
        c.dev_plane_check(plane(p + 64 * 64 - 1, w=1, h=1))
        c.dev_plane_check(plane(p, sy=0))                                    # one row read 64 times overlaps nothing inside a row
        a = torch.ones(8, device="cuda") * 2                                 # the runtime is as it was: no error left behind
        assert float(a.sum().item()) == 16.0
        assert_slot_unchanged(c, 0, state, "after the refused descriptors")
    finally:
        c.close()
        torch.cuda.synchronize()


def test_ingest_refusals_leave_the_slot():
    """what nalo_frame_ingest_device itself refuses, each time with a filled slot that stays bit-identical. No refusal is followed by a call that would use the
    refused input."""
    w, h, levels = 72, 40, 4
    rx, ry, taps = planted_remap(w, h, WO, HO)
    raw = raw_image(np.uint8, WO, HO, taps, seed=5)
    rng = np.random.RandomState(2)
    img, mask, bgr = make_image(w, h), rng.rand(h, w).astype(np.float32), rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    c = context(w, h, levels, n_slots=2)
    try:
        c.frame_upload(0, img, mask=mask, bgr=bgr)
        state = slot_state(c, 0)
        t8, t16 = dev(raw), dev(raw.astype(np.uint16) * 257)
        good_mask = binding.dev_plane(dev(np.zeros((HO, WO), np.uint8)))
        # before nalo_undist_set
        assert ingest_rc(c, 0, image=binding.dev_plane(t8)) == ERR_STATE
        with pytest.raises(binding.NaloError, match="error %d.*has not run" % ERR_STATE):
            c.frame_ingest(0, image=t8)
        assert_slot_unchanged(c, 0, state, "before undist_set")
        c.undist_set(WO, HO, response(256), None, 1, rx, ry)
        refused = {
            "a sensor image of the wrong size": (dict(image=binding.dev_plane(dev(raw[:-1]))), ERR_ARG),
            "a sensor image in the rectified size": (dict(image=binding.dev_plane(dev(np.zeros((h, w), np.uint8)))), ERR_ARG),
            "an F32 image of the wrong size": (dict(image=binding.dev_plane(dev(np.zeros((h, w + 2), np.float32)))), ERR_ARG),
            "an F32 plane in the sensor's size": (dict(image=binding.dev_plane(dev(np.zeros((HO, WO), np.float32)))), ERR_ARG),
            "U16 over a 256-entry response": (dict(image=binding.dev_plane(t16)), ERR_ARG),
            "an I32 plane as the image": (dict(image=binding.dev_plane(dev(np.zeros((HO, WO), np.int32)))), ERR_ARG),
            "a 3-channel plane as the image": (dict(image=binding.dev_plane(dev(np.zeros((HO, WO, 3), np.uint8)), "hwc")), ERR_ARG),
            "a U16 mask": (dict(image=binding.dev_plane(t8), mask=binding.dev_plane(t16)), ERR_ARG),
            "a 3-channel mask": (dict(image=binding.dev_plane(t8), mask=binding.dev_plane(dev(np.zeros((h, w, 3), np.uint8)), "hwc")), ERR_ARG),
            "a one-channel colour": (dict(image=binding.dev_plane(t8), colour=binding.dev_plane(t8)), ERR_ARG),
            "an F32 colour": (dict(image=binding.dev_plane(t8), colour=binding.dev_plane(dev(np.zeros((h, w, 3), np.float32)), "hwc")), ERR_ARG),
            "a good image with a mask in host memory": (dict(image=binding.dev_plane(t8), mask=plane(np.zeros((64, 64), np.uint8).ctypes.data)), ERR_ARG),
            "no plane at all": (dict(), ERR_ARG),
        }
        for name, (kw, code) in refused.items():
            assert ingest_rc(c, 0, **kw) == code, name
            assert_slot_unchanged(c, 0, state, name)
        for slot in (-1, 2, 5):
            assert ingest_rc(c, slot, image=binding.dev_plane(t8)) == ERR_ARG
            assert c.L.nalo_frame_release(c.h_, slot, None) == ERR_ARG
        assert ingest_rc(c, 1, mask=good_mask) == ERR_STATE                  # attach to an empty slot
        assert c.L.nalo_frame_ingest_device(c.h_, 0, None) == ERR_ARG
        assert_slot_unchanged(c, 0, state, "after every refusal")
        # what the Python layer stops before the library is called
        with pytest.raises(TypeError):
            c.frame_ingest(0, image=raw)                                     # a numpy array: no silent copy to the device
        with pytest.raises(binding.NaloError, match="outside the table"):
            c.frame_ingest(0, image=dev(raw.astype(np.float64)))
        with pytest.raises(binding.NaloError, match="negative strides|does not fit"):
            c.frame_ingest(0, image=dev(np.zeros((HO, WO, 3), np.uint8)))
        with pytest.raises(binding.NaloError, match="colour_layout"):
            c.frame_ingest(0, image=t8, colour=dev(bgr), colour_layout="cwh")
        assert_slot_unchanged(c, 0, state, "after the Python layer's refusals")
        assert c.L.nalo_frame_release(c.h_, 1, None) == 0                    # nothing was ever ingested into slot 1: nothing to wait for
    finally:
        c.close()
        torch.cuda.synchronize()
