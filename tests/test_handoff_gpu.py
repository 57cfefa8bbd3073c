"""Frames and the tracking reference handed between contexts on the device: nalo_frame_plane, nalo_trk_ref_export, nalo_trk_ref_import, nalo_trk_ref_release
(handoff_copy_kernel, kernels_handoff.hip) - the threaded layout of the reference, which tracks on the caller's thread and maps on its own
(FullSystem.cpp:1183-1252) with two CoarseTracker objects swapped under a mutex (:1094-1098, :1401-1410).

Every comparison is bit for bit (uint32 words; NaN payloads, infinities and -0.0 are planted where they can travel): a hand-off copies words, so there is no
tolerance to state. The one exception is the threaded run's tracked poses when a tracker lost co-residency to the mapper's kernels and latched the host-driven
LM loop: there the bound is the one tests/test_tracker_gpu.py:219 already uses between the two LM loops (pose_dist < 1e-5, affine < 1e-3)."""
import ctypes as C
import math
import queue
import threading
import time

import numpy as np
import pytest
import torch

import lifecycle_model as lm
import lifecycle_scenes as sc
import orc
from helpers import _hip, pose_dist, tracker_inputs, true_rel_pose
from nalo_slam_amd import binding, synth
from test_device_ingest_gpu import bits, dev, special_image
from test_frontend_edges_gpu import (ERR_ARG, ERR_STATE, GAMMA, HO, WO, assert_pyramids_equal, context, gpu_pyramid, make_image, planted_remap, raw_image, response,
                                     vignette_inv)
from test_trk_ref_window_gpu import assert_same_ref, tracker_ref, window_ctx

pytestmark = pytest.mark.gpu

ERR_HIP = -3
TIMEOUT = 60.0                                                               # of every queue get and join below: reached only when the other side has failed


def as_numpy(view):
    """a DeviceView through torch: the zero-copy tensor's words on the host"""
    t = torch.as_tensor(view, device="cuda")
    assert t.data_ptr() == view.ptr, "torch.as_tensor copied"
    return t.cpu().numpy()


def special_mask(w, h, seed):
    rng = np.random.RandomState(seed)
    m = (rng.rand(h, w) * 255).astype(np.float32)
    b = m.view(np.uint32)
    m[0, 0], m[h - 1, w - 1], m[h // 2, w // 2] = -0.0, np.inf, -np.inf
    b[0, w - 1], b[h - 1, 0], b[h // 2, 1] = 0x7FC54321, 0xFFC00007, 0x00000001
    return m


def track_bits(r):
    """a trk_track result as words: ok, pose, affine, residuals (NaN on unused levels), flow, evaluations"""
    return (r[0], np.asarray(r[1]).tobytes(), np.asarray(r[2]).tobytes(), np.asarray(r[3]).tobytes(), np.asarray(r[4]).tobytes(), r[5])


# ------------------------------------------------------------------------------------------------ 1. planes
@pytest.mark.parametrize("w,h,levels", [(70, 34, 3), (72, 40, 0)], ids=["70x34", "72x40"])
def test_planes_of_every_kind_of_slot(w, h, levels):
    """slot 0 filled by frame_upload with mask and colour, slot 1 by frame_upload_raw through a remap, slot 2 by frame_ingest from tensors: every plane as a
    zero-copy tensor equals the read-back route; then every refusal, with `out` untouched"""
    rng = np.random.RandomState(w)
    img, mask, bgr = special_image(w, h, seed=4), special_mask(w, h, seed=5), rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    rx, ry, taps = planted_remap(w, h, WO, HO)
    raw = raw_image(np.uint8, WO, HO, taps, seed=6)
    mask_o, bgr_o = rng.randint(0, 256, (HO, WO)).astype(np.uint8), rng.randint(0, 256, (HO, WO, 3)).astype(np.uint8)
    c = context(w, h, levels, n_slots=5)
    try:
        c.undist_set(WO, HO, response(256), vignette_inv(WO, HO), 2, rx, ry)
        c.frame_upload(0, img, mask=mask, bgr=bgr, gammaB=GAMMA)
        c.frame_upload_raw(1, raw, exposure=0.02, mask_org=mask_o, bgr_org=bgr_o)
        c.frame_ingest(2, image=dev(img), mask=dev(mask), colour=dev(bgr))
        c.frame_upload(3, img)                                               # a tracked frame: neither mask nor colour
        c.sync()
        for slot in (0, 1, 2):
            views = {k: c.frame_plane(slot, k) for k in ("irradiance", "mask", "colour")}
            for v in views.values():
                assert v.stream == c.stream and v.owner is c
            c.dev_plane_check(binding.dev_plane(views["irradiance"]))
            c.dev_plane_check(binding.dev_plane(views["mask"]))
            c.dev_plane_check(binding.dev_plane(views["colour"], "hwc"))
            want_m, want_b = c.frame_download_mask(slot)
            want_I = c.frame_download(slot, 0)[0][:, 0]
            got_I, got_m, got_b = as_numpy(views["irradiance"]), as_numpy(views["mask"]), as_numpy(views["colour"])
            assert got_I.shape == (h, w) and got_I.dtype == np.float32 and np.array_equal(bits(got_I), bits(want_I)), slot
            assert got_m.shape == (h, w) and got_m.dtype == np.float32 and np.array_equal(bits(got_m), bits(want_m)), slot
            assert got_b.shape == (h, w, 3) and got_b.dtype == np.uint8 and np.array_equal(got_b, want_b), slot
            assert c.frame_plane(slot, binding.PLANE_MASK).ptr == views["mask"].ptr
        assert np.array_equal(bits(as_numpy(c.frame_plane(0, "irradiance"))), bits(img)) and np.array_equal(bits(as_numpy(c.frame_plane(2, "mask"))), bits(mask))
        assert {0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000} <= set(bits(as_numpy(c.frame_plane(2, "irradiance"))).tolist())
        # refusals
        sentinel = binding.DevPlane(0x1234, 7, -1, -2, 9, 11, 12, 13)
        raw_bytes = bytes(sentinel)
        refused = [(-1, 0, ERR_ARG), (5, 0, ERR_ARG), (0, 3, ERR_ARG), (0, -1, ERR_ARG), (4, 0, ERR_STATE), (4, 1, ERR_STATE), (4, 2, ERR_STATE), (3, 1, ERR_STATE), (3, 2, ERR_STATE)]
        for slot, which, code in refused:
            assert c.L.nalo_frame_plane(c.h_, slot, which, C.byref(sentinel)) == code, (slot, which)
            assert bytes(sentinel) == raw_bytes, (slot, which)
            if 0 <= which <= 2:                                              # exactly where nalo_frame_download_mask refuses the same plane (the mask stands in for the image)
                m = np.zeros((h, w), np.float32) if which != 2 else None
                b = np.zeros((h, w, 3), np.uint8) if which == 2 else None
                assert c.L.nalo_frame_download_mask(c.h_, slot, binding._f(m), binding._u8(b)) == code, (slot, which)
        assert c.L.nalo_frame_plane(c.h_, 0, 0, None) == ERR_ARG
        assert c.L.nalo_frame_plane(None, 0, 0, C.byref(sentinel)) == ERR_ARG and bytes(sentinel) == raw_bytes
        with pytest.raises(binding.NaloError, match="error %d" % ERR_STATE):
            c.frame_plane(3, "mask")
        assert c.frame_plane(3, "irradiance").shape == (h, w)                # the plane a tracked frame does have
    finally:
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. frame hand-off
@pytest.mark.parametrize("gamma", [False, True], ids=["plain", "gammaB"])
def test_frame_hand_off_is_bit_identical(gamma):
    """tracker context -> mapper context through planes and frame_ingest: every level's {I, dx, dy} and absSquaredGrad, mask and colour"""
    B = GAMMA if gamma else None
    for w, h, levels in ((72, 40, 4), (70, 34, 3)):
        rng = np.random.RandomState(h)
        img, mask, bgr = special_image(w, h, seed=8), special_mask(w, h, seed=9), rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        T, M = context(w, h, levels, n_slots=2), context(w, h, levels, n_slots=2)
        try:
            T.frame_upload(1, img, mask=mask, bgr=bgr, gammaB=B)
            M.frame_ingest(0, image=T.frame_plane(1, "irradiance"), mask=T.frame_plane(1, "mask"), colour=T.frame_plane(1, "colour"), gammaB=B)   # release=True: the back edge
            got, want = gpu_pyramid(M, 0), gpu_pyramid(T, 1)
            assert_pyramids_equal(got, want, (w, h, gamma))
            for (g_dI, g_ab), (t_dI, t_ab) in zip(got, want):
                assert np.array_equal(bits(g_dI), bits(t_dI)) and np.array_equal(bits(g_ab), bits(t_ab))      # NaN payloads included
            (gm, gb), (tm, tb) = M.frame_download_mask(0), T.frame_download_mask(1)
            assert np.array_equal(bits(gm), bits(tm)) and np.array_equal(gb, tb)
            T.frame_upload(1, make_image(w, h, seed=1))                       # the tracker reuses its slot: the mapper's copy stays
            assert_pyramids_equal(gpu_pyramid(M, 0), want, (w, h, gamma, "after the source was overwritten"))
        finally:
            T.close(); M.close()
            torch.cuda.synchronize()


@pytest.mark.parametrize("gamma", [False, True], ids=["plain", "gammaB"])
def test_consumers_see_the_same_frame_on_both_sides(small_window, gamma):
    """one consumer on each side: pixsel_make_maps of the handed frame, and trk_track of it against a common reference"""
    win, B = small_window, (GAMMA if gamma else None)
    rng = np.random.RandomState(3)
    rp = rng.randint(0, 256, win.w * win.h).astype(np.uint8)
    mask, bgr = (rng.rand(win.h, win.w) * 4).astype(np.int32).astype(np.float32), rng.randint(0, 256, (win.h, win.w, 3)).astype(np.uint8)
    Ku, Kv, nid, hdi = tracker_inputs(win)
    T0 = orc.se3_exp(orc.se3_log(true_rel_pose(win, win.W - 1, win.W)) * 0.9)
    T, M = [binding.Context(win.w, win.h, win.K, n_slots=2) for _ in range(2)]
    try:
        for c in (T, M):
            c.pixsel_set_random(rp)
            c.frame_upload(0, win.images[win.W - 1], gammaB=B)
            c.trk_set_ref(0, Ku, Kv, nid, hdi)
        T.frame_upload(1, win.images[win.W], mask=mask, bgr=bgr, gammaB=B)
        M.frame_ingest(1, image=T.frame_plane(1, "irradiance"), mask=T.frame_plane(1, "mask"), colour=T.frame_plane(1, "colour"), gammaB=B)
        mt, mm = T.pixsel_make_maps(1, 1500.0, 3), M.pixsel_make_maps(1, 1500.0, 3)
        assert mt[1] == mm[1] > 0 and mt[2] == mm[2] and np.array_equal(bits(mt[0]), bits(mm[0]))
        rt, rm = T.trk_track(1, T0, [0, 0], [0, 0], [1, 1], win.levels - 1), M.trk_track(1, T0, [0, 0], [0, 0], [1, 1], win.levels - 1)
        assert rt[0] == 1 and track_bits(rt) == track_bits(rm)
        assert T.trk_launch_config()["driver"] == M.trk_launch_config()["driver"] == 1
    finally:
        T.close(); M.close()


# ------------------------------------------------------------------------------------------------ 3. stream order
def test_stream_order_across_two_contexts():
    """built like test_device_ingest_gpu.py::test_stream_order_without_a_host_wait, one context further: the source ingests a tensor that holds the wrong data
    until a chain of matmuls of at least 0.2 s on a torch stream has run, the destination ingests from the source's planes while the chain runs. That call
    returns before the chain has ended, its pyramid is the right data's, and after frame_release(dst, slot, src.stream) the source slot is overwritten at once"""
    w, h, levels = 72, 40, 4
    right, wrong, junk = make_image(w, h, seed=11), make_image(w, h, seed=12), make_image(w, h, seed=13)
    S, D = context(w, h, levels, n_slots=2), context(w, h, levels, n_slots=2)
    try:
        D.frame_upload(1, right)
        want = gpu_pyramid(D, 1)
        t_right, t_wrong, t_junk = dev(right), dev(wrong), dev(junk)
        t = torch.empty_like(t_right)
        S.frame_ingest(0, image=t_wrong)                                     # steady state on both sides: buffers and events exist, and both slots hold the wrong data
        D.frame_ingest(0, image=S.frame_plane(0, "irradiance"))
        S.sync(); D.sync()
        assert_pyramids_equal(gpu_pyramid(D, 0), gpu_pyramid(S, 0), "warm-up")
        torch.cuda.synchronize()
        a = torch.randn(4096, 4096, device="cuda")
        out = torch.empty_like(a)
        TS = torch.cuda.Stream()
        with torch.cuda.stream(TS):
            torch.mm(a, a, out=out)
            TS.synchronize()
            t0 = time.perf_counter()
            torch.mm(a, a, out=out)
            TS.synchronize()
            one = max(time.perf_counter() - t0, 1e-5)
            reps = min(int(math.ceil(0.25 / one)) + 1, 20000)                # 0.2 s and a quarter more
            t.copy_(t_wrong)
            for _ in range(reps):
                torch.mm(a, a, out=out)
            t.copy_(t_right)
            behind = torch.cuda.Event()
            behind.record(TS)
            S.frame_ingest(0, image=t, release=False)                        # the source's main stream now waits for the chain
            plane = S.frame_plane(0, "irradiance")                           # a view of what that stream WILL have produced
            D.frame_ingest(0, image=plane, release=False)                    # stream = plane.stream = S.stream
            returned_early = not behind.query()
            D.frame_release(0, S.stream)                                     # the back edge ...
            S.frame_ingest(0, image=t_junk, stream=torch.cuda.default_stream().cuda_stream)   # ... and the source slot is overwritten at once
            assert returned_early, "the hand-off waited for the producer (%d matmuls of %.2e s)" % (reps, one)
            assert_pyramids_equal(gpu_pyramid(D, 0), want, "the destination holds the right data")
            assert np.array_equal(bits(gpu_pyramid(S, 0)[0][0][:, 0]), bits(junk))
            TS.synchronize()
    finally:
        S.close(); D.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. the imported reference equals its source
def test_import_equals_its_source(small_window):
    """640x480: trk_set_ref in A, export, import in B; then the same after trk_set_ref_from_window on a small optimised window. A's intrinsics are moved off
    nalo_create's by nalo_trk_make_k first, so the clone only tracks alike when the import takes them over"""
    win = small_window
    Ku, Kv, nid, hdi = tracker_inputs(win)
    T0 = orc.se3_exp(orc.se3_log(true_rel_pose(win, win.W - 1, win.W)) * 0.9)
    order = np.random.RandomState(5).permutation(len(win.host))
    A = window_ctx(win, order, synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003), n_slots=win.W + 1)
    B = binding.Context(win.w, win.h, win.K, n_slots=3)
    try:
        A.frame_upload(win.W, win.images[win.W])
        B.frame_upload(2, win.images[win.W - 1]); B.frame_upload(1, win.images[win.W])
        with pytest.raises(binding.NaloError, match="error %d" % ERR_STATE):
            B.trk_ref_export()                                               # no reference yet
        assert A.L.nalo_trk_make_k(A.h_, win.K[0] * 1.001, win.K[1] * 0.999, win.K[2] + 0.25, win.K[3] - 0.25) == 0
        A.trk_set_ref(win.W - 1, Ku, Kv, nid, hdi)
        e = A.trk_ref_export()
        assert e["slot_ref"] == win.W - 1 and e["stream"] == A.stream and all(n > 0 for n in e["n"]) and len(e["levels"]) == win.levels
        assert not np.array_equal(e["intrinsics"], binding.pyr_intrinsics(win.K, win.levels))
        B.trk_ref_import(2, e)
        B.trk_ref_release(A.stream)
        assert B.trk_ref_export()["slot_ref"] == 2
        # the views as torch sees them: zero-copy, the read-backs' words
        A.sync()
        for l in (0, win.levels - 1):
            pc, dm = A.trk_get_pc(l), A.trk_get_depth(l)
            for k, name in enumerate(("u", "v", "idepth", "color")):
                assert np.array_equal(bits(as_numpy(e["levels"][l][name])), bits(pc[k])), (l, name)
            assert np.array_equal(bits(as_numpy(e["levels"][l]["idepth_map"])), bits(dm[0])) and np.array_equal(bits(as_numpy(e["levels"][l]["weight_sums"])), bits(dm[1]))
        # frames: A tracks slot W, B its slot 1 - the same image
        assert_same_ref(tracker_ref(B), tracker_ref(A))
        ra = A.trk_track(win.W, T0, [0, 0], [0, 0], [1, 1], win.levels - 1)
        rb = B.trk_track(1, T0, [0, 0], [0, 0], [1, 1], win.levels - 1)
        assert A.trk_launch_config()["driver"] == 1 and B.trk_launch_config() == A.trk_launch_config()
        assert ra[0] == 1 and track_bits(ra) == track_bits(rb)
        # the reference of an optimised window
        A.ba_optimize(its=3)
        A.trk_set_ref_from_window()
        e2 = A.trk_ref_export()
        assert e2["n"] != e["n"]
        B.trk_ref_import(2, e2["view"])
        B.trk_ref_release(A.stream)
        assert_same_ref(tracker_ref(B), tracker_ref(A))
        assert np.array_equal(bits(B.trk_ref_export()["intrinsics"]), bits(e2["intrinsics"]))
        ra2 = A.trk_track(win.W, T0, [0, 0], [0, 0], [1, 1], win.levels - 1)
        rb2 = B.trk_track(1, T0, [0, 0], [0, 0], [1, 1], win.levels - 1)
        assert A.trk_launch_config()["driver"] == 1 and B.trk_launch_config() == A.trk_launch_config()
        assert ra2[0] == 1 and track_bits(ra2) == track_bits(rb2) and track_bits(ra2) != track_bits(ra)
    finally:
        A.close(); B.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. planted sizes and alignments
PLANTED_N = [595, 0, 1, 3, 4, 5, 255, 256, 257]                              # in this order 595 -> 0 and 257 -> 595 (wrap) are a smaller n behind a larger one


def words(rng, n):
    """n random 32-bit patterns as float32: NaN payloads, infinities, denormals and -0.0 among them"""
    return rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def test_planted_sizes_and_alignments():
    """Context(140, 68, levels=3): levels of 9520, 2380 and 595 words (three chunks with a tail, one chunk, one chunk with a tail). The views are torch
    slices 0, 1, 2 and 3 floats off a 16-byte boundary, so the 16-byte path, the 4-byte path and the word tail all run; maps are present on some levels and NULL
    on others; every imported word is read back"""
    w, h, L = 140, 68, 3
    npx = [(w >> l) * (h >> l) for l in range(L)]
    assert npx == [9520, 2380, 595]
    rng = np.random.RandomState(77)
    c = context(w, h, L, n_slots=1)
    try:
        c.frame_upload(0, make_image(w, h))
        cases = [(off, [PLANTED_N[(i + l) % len(PLANTED_N)] for l in range(L)]) for off in range(4) for i in range(len(PLANTED_N))]
        cases += [(off, [9520, 2380, 595]) for off in range(4)] + [(1, [4097, 4, 257]), (0, [4096, 1, 3])]       # whole levels: a cloud of several chunks
        for ci, (off, ns) in enumerate(cases):
            host, lv = [], []
            for l in range(L):
                hv = dict(zip(("u", "v", "idepth", "color"), (words(rng, ns[l]) for _ in range(4))))
                with_maps = bool((ci >> l) & 1)
                if with_maps:
                    hv["idepth_map"], hv["weight_sums"] = words(rng, npx[l]), words(rng, npx[l])
                dv = {}
                for k, a in hv.items():
                    base = torch.zeros(len(a) + 8, dtype=torch.float32, device="cuda")
                    assert base.data_ptr() % 16 == 0
                    s = base[off:off + len(a)]
                    s.copy_(torch.from_numpy(a))
                    assert s.numel() == len(a) and (len(a) == 0 or s.data_ptr() % 16 == 4 * off)
                    dv[k] = s
                host.append(hv); lv.append(dv)
            torch.cuda.synchronize()
            c.trk_ref_import(0, lv, stream=torch.cuda.current_stream().cuda_stream)
            c.trk_ref_release(torch.cuda.current_stream().cuda_stream)
            del lv
            for l in range(L):
                pc = c.trk_get_pc(l)
                assert len(pc[0]) == ns[l], (ci, l)
                for k, name in enumerate(("u", "v", "idepth", "color")):
                    assert np.array_equal(bits(pc[k]), bits(host[l][name])), (ci, off, ns, l, name)
                dm = c.trk_get_depth(l)
                for k, name in enumerate(("idepth_map", "weight_sums")):
                    want = host[l].get(name, np.zeros(npx[l], np.float32))
                    assert np.array_equal(bits(dm[k]), bits(want)), (ci, off, ns, l, name)
        assert np.array_equal(bits(c.trk_ref_export()["intrinsics"]), bits(binding.pyr_intrinsics(c.K, L)))
    finally:
        c.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. refusals
def clone_view(V):
    out = binding.TrkRefView()
    C.memmove(C.byref(out), C.byref(V), C.sizeof(binding.TrkRefView))
    return out


def test_import_refusals_leave_the_reference(small_window):
    """every refusal of nalo_trk_ref_import, one by one; after each the destination's reference is bit-identical - clouds, maps and a trk_track result - and
    the next legal call still works"""
    win = small_window
    Ku, Kv, nid, hdi = tracker_inputs(win)
    T0 = orc.se3_exp(orc.se3_log(true_rel_pose(win, win.W - 1, win.W)) * 0.9)
    A, B = [binding.Context(win.w, win.h, win.K, n_slots=3) for _ in range(2)]
    try:
        for c in (A, B):
            c.frame_upload(0, win.images[win.W - 1]); c.frame_upload(1, win.images[win.W])
        A.trk_set_ref(0, Ku[:2000], Kv[:2000], nid[:2000], hdi[:2000])
        B.trk_set_ref(0, Ku, Kv, nid, hdi)                                   # B's own reference: what every refusal must leave
        ref0 = tracker_ref(B)
        trk0 = track_bits(B.trk_track(1, T0, [0, 0], [0, 0], [1, 1], win.levels - 1))
        V = A.trk_ref_export()["view"]
        A.sync()
        # an allocation of its own, 4 KB, straight from the runtime: a tensor of a caching allocator sits in a block that may be far larger than the tensor, and the
        # extent test sees the block. That the library refuses these extents is asked of nalo_dev_plane_check first, which launches nothing.
        hip = _hip()
        hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        tail_p = C.c_void_p()
        assert hip.hipMalloc(C.byref(tail_p), 4096) == 0
        tail = tail_p.value
        assert V.n[0] * 4 > 4096
        for n_words in (V.n[0], (win.w >> 1) * (win.h >> 1)):
            d = binding.DevPlane(tail, binding.DT_F32, n_words, 1, 1, 4 * n_words, 4, 0)
            assert B.L.nalo_dev_plane_check(B.h_, C.byref(d)) == ERR_ARG, "the runtime reports more than the 4 KB that were asked for"
        host_arr = np.zeros(win.w * win.h, np.float32)
        pinned = B.pinned_array((win.w * win.h,), np.float32)
        npx1 = (win.w >> 1) * (win.h >> 1)

        def mutated(**kw):
            v = clone_view(V)
            for k, val in kw.items():
                if isinstance(val, tuple):
                    getattr(v, k)[val[0]] = val[1]
                else:
                    setattr(v, k, val)
            return v
        refused = {
            "w differs": (0, mutated(w=win.w + 2), ERR_ARG), "h differs": (0, mutated(h=win.h - 2), ERR_ARG), "levels differ": (0, mutated(levels=win.levels - 1), ERR_ARG),
            "n < 0": (0, mutated(n=(1, -1)), ERR_ARG), "n beyond the level": (0, mutated(n=(1, npx1 + 1)), ERR_ARG),
            "a null cloud pointer with n > 0": (0, mutated(idepth=(0, None)), ERR_ARG),
            "idepth_map without weight_sums": (0, mutated(weight_sums=(2, None)), ERR_ARG), "weight_sums without idepth_map": (0, mutated(idepth_map=(0, None)), ERR_ARG),
            "a cloud in host memory": (0, mutated(u=(0, host_arr.ctypes.data)), ERR_ARG), "a map in pinned host memory": (0, mutated(idepth_map=(0, pinned.ctypes.data)), ERR_ARG),
            "a cloud pointer that is no multiple of 4": (0, mutated(color=(1, V.color[1] + 2)), ERR_ARG),
            "a map pointer that is no multiple of 4": (0, mutated(weight_sums=(1, V.weight_sums[1] + 1)), ERR_ARG),
            "a cloud that leaves its allocation": (0, mutated(v=(0, tail)), ERR_ARG),
            "a map that leaves its allocation": (0, mutated(idepth_map=(1, tail)), ERR_ARG),
            "slot_ref -1": (-1, clone_view(V), ERR_ARG), "slot_ref beyond the slots": (3, clone_view(V), ERR_ARG),
            "slot_ref without a pyramid": (2, clone_view(V), ERR_STATE),
        }
        for name, (slot, v, code) in refused.items():
            assert B.L.nalo_trk_ref_import(B.h_, slot, C.byref(v)) == code, name
            assert_same_ref(tracker_ref(B), ref0)
            assert track_bits(B.trk_track(1, T0, [0, 0], [0, 0], [1, 1], win.levels - 1)) == trk0, name
        assert hip.hipFree(tail_p) == 0                                      # no refused call queued anything that could still read it
        assert B.L.nalo_trk_ref_import(B.h_, 0, None) == ERR_ARG and B.L.nalo_trk_ref_import(None, 0, C.byref(V)) == ERR_ARG
        assert_same_ref(tracker_ref(B), ref0)
        assert B.L.nalo_trk_ref_release(None, None) == ERR_ARG and B.L.nalo_trk_ref_release(B.h_, None) == 0       # nothing imported yet: nothing to wait for
        a = torch.ones(8, device="cuda") * 2                                 # the runtime is as it was: no error left behind
        assert float(a.sum().item()) == 16.0
        # export's own refusals leave `out`
        fresh = binding.Context(win.w, win.h, win.K, n_slots=1)
        sentinel = clone_view(V)
        before = bytes(sentinel)
        assert fresh.L.nalo_trk_ref_export(fresh.h_, C.byref(sentinel)) == ERR_STATE and bytes(sentinel) == before
        assert fresh.L.nalo_trk_ref_export(fresh.h_, None) == ERR_ARG and fresh.L.nalo_trk_ref_export(None, C.byref(sentinel)) == ERR_ARG
        fresh.close()
        # the next legal call works
        B.trk_ref_import(0, V)
        B.trk_ref_release(A.stream)
        assert_same_ref(tracker_ref(B), tracker_ref(A))
        ref1 = tracker_ref(B)
        # a context whose exchange failed: NALO_ERR_HIP as nalo_trk_track, the reference as it was
        B.ba_exchange_failed("test")
        assert B.L.nalo_trk_ref_import(B.h_, 0, C.byref(V)) == ERR_HIP
        assert_same_ref(tracker_ref(B), ref1)
    finally:
        A.close(); B.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. three keyframes, threaded as the reference threads them
KF, PER_KF, RING = 3, 3, 4


class Chain:
    """The device chain on a mapper context and the tracking on a tracker context, joined by three queues. mapper(kf) and tracker(kf) are the two threads'
    bodies; called alternately on one thread they are the twin. Frame i lives in mapper slot i and in tracker slot i % RING: the reference frame and the three
    frames tracked against it are four consecutive frames, so the ring never overwrites a frame that is in use."""

    def __init__(self, win, st6):
        self.win, self.st6, self.W = win, st6, win.W
        self.F = win.images.shape[0]
        self.M = binding.Context(win.w, win.h, win.K, n_slots=self.F)
        self.T = binding.Context(win.w, win.h, win.K, n_slots=RING)
        self.swap = threading.Lock()                                         # coarseTrackerSwapMutex
        self.ref_q, self.frame_q, self.ack_q = queue.Queue(), queue.Queue(), queue.Queue()
        self.acked = set()
        self.out = dict(window=[], ref_m=[], ref_t=[], frames_m={}, frames_t={}, tracks=[], drivers=[])
        M = self.M
        for i in range(self.W):
            M.frame_upload(i, win.images[i])
        M.ba_set_prior_carry(True)
        M.ba_set_window(list(range(self.W)), win.world_to_cam[:self.W], state6=st6[:self.W], frame_ids=[200 + i for i in range(self.W)])
        M.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
        M.ba_set_residuals(win.exists)
        ng0, lt0, ls0 = lm.default_history(win.exists)
        ls0[win.host == self.W - 1, 0] = lm.IN
        M.ba_set_point_history(ng0, lt0, ls0)
        self.T.frame_upload((self.W - 1) % RING, win.images[self.W - 1])     # the first reference frame: the tracker has tracked it before the test begins
        self.m_stream, self.t_stream = M.stream, self.T.stream               # raw handles: all one thread ever uses of the other's context

    def ref_frame(self, kf):
        return self.W - 1 + PER_KF * kf

    def take_frames(self, n):
        """the mapper's end of deliverTrackedFrame: n frames from the queue, each ingested from the tracker's plane into slot i; release=True is the back edge"""
        for _ in range(n):
            i, plane = self.frame_q.get(timeout=TIMEOUT)
            self.M.frame_ingest(i, image=plane)
            self.ack_q.put(i)
            self.out["frames_m"][i] = gpu_pyramid(self.M, i)

    def mapper(self, kf):
        M, win = self.M, self.win
        if kf:
            self.take_frames(PER_KF)
            i = self.ref_frame(kf)
            M.ba_carry_window(M.frame_state(i, win.world_to_cam[i], frame_id=200 + i, state6=self.st6[i]))
        M.ba_optimize(its=3)
        pts, (fr, w2c, cal) = M.ba_get_points(), M.ba_get_frames()
        self.out["window"].append((bytes(fr), w2c.tobytes(), cal.tobytes(), {k: v.tobytes() for k, v in pts.items()}))
        with self.swap:                                                      # makeKeyFrame, FullSystem.cpp:1401-1410
            M.trk_set_ref_from_window()
            view = M.trk_ref_export()["view"]
        assert view.slot_ref == self.ref_frame(kf)
        self.ref_q.put(view)
        self.out["ref_m"].append(tracker_ref(M))
        ff = np.zeros(M.W, np.uint8); ff[0] = 1
        M.ba_flag_points(ff)
        M.ba_marginalize_flagged()
        M.ba_marginalize_frame(0)

    def wait_ack(self, i):
        while i not in self.acked:
            self.acked.add(self.ack_q.get(timeout=TIMEOUT))

    def tracker(self, kf):
        T, win = self.T, self.win
        r = self.ref_frame(kf)
        view = self.ref_q.get(timeout=TIMEOUT)
        with self.swap:                                                      # the swap of FullSystem.cpp:1094-1098
            T.trk_ref_import(r % RING, view)
            T.trk_ref_release(self.m_stream)                                 # the back edge: the mapper's next rebuild waits, on the device, for this import
        self.out["ref_t"].append(tracker_ref(T))
        for j in range(1, PER_KF + 1):
            i = r + j
            if i - RING >= self.W:                                           # the slot held a frame that was handed over: the mapper must have taken it
                self.wait_ack(i - RING)
            T.frame_upload(i % RING, win.images[i])
            T0 = orc.se3_exp(orc.se3_log(true_rel_pose(win, r, i)) * 0.9)
            res = T.trk_track(i % RING, T0, [0, 0], [0, 0], [1, 1], win.levels - 1)
            self.out["tracks"].append(res)
            self.out["drivers"].append(T.trk_launch_config()["driver"])
            self.out["frames_t"][i] = gpu_pyramid(T, i % RING)
            self.frame_q.put((i, T.frame_plane(i % RING, "irradiance")))

    def close(self):
        self.T.close(); self.M.close()


@pytest.fixture(scope="module")
def kitti_chain_scene():
    s = 3e-4
    W = 8
    win = synth.make_window(w=1224, h=368, W=W, P=2000, seed=sc.SEED, n_extra=KF * PER_KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    F = W + KF * PER_KF
    rng = np.random.RandomState(sc.SEED + 3)
    st6 = np.zeros((F, 6))
    st6[1:, :3] = 0.004 * rng.randn(F - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * rng.randn(F - 1, 3)
    return win, st6


def test_three_keyframes_threaded_as_the_reference_threads_them(kitti_chain_scene):
    """1224x368, W = 8: the mapper runs the device chain of tests/test_map_gpu.py::test_three_keyframes_of_the_device_chain and ends each keyframe's
    optimisation with trk_set_ref_from_window and an export under the lock; the tracker, on a second thread, imports at the swap, tracks three frames per
    keyframe, hands each to the mapper through its plane and a queue, and releases on both back edges. A twin runs the same calls on one thread."""
    win, st6 = kitti_chain_scene
    errors = []
    threaded = Chain(win, st6)
    th = None
    try:
        def tracker_thread():
            try:
                for kf in range(KF):
                    threaded.tracker(kf)
            except BaseException as e:                                       # reported by the main thread; the mapper's next queue get times out
                errors.append(e)
        th = threading.Thread(target=tracker_thread, name="tracker")
        th.start()
        for kf in range(KF):
            threaded.mapper(kf)
        threaded.take_frames(PER_KF)                                         # the last three tracked frames
        th.join(TIMEOUT)
        assert not th.is_alive(), "the tracker thread did not finish"
        assert not errors, errors
    finally:
        if th is None or not th.is_alive():                                  # never destroy a context under a thread that may still use it
            threaded.close()
    twin = Chain(win, st6)
    try:
        for kf in range(KF):
            twin.mapper(kf)
            twin.tracker(kf)
        twin.take_frames(PER_KF)
    finally:
        twin.close()
    a, b = threaded.out, twin.out
    assert len(a["window"]) == len(a["ref_m"]) == len(a["ref_t"]) == KF and len(a["tracks"]) == KF * PER_KF
    for kf in range(KF):
        assert all(len(lv[0]) > 0 for lv in a["ref_m"][kf]), kf              # a real reference on every level
        assert_same_ref(a["ref_t"][kf], a["ref_m"][kf])                      # the tracker's imported clouds and maps are the mapper's
        assert_same_ref(b["ref_t"][kf], b["ref_m"][kf])
        assert a["window"][kf] == b["window"][kf], "keyframe %d: the mapper's window after ba_optimize differs from the twin's" % kf
        assert_same_ref(a["ref_m"][kf], b["ref_m"][kf])
    assert sorted(a["frames_m"]) == sorted(a["frames_t"]) == list(range(win.W, win.W + KF * PER_KF))
    for run in (a, b):
        for i in run["frames_m"]:
            for (g_dI, g_ab), (t_dI, t_ab) in zip(run["frames_m"][i], run["frames_t"][i]):
                assert np.array_equal(bits(g_dI), bits(t_dI)) and np.array_equal(bits(g_ab), bits(t_ab)), i
    assert all(d == 1 for d in b["drivers"]), b["drivers"]                  # nothing else runs on the device in the twin
    print("HANDOFF threaded tracker drivers", a["drivers"])
    for k, (ra, rb) in enumerate(zip(a["tracks"], b["tracks"])):
        assert ra[0] == rb[0] == 1, k
        if a["drivers"][k] == 1:
            assert track_bits(ra) == track_bits(rb), k
        else:                                                                # the tracker lost co-residency to the mapper's kernels and latched the host-driven loop
            assert pose_dist(ra[1], rb[1]) < 1e-5 and np.abs(ra[2] - rb[2]).max() < 1e-3, k


# ------------------------------------------------------------------------------------------------ 8. a twin that is never exported from
def test_views_enqueue_nothing(small_window):
    """one context is exported from and has planes taken between every two calls of a keyframe, its twin is never touched that way: equal bits throughout"""
    win = small_window
    order = np.arange(len(win.host))
    st6 = synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003)
    T0 = orc.se3_exp(orc.se3_log(true_rel_pose(win, win.W - 1, win.W)) * 0.9)
    A, B = [window_ctx(win, order, st6, n_slots=win.W + 1) for _ in range(2)]
    try:
        def look(c):
            if c is A:
                for slot in range(win.W):
                    c.frame_plane(slot, "irradiance")
                if c.L.nalo_trk_ref_export(c.h_, C.byref(binding.TrkRefView())) == 0:
                    c.trk_ref_export()
        outs = []
        for c in (A, B):
            o = []
            look(c)
            c.frame_upload(win.W, win.images[win.W]); look(c)
            ng0, lt0, ls0 = lm.default_history(win.exists)
            c.ba_set_point_history(ng0, lt0, ls0); look(c)
            c.ba_optimize(its=3); look(c)
            o.append({k: v.tobytes() for k, v in c.ba_get_points().items()}); look(c)
            c.trk_set_ref_from_window(); look(c)
            o.append([[x.tobytes() for x in lv] for lv in tracker_ref(c)]); look(c)
            o.append(track_bits(c.trk_track(win.W, T0, [0, 0], [0, 0], [1, 1], win.levels - 1))); look(c)
            ff = np.zeros(win.W, np.uint8); ff[0] = 1
            dec, H, cnt = c.ba_flag_points(ff); look(c)
            o.append((dec.tobytes(), H.tobytes(), cnt.tobytes()))
            c.ba_marginalize_flagged(); look(c)
            o.append({k: v.tobytes() for k, v in c.ba_get_points().items()})
            fr, w2c, cal = c.ba_get_frames()
            o.append((bytes(fr), w2c.tobytes(), cal.tobytes()))
            outs.append(o)
        assert outs[0] == outs[1]
    finally:
        A.close(); B.close()
