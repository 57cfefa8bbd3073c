// C-ABI: context, frame pyramids, front-end tracker (host mirror of CoarseTracker, reference
// src/FullSystem/CoarseTracker.{h,cpp}). The LM loop of trackNewestCoarse stays on the host exactly as in the
// reference (8x8 LDL^T, SE3::exp); every calcRes/calcGSSSE pair is one fused kernel launch.
#include "nalo_internal.h"
#include "trk_device.h"
#include "handoff_device.h"
#include <cstdlib>

using namespace nalo;

static int pyr_levels_rule(int w, int h) {           // util/globalCalib.cpp:50-55
    int wl = w, hl = h, lv = 1;
    while (wl % 2 == 0 && hl % 2 == 0 && wl * hl > 5000 && lv < NALO_MAX_LEVELS) { wl /= 2; hl /= 2; lv++; }
    return lv;
}
static void set_pyr_calib(nalo_ctx* c, float fx, float fy, float cx, float cy) {   // globalCalib.cpp:74-104 / CoarseTracker::makeK
    c->fx[0] = fx; c->fy[0] = fy; c->cx[0] = cx; c->cy[0] = cy;
    for (int l = 1; l < c->levels; ++l) {
        c->fx[l] = c->fx[l - 1] * 0.5; c->fy[l] = c->fy[l - 1] * 0.5;
        c->cx[l] = (c->cx[0] + 0.5) / ((int)1 << l) - 0.5; c->cy[l] = (c->cy[0] + 0.5) / ((int)1 << l) - 0.5;
    }
}

extern "C" {

int nalo_create(nalo_ctx** out, int device, int w, int h, int levels, const float K[4], int n_slots) {
    if (!out || !K || w < 16 || h < 16 || n_slots < 1) return NALO_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return NALO_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return NALO_ERR_NO_DEVICE;
    nalo_ctx* c = new nalo_ctx();
    c->device = device; c->w = w; c->h = h;
    c->host_timing = std::getenv("NALO_HOST_TIMING") != nullptr;          // the one environment variable the library reads, here and nowhere else
    c->levels = levels > 0 ? levels : pyr_levels_rule(w, h);
    if (c->levels > NALO_MAX_LEVELS) { delete c; return NALO_ERR_ARG; }
    for (int l = 0; l < c->levels; ++l) { c->wl[l] = w >> l; c->hl[l] = h >> l; }
    for (int i = 0; i < 4; ++i) c->K0[i] = K[i];
    set_pyr_calib(c, K[0], K[1], K[2], K[3]);
    if (c->stream.create() != hipSuccess || c->side.create() != hipSuccess) { delete c; return NALO_ERR_HIP; }   // the context owns whatever it got so far
    c->slots.resize(n_slots);
    for (auto& s : c->slots)
        for (int l = 0; l < c->levels; ++l) {
            const size_t npx = (size_t)c->wl[l] * c->hl[l];
            if (s.I[l].reserve(npx) != hipSuccess || s.dI[l].reserve(npx) != hipSuccess || s.absg[l].reserve(npx) != hipSuccess) { nalo_destroy(c); return NALO_ERR_HIP; }
        }
    if (c->trk_out_host.reserve(128, hipHostMallocMapped) != hipSuccess) { nalo_destroy(c); return NALO_ERR_HIP; }
    *out = c;
    return NALO_OK;
}

void nalo_destroy(nalo_ctx* c) {
    if (!c) return;
    if (c->host_timing) for (auto& kv : c->host_t) fprintf(stderr, "[nalo host] %-28s calls=%6ld total=%10.1f us  avg=%8.2f us\n", kv.first.c_str(), kv.second.second, kv.second.first, kv.second.first / std::max(1L, kv.second.second));
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    rccl_release(c);
    ba_destroy(c);
    pixsel_destroy(c);
    init_destroy(c);
    map_destroy(c);
    map_dense_destroy(c);
    tsdf_destroy(c);
    tsdf_archive_destroy(c);
    if (c->copy) (void)hipStreamSynchronize(c->copy);
    // the profiling events are raw handles (they move between the pool and the pending pairs): this is where they end
    for (auto& kv : c->prof) for (auto& ev : kv.second.pending) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (hipEvent_t e : c->prof_pool) (void)hipEventDestroy(e);
    delete c;
}

// The reference constants this library was compiled with (ref_constants.h: the table the constexpr values of host and device code are generated from),
// the pattern offsets and the defaults of nalo_settings. Needs no device.
int nalo_constants(int cap, const char** names, double* values) {
    static const struct { const char* name; double value; } table[] = {
#define NALO_REF_ROW(type, name, refname, value) {refname, (double)(nalo::name)},
        NALO_REF_CONSTANTS(NALO_REF_ROW)
#undef NALO_REF_ROW
        {"patternP[0].x", (double)nalo::kPatternDx[0]}, {"patternP[0].y", (double)nalo::kPatternDy[0]}, {"patternP[1].x", (double)nalo::kPatternDx[1]}, {"patternP[1].y", (double)nalo::kPatternDy[1]},
        {"patternP[2].x", (double)nalo::kPatternDx[2]}, {"patternP[2].y", (double)nalo::kPatternDy[2]}, {"patternP[3].x", (double)nalo::kPatternDx[3]}, {"patternP[3].y", (double)nalo::kPatternDy[3]},
        {"patternP[4].x", (double)nalo::kPatternDx[4]}, {"patternP[4].y", (double)nalo::kPatternDy[4]}, {"patternP[5].x", (double)nalo::kPatternDx[5]}, {"patternP[5].y", (double)nalo::kPatternDy[5]},
        {"patternP[6].x", (double)nalo::kPatternDx[6]}, {"patternP[6].y", (double)nalo::kPatternDy[6]}, {"patternP[7].x", (double)nalo::kPatternDx[7]}, {"patternP[7].y", (double)nalo::kPatternDy[7]},
    };
    const int n = (int)(sizeof(table) / sizeof(table[0]));
    for (int i = 0; i < n && i < cap; ++i) { if (names) names[i] = table[i].name; if (values) values[i] = table[i].value; }
    return n;
}

// the same table as DEVICE code evaluates it: one lane writes every constant (+ the pattern the kernels index) from inside a kernel
__global__ void nalo_constants_kernel(double* out) {
    int i = 0;
#define NALO_REF_ROW(type, name, refname, value) out[i++] = (double)(nalo::name);
    NALO_REF_CONSTANTS(NALO_REF_ROW)
#undef NALO_REF_ROW
    constexpr int dx[8] = NALO_PATTERN_DX, dy[8] = NALO_PATTERN_DY;
    for (int k = 0; k < 8; ++k) { out[i++] = (double)dx[k]; out[i++] = (double)dy[k]; }
}
int nalo_constants_device(nalo_ctx* c, int cap, double* values) {
    if (!c || !values) return fail(c, NALO_ERR_ARG, "nalo_constants_device: bad argument");
    const int n = nalo_constants(0, nullptr, nullptr);
    NALO_HIP(c, hipSetDevice(c->device));
    DevBuf<double> d;
    NALO_HIP(c, d.reserve(n));
    nalo_constants_kernel<<<1, 1, 0, c->stream>>>(d.p);
    std::vector<double> h(n);
    NALO_HIP(c, hipMemcpyAsync(h.data(), d.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n && i < cap; ++i) values[i] = h[i];
    return n;
}

int nalo_test_inject(nalo_ctx* c, int what, int count) {
    if (!c || count < 0) return NALO_ERR_ARG;
    if (what == NALO_INJECT_LM_LOST_BLOCK) c->inject_lm_lost_block = count;
    else if (what == NALO_INJECT_GATED_SOLVE) c->inject_gated_solve = count;
    else return NALO_ERR_ARG;
    return NALO_OK;
}

const char* nalo_last_error(nalo_ctx* c) { return c ? c->err.c_str() : "null ctx"; }
int nalo_levels(nalo_ctx* c) { return c ? c->levels : NALO_ERR_ARG; }
int nalo_sync(nalo_ctx* c) { if (!c) return NALO_ERR_ARG; if (c->copy) NALO_HIP(c, hipStreamSynchronize(c->copy)); NALO_HIP(c, hipStreamSynchronize(c->stream)); NALO_HIP(c, hipStreamSynchronize(c->side)); return NALO_OK; }
void* nalo_stream(nalo_ctx* c) { return c ? (void*)c->stream : nullptr; }
void* nalo_side_stream(nalo_ctx* c) { return c ? (void*)c->side : nullptr; }

int nalo_frame_upload(nalo_ctx* c, int slot, const float* irradiance, const float* mask, const uint8_t* bgr, const float* gammaB) {
    if (!c || !irradiance || slot < 0 || slot >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_frame_upload: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    FrameSlot& s = c->slots[slot];
    const size_t n0 = (size_t)c->w * c->h;
    NALO_HIP(c, hipMemcpyAsync(s.I[0].p, irradiance, n0 * 4, hipMemcpyHostToDevice, c->stream));
    if (mask) { NALO_HIP(c, s.mask.reserve(n0)); NALO_HIP(c, hipMemcpyAsync(s.mask.p, mask, n0 * 4, hipMemcpyHostToDevice, c->stream)); }
    if (bgr) { NALO_HIP(c, s.bgr.reserve(n0 * 3)); NALO_HIP(c, hipMemcpyAsync(s.bgr.p, bgr, n0 * 3, hipMemcpyHostToDevice, c->stream)); }
    const float* gdev = nullptr;
    if (gammaB) { NALO_HIP(c, c->upload_tmp.reserve(256)); NALO_HIP(c, hipMemcpyAsync(c->upload_tmp.p, gammaB, 256 * 4, hipMemcpyHostToDevice, c->stream)); gdev = c->upload_tmp.p; }
    int rc = pyramid_build(c, s, gdev);
    if (rc) return rc;
    pixsel_invalidate_hists(c, slot);
    NALO_HIP(c, hipStreamSynchronize(c->stream));      // host buffers are caller-owned: safe to reuse on return
    s.valid = true;
    return NALO_OK;
}

// Asynchronous form of nalo_frame_upload for a per-frame pipeline (FullSystem::addActiveFrame -> makeImages, FullSystem.cpp:1053-1065): the H2D copies run
// on the context's copy stream, under whatever the main stream is executing (the previous frame's tracking), the pyramid kernels are queued on the main
// stream behind an event. Returns at once: the host buffers must stay untouched until nalo_frame_wait(ctx, slot) (or nalo_sync) returns. Truly
// asynchronous only from pinned host memory (nalo_host_alloc / hipHostMalloc); pageable buffers work but are staged by the HIP runtime.
// The gamma table is shared by all slots of the context: another slot's pyramid kernel (main stream) may still be reading it when the next frame arrives. A running
// system passes the same CalibHessian::B every frame, so the table is sent once; a DIFFERENT table is copied only after the copy stream has waited for everything
// queued on the main stream so far.
static int gamma_upload_async(nalo_ctx* c, const float* gammaB, bool* sent = nullptr) {   // *sent: a copy was queued on the copy stream
    if (sent) *sent = false;
    if (!gammaB) return NALO_OK;
    if (c->gamma_have && std::memcmp(c->gamma_last, gammaB, sizeof(c->gamma_last)) == 0) return NALO_OK;
    NALO_HIP(c, hipEventRecord(c->ev_main, c->stream));
    NALO_HIP(c, hipStreamWaitEvent(c->copy, c->ev_main, 0));
    std::memcpy(c->gamma_last, gammaB, sizeof(c->gamma_last));
    NALO_HIP(c, hipMemcpyAsync(c->gamma_dev.p, c->gamma_last, 256 * 4, hipMemcpyHostToDevice, c->copy));   // from the context's copy: the caller's table may change after the call
    c->gamma_have = true;
    if (sent) *sent = true;
    return NALO_OK;
}
int nalo_frame_upload_async(nalo_ctx* c, int slot, const float* irradiance, const float* mask, const uint8_t* bgr, const float* gammaB) {
    if (!c || !irradiance || slot < 0 || slot >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_frame_upload_async: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    FrameSlot& s = c->slots[slot];
    NALO_HIP(c, c->copy.create()); NALO_HIP(c, c->ev_main.create(hipEventDisableTiming));
    NALO_HIP(c, s.ev_up.create(hipEventDisableTiming));
    const size_t n0 = (size_t)c->w * c->h;
    if (mask) NALO_HIP(c, s.mask.reserve(n0));
    if (bgr) NALO_HIP(c, s.bgr.reserve(n0 * 3));
    if (gammaB) NALO_HIP(c, c->gamma_dev.reserve(256));
    if (s.valid) {                                                   // kernels already queued on the main stream may still read this slot
        NALO_HIP(c, hipEventRecord(c->ev_main, c->stream));
        NALO_HIP(c, hipStreamWaitEvent(c->copy, c->ev_main, 0));
    }
    NALO_HIP(c, hipMemcpyAsync(s.I[0].p, irradiance, n0 * 4, hipMemcpyHostToDevice, c->copy));
    if (mask) NALO_HIP(c, hipMemcpyAsync(s.mask.p, mask, n0 * 4, hipMemcpyHostToDevice, c->copy));
    if (bgr) NALO_HIP(c, hipMemcpyAsync(s.bgr.p, bgr, n0 * 3, hipMemcpyHostToDevice, c->copy));
    { int rg = gamma_upload_async(c, gammaB); if (rg) return rg; }
    NALO_HIP(c, hipEventRecord(s.ev_up, c->copy));
    NALO_HIP(c, hipStreamWaitEvent(c->stream, s.ev_up, 0));
    int rc = pyramid_build(c, s, gammaB ? c->gamma_dev.p : nullptr);
    if (rc) return rc;
    pixsel_invalidate_hists(c, slot);
    s.valid = true;
    return NALO_OK;
}
// Undistort / PhotometricUndistorter tables (util/Undistort.cpp:49-190 builds G and vignetteMapInv, :637-1018 remapX / remapY): device resident after this call
int nalo_undist_set(nalo_ctx* c, int wOrg, int hOrg, const float* G, int GDepth, const float* vignetteMapInv, int photometricCalibration, const float* remapX, const float* remapY) {
    if (!c || wOrg <= 1 || hOrg <= 1 || photometricCalibration < 0 || photometricCalibration > 2 || (!remapX) != (!remapY)) return fail(c, NALO_ERR_ARG, "nalo_undist_set: bad argument");
    if (photometricCalibration > 0 && (!G || GDepth < 256)) return fail(c, NALO_ERR_ARG, "nalo_undist_set: the response G needs >= 256 entries (Undistort.cpp:83-87)");
    if (photometricCalibration == 2 && !vignetteMapInv) return fail(c, NALO_ERR_ARG, "nalo_undist_set: photometricCalibration 2 needs the vignette");
    if (!remapX && (wOrg != c->w || hOrg != c->h)) return fail(c, NALO_ERR_ARG, "nalo_undist_set: passthrough needs wOrg x hOrg = w x h");
    const size_t no = (size_t)wOrg * hOrg, n = (size_t)c->w * c->h;
    // the whole table is checked before anything is copied or reserved: a refused call leaves the context as it was (the old response with the old remap).
    // The four taps of every output pixel must lie inside the original image (the reference's makeOptimalK_crop / the remap construction guarantee it:
    // out-of-image entries are -1, Undistort.cpp:998-1010); a violated table is an out-of-bounds device read. The test is made in floating point: (int) of a
    // NaN, an infinity or a value >= 2^31 is not a number to compare with, and x < wOrg - 1 accepts exactly the finite entries (int)x + 1 < wOrg accepts.
    if (remapX) {
        const double xmax = wOrg - 1, ymax = hOrg - 1;                  // exact for any int; a float converts to double exactly
        for (size_t i = 0; i < n; ++i) if (!(remapX[i] < 0) && !(remapX[i] >= 0 && remapY[i] >= 0 && remapX[i] < xmax && remapY[i] < ymax))
            return fail(c, NALO_ERR_ARG, "nalo_undist_set: remap entry outside the original image");
    }
    NALO_HIP(c, hipSetDevice(c->device));
    if (G) { NALO_HIP(c, c->und_G.reserve(GDepth)); NALO_HIP(c, hipMemcpy(c->und_G.p, G, (size_t)GDepth * 4, hipMemcpyHostToDevice)); }
    if (vignetteMapInv) { NALO_HIP(c, c->und_vinv.reserve(no)); NALO_HIP(c, hipMemcpy(c->und_vinv.p, vignetteMapInv, no * 4, hipMemcpyHostToDevice)); }
    if (remapX) {
        std::vector<float> xy(2 * n);
        for (size_t i = 0; i < n; ++i) { xy[2 * i] = remapX[i]; xy[2 * i + 1] = remapY[i]; }
        NALO_HIP(c, c->und_rxy.reserve(2 * n));
        NALO_HIP(c, hipMemcpy(c->und_rxy.p, xy.data(), 2 * n * 4, hipMemcpyHostToDevice));
    }
    c->und_wOrg = wOrg; c->und_hOrg = hOrg; c->und_photometric = photometricCalibration; c->und_GDepth = GDepth; c->und_remap = remapX != nullptr; c->und_vig = vignetteMapInv != nullptr;
    c->und_set = true;
    return NALO_OK;
}

int nalo_frame_upload_raw(nalo_ctx* c, int slot, const void* raw, int bytes_per_px, float exposure_time, float factor, const uint8_t* mask_org, const uint8_t* bgr_org,
                          const float* gammaB) {
    if (!c || !raw || slot < 0 || slot >= (int)c->slots.size() || (bytes_per_px != 1 && bytes_per_px != 2)) return fail(c, NALO_ERR_ARG, "nalo_frame_upload_raw: bad argument");
    if (!c->und_set) return fail(c, NALO_ERR_STATE, "nalo_frame_upload_raw: nalo_undist_set has not run");
    NALO_HIP(c, hipSetDevice(c->device));
    FrameSlot& s = c->slots[slot];
    const size_t no = (size_t)c->und_wOrg * c->und_hOrg, n0 = (size_t)c->w * c->h;
    // processFrame: `if(!valid || exposure_time <= 0 || setting_photometricCalibration==0)` -> data = factor * image_in (:224-231)
    int photometric = c->und_photometric;
    if (exposure_time <= 0) photometric = 0;
    if (photometric > 0 && bytes_per_px == 2 && c->und_GDepth < 65536) return fail(c, NALO_ERR_ARG, "nalo_frame_upload_raw: 16-bit frames index G beyond its depth");
    NALO_HIP(c, c->und_raw.reserve(no * 2));
    NALO_HIP(c, hipMemcpyAsync(c->und_raw.p, raw, no * bytes_per_px, hipMemcpyHostToDevice, c->stream));
    if (mask_org) { NALO_HIP(c, c->und_mask.reserve(no)); NALO_HIP(c, hipMemcpyAsync(c->und_mask.p, mask_org, no, hipMemcpyHostToDevice, c->stream)); NALO_HIP(c, s.mask.reserve(n0)); }
    if (bgr_org) { NALO_HIP(c, c->und_bgr.reserve(no * 3)); NALO_HIP(c, hipMemcpyAsync(c->und_bgr.p, bgr_org, no * 3, hipMemcpyHostToDevice, c->stream)); NALO_HIP(c, s.bgr.reserve(n0 * 3)); }
    const float* gdev = nullptr;
    if (gammaB) { NALO_HIP(c, c->upload_tmp.reserve(256)); NALO_HIP(c, hipMemcpyAsync(c->upload_tmp.p, gammaB, 256 * 4, hipMemcpyHostToDevice, c->stream)); gdev = c->upload_tmp.p; }
    int rc = ingest_launch(c, c->stream, c->und_raw.p, bytes_per_px, c->und_wOrg, c->und_hOrg, c->und_G.p, c->und_vig ? c->und_vinv.p : nullptr, c->und_remap ? reinterpret_cast<const float2*>(c->und_rxy.p) : nullptr,
                           photometric, factor, mask_org ? c->und_mask.p : nullptr, bgr_org ? c->und_bgr.p : nullptr, s.I[0].p, s.mask.p, s.bgr.p);
    if (rc) return rc;
    rc = pyramid_build(c, s, gdev);
    if (rc) return rc;
    pixsel_invalidate_hists(c, slot);
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    s.valid = true;
    return NALO_OK;
}

// The per-frame entry of a running pipeline for SENSOR frames: the 1-2 B/px raw image is copied on the copy stream (under the tracking of the previous frame),
// the ingest + pyramid kernels are queued on the main stream behind the copy's event. raw must stay untouched until nalo_frame_wait (pinned memory for a truly
// asynchronous copy). Mask / colour are not taken here (keyframe-only inputs: use nalo_frame_upload_raw for those frames).
int nalo_frame_upload_raw_async(nalo_ctx* c, int slot, const void* raw, int bytes_per_px, float exposure_time, float factor, const float* gammaB) {
    if (!c || !raw || slot < 0 || slot >= (int)c->slots.size() || (bytes_per_px != 1 && bytes_per_px != 2)) return fail(c, NALO_ERR_ARG, "nalo_frame_upload_raw_async: bad argument");
    if (!c->und_set) return fail(c, NALO_ERR_STATE, "nalo_frame_upload_raw_async: nalo_undist_set has not run");
    NALO_HIP(c, hipSetDevice(c->device));
    FrameSlot& s = c->slots[slot];
    const size_t no = (size_t)c->und_wOrg * c->und_hOrg;
    int photometric = c->und_photometric;
    if (exposure_time <= 0) photometric = 0;
    if (photometric > 0 && bytes_per_px == 2 && c->und_GDepth < 65536) return fail(c, NALO_ERR_ARG, "nalo_frame_upload_raw_async: 16-bit frames index G beyond its depth");
    NALO_HIP(c, c->copy.create()); NALO_HIP(c, c->ev_main.create(hipEventDisableTiming));
    NALO_HIP(c, s.ev_up.create(hipEventDisableTiming));
    if (s.raw.cap < no * 2) { if (s.raw.p) NALO_HIP(c, hipStreamSynchronize(c->stream)); NALO_HIP(c, s.raw.reserve(no * 2)); }   // the ingest kernel of an earlier frame may still read the old block
    if (gammaB) NALO_HIP(c, c->gamma_dev.reserve(256));
    if (s.valid) {                                                   // kernels already queued on the main stream may still read this slot (incl. its raw buffer)
        NALO_HIP(c, hipEventRecord(c->ev_main, c->stream));
        NALO_HIP(c, hipStreamWaitEvent(c->copy, c->ev_main, 0));
    }
    NALO_HIP(c, hipMemcpyAsync(s.raw.p, raw, no * bytes_per_px, hipMemcpyHostToDevice, c->copy));
    { int rg = gamma_upload_async(c, gammaB); if (rg) return rg; }
    NALO_HIP(c, hipEventRecord(s.ev_up, c->copy));
    NALO_HIP(c, hipStreamWaitEvent(c->stream, s.ev_up, 0));
    int rc = ingest_launch(c, c->stream, s.raw.p, bytes_per_px, c->und_wOrg, c->und_hOrg, c->und_G.p, c->und_vig ? c->und_vinv.p : nullptr, c->und_remap ? reinterpret_cast<const float2*>(c->und_rxy.p) : nullptr,
                           photometric, factor, nullptr, nullptr, s.I[0].p, nullptr, nullptr);
    if (rc) return rc;
    rc = pyramid_build(c, s, gammaB ? c->gamma_dev.p : nullptr);
    if (rc) return rc;
    pixsel_invalidate_hists(c, slot);
    s.valid = true;
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ frames that already live on the device
static size_t dev_plane_elem(int dtype) { return dtype == NALO_DT_U8 ? 1 : dtype == NALO_DT_U16 ? 2 : (dtype == NALO_DT_I32 || dtype == NALO_DT_F32) ? 4 : 0; }
// The one validation of a descriptor (nalo_dev_plane_check, and nalo_frame_ingest_device on every plane before it enqueues or reserves anything). Launches nothing;
// a failed runtime query leaves no sticky error behind.
static int dev_plane_validate(nalo_ctx* c, const nalo_dev_plane* d, const char* who, const char* what) {
    const std::string W = std::string(who) + ": " + what + ": ";
    if (!d || !d->ptr) return fail(c, NALO_ERR_ARG, W + "null pointer");
    const size_t el = dev_plane_elem(d->dtype);
    if (!el) return fail(c, NALO_ERR_ARG, W + "dtype outside NALO_DT_*");
    if (d->channels != 1 && d->channels != 3) return fail(c, NALO_ERR_ARG, W + "channels must be 1 or 3");
    if (d->w < 1 || d->h < 1) return fail(c, NALO_ERR_ARG, W + "w and h must be >= 1");
    const long long sy = d->stride_y, sx = d->stride_x, sc = d->channels == 3 ? d->stride_c : 0, e = (long long)el;
    if (sy < 0 || sx < 0 || sc < 0) return fail(c, NALO_ERR_ARG, W + "negative stride");
    // the loads are naturally aligned ones: the address of every element is a multiple of its size
    if ((uintptr_t)d->ptr % el || sy % e || sx % e || sc % e) return fail(c, NALO_ERR_ARG, W + "pointer or stride is not a multiple of the element size");
    // inside a row no two elements may overlap: pixels at least an element apart, and the three channels either inside the pixel step (interleaved) or a step
    // beyond the row (planar)
    const __int128 row = (__int128)(d->w - 1) * sx + e;                    // bytes one channel of a row spans
    if (d->w > 1 && sx < e) return fail(c, NALO_ERR_ARG, W + "stride_x smaller than the element");
    if (d->channels == 3) {
        const bool interleaved = sc >= e && (d->w == 1 || (__int128)2 * sc + e <= sx), planar = (__int128)sc >= row;
        if (!interleaved && !planar) return fail(c, NALO_ERR_ARG, W + "stride_c makes the channels overlap inside a row");
    }
    const __int128 extent = (__int128)(d->h - 1) * sy + (__int128)(d->w - 1) * sx + (__int128)(d->channels - 1) * sc + e;
    if (extent > ((__int128)1 << 62)) return fail(c, NALO_ERR_ARG, W + "the described extent is not an allocation's");
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, d->ptr) != hipSuccess) { (void)hipGetLastError(); return fail(c, NALO_ERR_ARG, W + "not memory the runtime knows (a host pointer?)"); }
    if (at.type != hipMemoryTypeDevice || at.isManaged || at.device != c->device) return fail(c, NALO_ERR_ARG, W + "not device memory of the context's GPU (host, pinned, managed and other devices' memory are refused)");
    void* base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(d->ptr)) != hipSuccess) (void)hipGetLastError();      // no answer: the extent cannot be checked
    else if ((__int128)((const char*)d->ptr - (const char*)base) + extent > (__int128)size) return fail(c, NALO_ERR_ARG, W + "the described bytes leave the allocation");
    return NALO_OK;
}
int nalo_dev_plane_check(nalo_ctx* c, const nalo_dev_plane* plane) {
    if (!c) return NALO_ERR_ARG;
    return dev_plane_validate(c, plane, "nalo_dev_plane_check", "plane");
}

// Sensor frame / rectified image, mask and colour from device memory, in stream order: the main stream waits (on the device) for what producer_stream has queued,
// ingest / copy, attach and the pyramid are queued on it, and the slot's ev_up is recorded behind the last kernel that reads a caller's plane. Everything is
// checked before anything is queued, reserved or changed. No host wait in steady state (buffers sized, the gamma table of the last call).
int nalo_frame_ingest_device(nalo_ctx* c, int slot, const nalo_frame_ingest_args* a) {
    const char* who = "nalo_frame_ingest_device";
    if (!c || !a || slot < 0 || slot >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: bad argument");
    if (!a->image && !a->mask && !a->colour) return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: no plane given");
    NALO_HIP(c, hipSetDevice(c->device));
    FrameSlot& s = c->slots[slot];
    int rc;
    if (a->image && (rc = dev_plane_validate(c, a->image, who, "image"))) return rc;
    if (a->mask && (rc = dev_plane_validate(c, a->mask, who, "mask"))) return rc;
    if (a->colour && (rc = dev_plane_validate(c, a->colour, who, "colour"))) return rc;
    int photometric = 0;
    if (a->image) {
        const nalo_dev_plane& im = *a->image;
        if (im.channels != 1) return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: the image has one channel");
        if (im.dtype == NALO_DT_F32) {
            if (im.w != c->w || im.h != c->h) return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: a rectified (F32) image is w x h");
        } else if (im.dtype == NALO_DT_U8 || im.dtype == NALO_DT_U16) {
            if (!c->und_set) return fail(c, NALO_ERR_STATE, "nalo_frame_ingest_device: nalo_undist_set has not run");
            if (im.w != c->und_wOrg || im.h != c->und_hOrg) return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: a sensor (U8 / U16) image is und_wOrg x und_hOrg");
            photometric = a->exposure_time <= 0 ? 0 : c->und_photometric;                                  // as nalo_frame_upload_raw (processFrame, Undistort.cpp:224-231)
            if (photometric > 0 && im.dtype == NALO_DT_U16 && c->und_GDepth < 65536) return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: 16-bit frames index G beyond its depth");
        } else return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: the image is U8 / U16 (sensor) or F32 (rectified)");
    } else if (!s.valid) return fail(c, NALO_ERR_STATE, "nalo_frame_ingest_device: attach needs a slot that holds a pyramid");
    if (a->mask && (a->mask->channels != 1 || (a->mask->dtype != NALO_DT_U8 && a->mask->dtype != NALO_DT_I32 && a->mask->dtype != NALO_DT_F32)))
        return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: the mask is one channel of U8, I32 or F32");
    if (a->colour && (a->colour->channels != 3 || a->colour->dtype != NALO_DT_U8)) return fail(c, NALO_ERR_ARG, "nalo_frame_ingest_device: the colour image is three channels of U8");
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "frame_ingest_device");
    const size_t n0 = (size_t)c->w * c->h;
    NALO_HIP(c, s.ev_up.create(hipEventDisableTiming)); NALO_HIP(c, c->ev_prod.create(hipEventDisableTiming));
    if (a->mask) NALO_HIP(c, s.mask.reserve(n0));
    if (a->colour) NALO_HIP(c, s.bgr.reserve(n0 * 3));
    const bool gamma = a->image && a->gammaB;
    if (gamma) {                                                           // the table goes the way the asynchronous uploads send it: only when it differs from the last one
        NALO_HIP(c, c->copy.create()); NALO_HIP(c, c->ev_main.create(hipEventDisableTiming)); NALO_HIP(c, c->gamma_dev.reserve(256));
        bool sent = false;
        rc = gamma_upload_async(c, a->gammaB, &sent); if (rc) return rc;
        if (sent) { NALO_HIP(c, hipEventRecord(s.ev_up, c->copy)); NALO_HIP(c, hipStreamWaitEvent(c->stream, s.ev_up, 0)); }
    }
    hipStream_t prod = (hipStream_t)a->producer_stream;                    // NULL: the null stream, which the context's non-blocking stream does not wait for by itself
    if (prod != (hipStream_t)c->stream) { NALO_HIP(c, hipEventRecord(c->ev_prod, prod)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0)); }
    if (a->image) {
        rc = ingest_dev_launch(c, c->stream, *a->image, c->und_G.p, c->und_vig ? c->und_vinv.p : nullptr, c->und_remap ? reinterpret_cast<const float2*>(c->und_rxy.p) : nullptr,
                               photometric, a->factor, s.I[0].p);
        if (rc) return rc;
    }
    rc = attach_launch(c, c->stream, a->mask, a->colour, a->colour_is_rgb, s.mask.p, s.bgr.p); if (rc) return rc;
    NALO_HIP(c, hipEventRecord(s.ev_up, c->stream));                       // the caller's planes have been read: nalo_frame_wait / nalo_frame_release
    if (a->image) {
        rc = pyramid_build(c, s, gamma ? c->gamma_dev.p : nullptr); if (rc) return rc;
        pixsel_invalidate_hists(c, slot);
        s.valid = true;
    } else pixsel_invalidate_map(c, slot);
    return NALO_OK;
}

int nalo_frame_release(nalo_ctx* c, int slot, void* stream) {
    if (!c || slot < 0 || slot >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_frame_release: bad slot");
    if (!c->slots[slot].ev_up) return NALO_OK;                             // nothing was ever ingested into the slot: nothing to wait for
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamWaitEvent((hipStream_t)stream, c->slots[slot].ev_up, 0));
    return NALO_OK;
}

// Mask and colour for a slot that already holds a pyramid, from host memory in the sensor's size: the tracked frame that became a keyframe (FullSystem.cpp:1113-1132)
// gets the keyframe-only inputs without its image being sent or its pyramid being built again. Staged through und_mask / und_bgr like nalo_frame_upload_raw.
int nalo_frame_attach(nalo_ctx* c, int slot, const uint8_t* mask_org, const uint8_t* bgr_org) {
    if (!c || slot < 0 || slot >= (int)c->slots.size() || (!mask_org && !bgr_org)) return fail(c, NALO_ERR_ARG, "nalo_frame_attach: bad argument");
    if (!c->und_set) return fail(c, NALO_ERR_STATE, "nalo_frame_attach: nalo_undist_set has not run");
    FrameSlot& s = c->slots[slot];
    if (!s.valid) return fail(c, NALO_ERR_STATE, "nalo_frame_attach: the slot holds no pyramid");
    NALO_HIP(c, hipSetDevice(c->device));
    const size_t no = (size_t)c->und_wOrg * c->und_hOrg, n0 = (size_t)c->w * c->h;
    nalo_dev_plane m = {}, b = {};
    if (mask_org) {
        NALO_HIP(c, c->und_mask.reserve(no)); NALO_HIP(c, s.mask.reserve(n0));
        NALO_HIP(c, hipMemcpyAsync(c->und_mask.p, mask_org, no, hipMemcpyHostToDevice, c->stream));
        m.ptr = c->und_mask.p; m.dtype = NALO_DT_U8; m.w = c->und_wOrg; m.h = c->und_hOrg; m.channels = 1; m.stride_y = c->und_wOrg; m.stride_x = 1;
    }
    if (bgr_org) {
        NALO_HIP(c, c->und_bgr.reserve(no * 3)); NALO_HIP(c, s.bgr.reserve(n0 * 3));
        NALO_HIP(c, hipMemcpyAsync(c->und_bgr.p, bgr_org, no * 3, hipMemcpyHostToDevice, c->stream));
        b.ptr = c->und_bgr.p; b.dtype = NALO_DT_U8; b.w = c->und_wOrg; b.h = c->und_hOrg; b.channels = 3; b.stride_y = 3LL * c->und_wOrg; b.stride_x = 3; b.stride_c = 1;
    }
    int rc = attach_launch(c, c->stream, mask_org ? &m : nullptr, bgr_org ? &b : nullptr, 0, s.mask.p, s.bgr.p); if (rc) return rc;
    pixsel_invalidate_map(c, slot);
    NALO_HIP(c, hipStreamSynchronize(c->stream));                          // host buffers are caller-owned: safe to reuse on return
    return NALO_OK;
}

int nalo_frame_wait(nalo_ctx* c, int slot) {
    if (!c || slot < 0 || slot >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_frame_wait: bad slot");
    if (c->slots[slot].ev_up) NALO_HIP(c, hipEventSynchronize(c->slots[slot].ev_up));
    return NALO_OK;
}
void* nalo_host_alloc(size_t bytes) { void* p = nullptr; return hipHostMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
void nalo_host_free(void* p) { if (p) (void)hipHostFree(p); }

int nalo_frame_rebuild(nalo_ctx* c, int slot) {
    if (!c || slot < 0 || slot >= (int)c->slots.size() || !c->slots[slot].valid) return fail(c, NALO_ERR_ARG, "nalo_frame_rebuild: bad slot");
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "frame_rebuild");
    return pyramid_build(c, c->slots[slot], nullptr);
}

int nalo_frame_download(nalo_ctx* c, int slot, int lvl, float* dI3, float* absg) {
    if (!c || slot < 0 || slot >= (int)c->slots.size() || lvl < 0 || lvl >= c->levels) return fail(c, NALO_ERR_ARG, "nalo_frame_download: bad argument");
    FrameSlot& s = c->slots[slot];
    if (!s.valid) return fail(c, NALO_ERR_STATE, "nalo_frame_download: empty slot");
    const size_t npx = (size_t)c->wl[lvl] * c->hl[lvl];
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    if (dI3) {
        std::vector<float4> tmp(npx);
        NALO_HIP(c, hipMemcpy(tmp.data(), s.dI[lvl].p, npx * 16, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < npx; ++i) { dI3[3 * i] = tmp[i].x; dI3[3 * i + 1] = tmp[i].y; dI3[3 * i + 2] = tmp[i].z; }
    }
    if (absg) NALO_HIP(c, hipMemcpy(absg, s.absg[lvl].p, npx * 4, hipMemcpyDeviceToHost));
    return NALO_OK;
}

int nalo_frame_download_mask(nalo_ctx* c, int slot, float* mask, uint8_t* bgr) {
    if (!c || slot < 0 || slot >= (int)c->slots.size() || (!mask && !bgr)) return fail(c, NALO_ERR_ARG, "nalo_frame_download_mask: bad argument");
    FrameSlot& s = c->slots[slot];
    if (!s.valid || (mask && !s.mask.p) || (bgr && !s.bgr.p)) return fail(c, NALO_ERR_STATE, "nalo_frame_download_mask: the slot holds no such plane");
    const size_t n0 = (size_t)c->w * c->h;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    if (mask) NALO_HIP(c, hipMemcpy(mask, s.mask.p, n0 * 4, hipMemcpyDeviceToHost));
    if (bgr) NALO_HIP(c, hipMemcpy(bgr, s.bgr.p, n0 * 3, hipMemcpyDeviceToHost));
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ tracker
int nalo_trk_make_k(nalo_ctx* c, float fx, float fy, float cx, float cy) {
    if (!c) return NALO_ERR_ARG;
    set_pyr_calib(c, fx, fy, cx, cy);
    return NALO_OK;
}

static int upload4(nalo_ctx* c, int n, const float* a, const float* b, const float* d, const float* e, float** dev) {
    // one pinned staging buffer, one H2D copy (four pageable copies cost four blocking round trips); the previous upload has been consumed:
    // trk_build_ref ends on a flag published after it in stream order
    NALO_HIP(c, c->upload_tmp.reserve((size_t)4 * n + 256));
    if (c->pinned_f.cap < (size_t)4 * n) NALO_HIP(c, c->pinned_f.reserve((size_t)4 * n + 256));   // 256 floats of slack: a slightly larger cloud does not reallocate
    float* base = c->upload_tmp.p + 256;
    const float* src[4] = {a, b, d, e};
    for (int k = 0; k < 4; ++k) { std::memcpy(c->pinned_f.p + (size_t)k * n, src[k], (size_t)n * 4); dev[k] = base + (size_t)k * n; }
    NALO_HIP(c, hipMemcpyAsync(base, c->pinned_f.p, (size_t)4 * n * 4, hipMemcpyHostToDevice, c->stream));
    return NALO_OK;
}

int nalo_trk_set_ref(nalo_ctx* c, int slot_ref, int n, const float* Ku, const float* Kv, const float* new_idepth, const float* HdiF) {
    if (!c || slot_ref < 0 || slot_ref >= (int)c->slots.size() || n < 0 || (n > 0 && (!Ku || !Kv || !new_idepth || !HdiF)))
        return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref: bad argument");
    if (!c->slots[slot_ref].valid) return fail(c, NALO_ERR_STATE, "nalo_trk_set_ref: reference slot has no pyramid");
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "trk_set_ref");
    c->slot_ref = slot_ref;
    float* dev[4] = {};
    if (n > 0) { int rc = upload4(c, n, Ku, Kv, new_idepth, HdiF, dev); if (rc) return rc; }
    return trk_build_ref(c, n, dev[0], dev[1], dev[2], dev[3]);
}

int nalo_trk_ref_upload(nalo_ctx* c, int n, const float* Ku, const float* Kv, const float* new_idepth, const float* HdiF) {
    if (!c || n < 0 || (n > 0 && (!Ku || !Kv || !new_idepth || !HdiF))) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_upload: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    c->ref_res_n = -1;
    if (n > 0) {
        float* dev[4] = {};
        int rc = upload4(c, n, Ku, Kv, new_idepth, HdiF, dev); if (rc) return rc;                  // pinned staging + ONE H2D copy into the shared scratch ...
        NALO_HIP(c, c->ref_res.reserve((size_t)4 * n));
        NALO_HIP(c, hipMemcpyAsync(c->ref_res.p, dev[0], (size_t)4 * n * 4, hipMemcpyDeviceToDevice, c->stream));   // ... and from there into the block that stays
        NALO_HIP(c, hipStreamSynchronize(c->stream));                                              // the staging buffers are free again when this returns
    }
    c->ref_res_n = n;
    return NALO_OK;
}
int nalo_trk_set_ref_resident(nalo_ctx* c, int slot_ref) {
    if (!c || slot_ref < 0 || slot_ref >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_resident: bad argument");
    if (!c->slots[slot_ref].valid) return fail(c, NALO_ERR_STATE, "nalo_trk_set_ref_resident: reference slot has no pyramid");
    if (c->ref_res_n < 0) return fail(c, NALO_ERR_STATE, "nalo_trk_set_ref_resident: no resident inputs (nalo_trk_ref_upload)");
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "trk_set_ref");
    c->slot_ref = slot_ref;
    const size_t n = (size_t)c->ref_res_n;
    const float* b = c->ref_res.p;
    return trk_build_ref(c, c->ref_res_n, b, b + n, b + 2 * n, b + 3 * n);
}
int nalo_trk_set_ref_from_window(nalo_ctx* c) {
    if (!c) return NALO_ERR_ARG;
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "trk_set_ref");
    int slot = -1, n = 0; const float* b = nullptr;
    const int rc = ba_trk_ref_inputs(c, &slot, &n, &b); if (rc) return rc;     // the gather is in the stream: no host copy, no round trip
    c->slot_ref = slot;
    return trk_build_ref(c, n, b, b + n, b + 2 * (size_t)n, b + 3 * (size_t)n);
}
// a2 fed from a depth plane on the device. Everything is tested before anything is queued or reserved, and slot_ref moves only once the call is accepted; then
// the main stream waits (on the device) for the producer, ONE kernel reads the plane and the call ends on the pc_n poll behind it.
int nalo_trk_set_ref_from_depth(nalo_ctx* c, int slot_ref, nalo_trk_depth_ref_args* a) {
    if (a) a->n_seeded = 0;
    if (!c || !a) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: bad argument");
    if (slot_ref < 0 || slot_ref >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: bad slot_ref");
    NALO_HIP(c, hipSetDevice(c->device));
    { const int rc = dev_plane_validate(c, &a->depth, "nalo_trk_set_ref_from_depth", "depth"); if (rc) return rc; }
    if (a->depth.dtype != NALO_DT_F32 || a->depth.channels != 1) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: the depth plane is one channel of F32");
    if (a->depth.w != c->w || a->depth.h != c->h) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: the depth plane's w x h differ from the context's");
    if (!std::isfinite(a->min_depth) || !(a->min_depth > 0.0f)) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: min_depth must be finite and > 0");
    if (!std::isfinite(a->max_depth) || a->min_depth > a->max_depth) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: max_depth must be finite and >= min_depth");
    if (!std::isfinite(a->hdi) || a->hdi < 0.0f) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: hdi must be finite and >= 0");
    if (a->step < 1) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: step must be >= 1");
    if (a->min_grad != a->min_grad) return fail(c, NALO_ERR_ARG, "nalo_trk_set_ref_from_depth: min_grad is NaN");
    if (!c->slots[slot_ref].valid) return fail(c, NALO_ERR_STATE, "nalo_trk_set_ref_from_depth: reference slot has no pyramid");
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "trk_set_ref_from_depth");
    NALO_HIP(c, c->ev_prod.create(hipEventDisableTiming));
    hipStream_t prod = (hipStream_t)a->producer_stream;                    // NULL: the null stream, which the context's non-blocking stream does not wait for by itself
    if (prod != (hipStream_t)c->stream) { NALO_HIP(c, hipEventRecord(c->ev_prod, prod)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0)); }
    c->slot_ref = slot_ref;
    return trk_build_ref_from_depth(c, a->depth, a->min_depth, a->max_depth, a->hdi, a->step, a->min_grad, &a->n_seeded);
}

int nalo_trk_set_pc(nalo_ctx* c, int slot_ref, int lvl, int n, const float* u, const float* v, const float* idepth, const float* color) {
    if (!c || slot_ref < 0 || slot_ref >= (int)c->slots.size() || lvl < 0 || lvl >= c->levels || n < 0) return fail(c, NALO_ERR_ARG, "nalo_trk_set_pc: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    c->slot_ref = slot_ref;
    const size_t cap = std::max((size_t)n, (size_t)c->wl[lvl] * c->hl[lvl]);
    NALO_HIP(c, c->pc_u[lvl].reserve(cap)); NALO_HIP(c, c->pc_v[lvl].reserve(cap)); NALO_HIP(c, c->pc_id[lvl].reserve(cap)); NALO_HIP(c, c->pc_col[lvl].reserve(cap));
    NALO_HIP(c, hipMemcpy(c->pc_u[lvl].p, u, (size_t)n * 4, hipMemcpyHostToDevice));
    NALO_HIP(c, hipMemcpy(c->pc_v[lvl].p, v, (size_t)n * 4, hipMemcpyHostToDevice));
    NALO_HIP(c, hipMemcpy(c->pc_id[lvl].p, idepth, (size_t)n * 4, hipMemcpyHostToDevice));
    NALO_HIP(c, hipMemcpy(c->pc_col[lvl].p, color, (size_t)n * 4, hipMemcpyHostToDevice));
    c->pc_n[lvl] = n;
    return NALO_OK;
}

// dense=1 glue: append the plane-sampled points of one mask cluster to the level-0 cloud on the device (CoarseTracker.cpp:628-655)
int nalo_trk_append_plane_points(nalo_ctx* c, const float dir[3], float dis_plane, int refMaskColor, const int rect[4], int* n_added) {
    if (!c || !dir || !rect) return fail(c, NALO_ERR_ARG, "nalo_trk_append_plane_points: bad argument");
    if (c->slot_ref < 0 || !c->slots[c->slot_ref].valid || !c->pc_u[0].p) return fail(c, NALO_ERR_STATE, "nalo_trk_append_plane_points: no tracking reference");
    const FrameSlot& s = c->slots[c->slot_ref];
    if (!s.mask.p) return fail(c, NALO_ERR_STATE, "nalo_trk_append_plane_points: the reference frame was uploaded without a mask");
    const int minx = rect[0], maxx = rect[1], miny = rect[2], maxy = rect[3];
    // `if(maxx>w[0]-1||minx<1||maxy>h[0]-1||miny<1) continue;` and `if (refMaskColor==0) continue;` (:621-630): nothing is appended
    if (n_added) *n_added = 0;
    if (maxx > c->w - 1 || minx < 1 || maxy > c->h - 1 || miny < 1 || refMaskColor == 0 || dis_plane == 0.f) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    const int x0 = ((minx + 4) / 5) * 5, y0 = ((miny + 4) / 5) * 5;
    const int nx = x0 < maxx ? (maxx - 1 - x0) / 5 + 1 : 0, ny = y0 < maxy ? (maxy - 1 - y0) / 5 + 1 : 0;
    const int n0 = c->pc_n[0];
    if ((size_t)n0 + 2 + (size_t)nx * ny > c->pc_u[0].cap) return fail(c, NALO_ERR_STATE, "nalo_trk_append_plane_points: the level-0 cloud would outgrow its w*h buffer");
    if (nx == 0 || ny == 0) return NALO_OK;
    NALO_HIP(c, c->scan_tmp.reserve(64));
    int rc = trk_append_plane_launch(c, s.mask.p, s.dI[0].p, dir, dis_plane, (float)refMaskColor, x0, nx, y0, ny, n0, c->scan_tmp.p); if (rc) return rc;
    int added = 0;
    NALO_HIP(c, hipMemcpyAsync(&added, c->scan_tmp.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    c->pc_n[0] = n0 + added;
    if (n_added) *n_added = added;
    return NALO_OK;
}

int nalo_trk_get_pc(nalo_ctx* c, int lvl, int* n, float* u, float* v, float* idepth, float* color) {
    if (!c || lvl < 0 || lvl >= c->levels || !n) return fail(c, NALO_ERR_ARG, "nalo_trk_get_pc: bad argument");
    *n = c->pc_n[lvl];
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const size_t b = (size_t)c->pc_n[lvl] * 4;
    if (u && b) NALO_HIP(c, hipMemcpy(u, c->pc_u[lvl].p, b, hipMemcpyDeviceToHost));
    if (v && b) NALO_HIP(c, hipMemcpy(v, c->pc_v[lvl].p, b, hipMemcpyDeviceToHost));
    if (idepth && b) NALO_HIP(c, hipMemcpy(idepth, c->pc_id[lvl].p, b, hipMemcpyDeviceToHost));
    if (color && b) NALO_HIP(c, hipMemcpy(color, c->pc_col[lvl].p, b, hipMemcpyDeviceToHost));
    return NALO_OK;
}

int nalo_trk_get_depth(nalo_ctx* c, int lvl, float* idepth, float* wsum) {
    if (!c || lvl < 0 || lvl >= c->levels) return fail(c, NALO_ERR_ARG, "nalo_trk_get_depth: bad argument");
    if (!c->trk_idepth[lvl].p) return fail(c, NALO_ERR_STATE, "nalo_trk_get_depth: no reference set");
    const size_t b = (size_t)c->wl[lvl] * c->hl[lvl] * 4;
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    if (idepth) NALO_HIP(c, hipMemcpy(idepth, c->trk_idepth[lvl].p, b, hipMemcpyDeviceToHost));
    if (wsum) NALO_HIP(c, hipMemcpy(wsum, c->trk_wsum[lvl].p, b, hipMemcpyDeviceToHost));
    return NALO_OK;
}

// direct injection of one level's inverse-depth map / weight sums: the counterpart of nalo_trk_get_depth. Nothing else is touched (no cloud, no other level).
int nalo_trk_set_depth(nalo_ctx* c, int slot_ref, int lvl, const float* idepth, const float* wsum) {
    if (!c || slot_ref < 0 || slot_ref >= (int)c->slots.size() || lvl < 0 || lvl >= c->levels) return fail(c, NALO_ERR_ARG, "nalo_trk_set_depth: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->wl[lvl] * c->hl[lvl];
    const bool fresh = !c->trk_idepth[lvl].p;
    NALO_HIP(c, c->trk_idepth[lvl].reserve(npx)); NALO_HIP(c, c->trk_wsum[lvl].reserve(npx)); NALO_HIP(c, c->trk_wbak[lvl].reserve(npx));
    if (fresh) {                                                                 // a half that is not given reads as zeros, not as whatever the allocation held
        NALO_HIP(c, hipMemsetAsync(c->trk_idepth[lvl].p, 0, npx * 4, c->stream));
        NALO_HIP(c, hipMemsetAsync(c->trk_wsum[lvl].p, 0, npx * 4, c->stream));
    }
    c->slot_ref = slot_ref;
    // on the main stream, behind whatever nalo_trk_set_ref* enqueued on these buffers
    if (idepth) NALO_HIP(c, hipMemcpyAsync(c->trk_idepth[lvl].p, idepth, npx * 4, hipMemcpyHostToDevice, c->stream));
    if (wsum) NALO_HIP(c, hipMemcpyAsync(c->trk_wsum[lvl].p, wsum, npx * 4, hipMemcpyHostToDevice, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));                                // the arrays are the caller's: free to reuse on return
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ views and the hand-off between contexts
// One level-0 plane of a slot as a descriptor (the reverse of nalo_frame_ingest_device). Host code only; the refusals are nalo_frame_download_mask's.
int nalo_frame_plane(nalo_ctx* c, int slot, int which, nalo_dev_plane* out) {
    if (!c || !out || slot < 0 || slot >= (int)c->slots.size() || which < NALO_PLANE_IRRADIANCE || which > NALO_PLANE_COLOUR) return fail(c, NALO_ERR_ARG, "nalo_frame_plane: bad argument");
    const FrameSlot& s = c->slots[slot];
    if (!s.valid || (which == NALO_PLANE_MASK && !s.mask.p) || (which == NALO_PLANE_COLOUR && !s.bgr.p)) return fail(c, NALO_ERR_STATE, "nalo_frame_plane: the slot holds no such plane");
    nalo_dev_plane d = {};
    d.w = c->w; d.h = c->h;
    if (which == NALO_PLANE_COLOUR) { d.ptr = s.bgr.p; d.dtype = NALO_DT_U8; d.channels = 3; d.stride_y = 3LL * c->w; d.stride_x = 3; d.stride_c = 1; }
    else { d.ptr = which == NALO_PLANE_MASK ? s.mask.p : s.I[0].p; d.dtype = NALO_DT_F32; d.channels = 1; d.stride_y = 4LL * c->w; d.stride_x = 4; }
    *out = d;
    return NALO_OK;
}

// The current reference as pointers and counts. A level without a cloud (nalo_trk_set_depth alone) reads n = 0, one without maps (nalo_trk_set_pc alone) NULL maps.
int nalo_trk_ref_export(nalo_ctx* c, nalo_trk_ref_view* out) {
    if (!c || !out) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_export: bad argument");
    if (c->slot_ref < 0) return fail(c, NALO_ERR_STATE, "nalo_trk_ref_export: no tracking reference (nalo_trk_set_ref* / nalo_trk_set_pc / nalo_trk_set_depth / nalo_trk_ref_import)");
    nalo_trk_ref_view v = {};
    v.w = c->w; v.h = c->h; v.levels = c->levels; v.slot_ref = c->slot_ref;
    for (int l = 0; l < c->levels; ++l) {
        const bool cloud = c->pc_u[l].p && c->pc_v[l].p && c->pc_id[l].p && c->pc_col[l].p;
        v.n[l] = cloud ? c->pc_n[l] : 0;
        if (cloud) { v.u[l] = c->pc_u[l].p; v.v[l] = c->pc_v[l].p; v.idepth[l] = c->pc_id[l].p; v.color[l] = c->pc_col[l].p; }
        if (c->trk_idepth[l].p && c->trk_wsum[l].p) { v.idepth_map[l] = c->trk_idepth[l].p; v.weight_sums[l] = c->trk_wsum[l].p; }
        v.fx[l] = c->fx[l]; v.fy[l] = c->fy[l]; v.cx[l] = c->cx[l]; v.cy[l] = c->cy[l];
    }
    v.stream = (void*)(hipStream_t)c->stream;
    *out = v;
    return NALO_OK;
}

// dst becomes a clone of the described reference. Everything is tested before anything is queued or reserved; then the main stream waits (on the device) for the
// producer, ONE kernel copies every segment (kernels_handoff.hip) and ev_imp is recorded behind it. The other context is never touched: only its stream handle is.
int nalo_trk_ref_import(nalo_ctx* c, int slot_ref, const nalo_trk_ref_view* v) {
    const char* who = "nalo_trk_ref_import";
    if (!c || !v) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_import: bad argument");
    if (slot_ref < 0 || slot_ref >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_import: bad slot_ref");
    if (c->xchg_failed) return fail(c, NALO_ERR_HIP, "nalo_trk_ref_import: a cross-rank sum of this context failed earlier; rebuild on a new context");
    if (v->w != c->w || v->h != c->h || v->levels != c->levels) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_import: the view's w, h or levels differ from the context's");
    NALO_HIP(c, hipSetDevice(c->device));
    for (int l = 0; l < c->levels; ++l) {
        const long long npx = (long long)c->wl[l] * c->hl[l];
        if (v->n[l] < 0 || v->n[l] > npx) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_import: n[l] outside 0 .. (w>>l)*(h>>l)");
        const float* cloud[4] = {v->u[l], v->v[l], v->idepth[l], v->color[l]};
        static const char* const cname[4] = {"u", "v", "idepth", "color"};
        if (v->n[l] > 0) for (int k = 0; k < 4; ++k) {
            if (!cloud[k]) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_import: a null cloud pointer with n[l] > 0");
            nalo_dev_plane d = {};                                             // n floats as one row: dev_plane_validate's pointer, alignment and extent tests
            d.ptr = cloud[k]; d.dtype = NALO_DT_F32; d.w = v->n[l]; d.h = 1; d.channels = 1; d.stride_y = 4LL * v->n[l]; d.stride_x = 4;
            const int rc = dev_plane_validate(c, &d, who, cname[k]); if (rc) return rc;
        }
        if (!v->idepth_map[l] != !v->weight_sums[l]) return fail(c, NALO_ERR_ARG, "nalo_trk_ref_import: idepth_map and weight_sums are given together or not at all");
        if (v->idepth_map[l]) for (const float* m : {v->idepth_map[l], v->weight_sums[l]}) {
            nalo_dev_plane d = {};
            d.ptr = m; d.dtype = NALO_DT_F32; d.w = c->wl[l]; d.h = c->hl[l]; d.channels = 1; d.stride_y = 4LL * c->wl[l]; d.stride_x = 4;
            const int rc = dev_plane_validate(c, &d, who, m == v->idepth_map[l] ? "idepth_map" : "weight_sums"); if (rc) return rc;
        }
    }
    if (!c->slots[slot_ref].valid) return fail(c, NALO_ERR_STATE, "nalo_trk_ref_import: slot_ref holds no pyramid");
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "trk_ref_import");
    HandoffTable T = {};
    for (int l = 0; l < c->levels; ++l) {
        const size_t npx = (size_t)c->wl[l] * c->hl[l];
        NALO_HIP(c, c->trk_idepth[l].reserve(npx)); NALO_HIP(c, c->trk_wsum[l].reserve(npx)); NALO_HIP(c, c->trk_wbak[l].reserve(npx));
        NALO_HIP(c, c->pc_u[l].reserve(npx)); NALO_HIP(c, c->pc_v[l].reserve(npx)); NALO_HIP(c, c->pc_id[l].reserve(npx)); NALO_HIP(c, c->pc_col[l].reserve(npx));
        const float* src[6] = {v->u[l], v->v[l], v->idepth[l], v->color[l], v->idepth_map[l], v->weight_sums[l]};
        float* dst[6] = {c->pc_u[l].p, c->pc_v[l].p, c->pc_id[l].p, c->pc_col[l].p, c->trk_idepth[l].p, c->trk_wsum[l].p};
        for (int k = 0; k < 6; ++k) {
            HandoffSeg& S = T.seg[T.nseg++];
            S.src = reinterpret_cast<const uint32_t*>(src[k]); S.dst = reinterpret_cast<uint32_t*>(dst[k]); S.words = k < 4 ? (size_t)v->n[l] : npx;
        }
    }
    NALO_HIP(c, c->ev_imp.create(hipEventDisableTiming)); NALO_HIP(c, c->ev_prod.create(hipEventDisableTiming));
    hipStream_t prod = (hipStream_t)v->stream;
    if (prod != (hipStream_t)c->stream) { NALO_HIP(c, hipEventRecord(c->ev_prod, prod)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0)); }
    const int rc = handoff_copy_launch(c, T); if (rc) return rc;
    NALO_HIP(c, hipEventRecord(c->ev_imp, c->stream));                     // the caller's arrays have been read: nalo_trk_ref_release
    c->slot_ref = slot_ref;
    for (int l = 0; l < c->levels; ++l) { c->pc_n[l] = v->n[l]; c->fx[l] = v->fx[l]; c->fy[l] = v->fy[l]; c->cx[l] = v->cx[l]; c->cy[l] = v->cy[l]; }
    return NALO_OK;
}

int nalo_trk_ref_release(nalo_ctx* c, void* stream) {
    if (!c) return NALO_ERR_ARG;
    if (!c->ev_imp) return NALO_OK;                                        // nothing was ever imported: nothing to wait for
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamWaitEvent((hipStream_t)stream, c->ev_imp, 0));
    return NALO_OK;
}

// CoarseTracker::debugPlotIDepthMap (CoarseTracker.cpp:1263-1359) from the resident level-0 map and the reference slot's irradiance (kernels_depth_image.hip).
// Everything is enqueued on the main stream; the image, the optional map and the scalars come up through one pinned block behind ONE wait, and reach the
// caller's arrays only when the call succeeds.
int nalo_trk_depth_image(nalo_ctx* c, nalo_depth_image_args* a) {
    if (!c || !a || !a->bgr) return fail(c, NALO_ERR_ARG, "nalo_trk_depth_image: bad argument");
    if (c->xchg_failed) return fail(c, NALO_ERR_HIP, "nalo_trk_depth_image: a cross-rank sum of this context failed earlier; rebuild on a new context");
    if (c->slot_ref < 0 || !c->slots[c->slot_ref].valid || !c->trk_idepth[0].p) return fail(c, NALO_ERR_STATE, "nalo_trk_depth_image: no tracking reference (nalo_trk_set_ref* / nalo_trk_set_depth on a slot that holds a frame)");
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "trk_depth_image");
    const size_t npx = (size_t)c->w * c->h, off_bgr = 64, off_id = off_bgr + ((3 * npx + 15) & ~(size_t)15);
    NALO_HIP(c, c->di_scr.reserve(kDepthImageScratchWords)); NALO_HIP(c, c->di_bgr.reserve(3 * npx));
    NALO_HIP(c, c->di_host.reserve(off_id + (a->idepth ? 4 * npx : 0)));
    const float* const map = c->trk_idepth[0].p;
    const bool io = a->minmax_io != nullptr;
    unsigned* const res_dev = c->di_scr.p + kDepthImageScratchWords - 8;
    {
        ProfScope ps(c, "trk_depth_image");
        const int rc = depth_image_launch(c, map, c->slots[c->slot_ref].I[0].p, io ? a->minmax_io[0] : 0.f, io ? a->minmax_io[1] : 0.f, io ? 1 : 0, c->di_scr.p, c->di_bgr.p);
        if (rc) return rc;
    }
    NALO_HIP(c, hipMemcpyAsync(c->di_host.p, res_dev, 32, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(c->di_host.p + off_bgr, c->di_bgr.p, 3 * npx, hipMemcpyDeviceToHost, c->stream));
    if (a->idepth) NALO_HIP(c, hipMemcpyAsync(c->di_host.p + off_id, map, 4 * npx, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    unsigned res[8];
    std::memcpy(res, c->di_host.p, sizeof(res));
    a->n_positive = (int)res[0];
    if (res[0] == 0) return fail(c, NALO_ERR_STATE, "nalo_trk_depth_image: the level-0 map holds no positive inverse depth");   // the reference indexes an empty vector here
    std::memcpy(&a->min_new, &res[1], 4); std::memcpy(&a->max_new, &res[2], 4);
    std::memcpy(&a->min_used, &res[3], 4); std::memcpy(&a->max_used, &res[4], 4);
    if (io) std::memcpy(a->minmax_io, &res[5], 8);
    std::memcpy(a->bgr, c->di_host.p + off_bgr, 3 * npx);
    if (a->idepth) std::memcpy(a->idepth, c->di_host.p + off_id, 4 * npx);
    return NALO_OK;
}

// SURVEY 8(e), tracker: every rank holds the whole reference (nalo_trk_set_ref is replicated: makeCoarseDepthL0's dilation and normalisation need every point's
// neighbours) and evaluates rank/world of every level's point cloud; the 45 + 7 sums of an evaluation are all-reduced through the hook, so every rank takes the same LM
// step. Worth it for level sizes of ~1e5 points and more (CoarseTracker.cpp:828-885 sums per thread in the reference).
int nalo_trk_set_shard(nalo_ctx* c, int rank, int world, nalo_allreduce_fn hook, void* user, int stream_ordered) {
    if (!c || world < 1 || rank < 0 || rank >= world) return fail(c, NALO_ERR_ARG, "nalo_trk_set_shard: bad argument");
    if (world > 1 && !hook) return fail(c, NALO_ERR_ARG, "nalo_trk_set_shard: a sharded tracker needs the all-reduce hook");
    c->trk_rank = rank; c->trk_world = world; c->trk_hook = world > 1 ? hook : nullptr; c->trk_hook_user = user; c->trk_hook_stream_ordered = stream_ordered != 0;
    return NALO_OK;
}

int nalo_trk_eval(nalo_ctx* c, int slot_new, int lvl, const double R[9], const double t[3], const float affLL[2], float b0,
                  float cutoffTH, int want_gs, double stats6[6], double H[64], double b[8]) {
    if (!c || !R || !t || !affLL || !stats6 || lvl < 0 || lvl >= c->levels || slot_new < 0 || slot_new >= (int)c->slots.size())
        return fail(c, NALO_ERR_ARG, "nalo_trk_eval: bad argument");
    if (c->xchg_failed) return fail(c, NALO_ERR_HIP, "nalo_trk_eval: a cross-rank sum of this context failed earlier; rebuild on a new context");
    if (c->slot_ref < 0 || !c->slots[slot_new].valid) return fail(c, NALO_ERR_STATE, "nalo_trk_eval: no reference / empty frame slot");
    if (want_gs && (!H || !b)) return fail(c, NALO_ERR_ARG, "nalo_trk_eval: H/b required");
    // RKi = R.cast<float>() * Ki[lvl], t = translation.cast<float>() (CoarseTracker.cpp:907-908)
    const float fx = c->fx[lvl], fy = c->fy[lvl], cx = c->cx[lvl], cy = c->cy[lvl];
    const float Ki[9] = {1.0f / fx, 0, -cx / fx, 0, 1.0f / fy, -cy / fy, 0, 0, 1};
    float Rf[9], RKi[9], tf[3];
    for (int i = 0; i < 9; ++i) Rf[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) RKi[i * 3 + j] = Rf[i * 3] * Ki[j] + Rf[i * 3 + 1] * Ki[3 + j] + Rf[i * 3 + 2] * Ki[6 + j];
    for (int i = 0; i < 3; ++i) tf[i] = (float)t[i];
    const float maxEnergy = 2 * kHuberTH * cutoffTH - kHuberTH * kHuberTH;          // :916
    double o[64];
    int rc = trk_eval_launch(c, slot_new, lvl, RKi, tf, Ki, affLL[0], affLL[1], b0, cutoffTH, maxEnergy, o);
    if (rc) return rc;
    const double E = o[kTrkE], nE = o[kTrkNE], nSat = o[kTrkNSat], nW = o[kTrkNWarped], sT = o[kTrkST], sRT = o[kTrkSRT], sN = o[kTrkSN];
    stats6[0] = E; stats6[1] = nE; stats6[2] = sT / (sN + 0.1); stats6[3] = 0; stats6[4] = sRT / (sN + 0.1);
    stats6[5] = (double)((float)nSat / (float)nE);
    if (want_gs) {
        const double npad = (double)(((long)nW + 3) & ~3L);          // divided by the padded count
        const double inv = 1.0 / npad;
        static const double sc[8] = {kScaleXiRot, kScaleXiRot, kScaleXiRot, kScaleXiTrans, kScaleXiTrans, kScaleXiTrans, kScaleA, kScaleB};
        for (int r = 0; r < 8; ++r) {
            for (int cc = 0; cc < 8; ++cc) H[r * 8 + cc] = o[r < cc ? trk_ut(r, cc) : trk_ut(cc, r)] * inv * sc[r] * sc[cc];
            b[r] = o[trk_ut(r, 8)] * inv * sc[r];
        }
    }
    return NALO_OK;
}

// evaluations per pyramid level and point-cloud sizes of the last nalo_trk_track (either LM driver): the algorithmic bytes of that frame are
// sum_l evals[l] * n[l] * 64 (16 B point + four 12-B taps per point and evaluation)
int nalo_trk_last_evals(nalo_ctx* c, int evals[5], int n[5]) {
    if (!c) return NALO_ERR_ARG;
    for (int i = 0; i < 5; ++i) { if (evals) evals[i] = c->lm_evals_lvl[i]; if (n) n[i] = i < c->levels ? c->pc_n[i] : 0; }
    return NALO_OK;
}
int nalo_trk_get_launch_config(nalo_ctx* c, int cfg[9]) {
    if (!c || !cfg) return fail(c, NALO_ERR_ARG, "nalo_trk_get_launch_config: bad argument");
    std::memcpy(cfg, c->trk_cfg, sizeof(c->trk_cfg));
    return NALO_OK;
}
int nalo_trk_track(nalo_ctx* c, int slot_new, double T_io[12], double aff_io[2], const double ref_aff[2], const float exposures[2],
                   int coarsestLvl, const double minResForAbort[5], double lastResiduals[5], double lastFlow[3], int* ok, int* n_evals) {
    if (!c || !T_io || !aff_io || !ref_aff || !exposures || !ok) return fail(c, NALO_ERR_ARG, "nalo_trk_track: bad argument");
    if (!(coarsestLvl >= 0 && coarsestLvl < 5 && coarsestLvl < c->levels)) return fail(c, NALO_ERR_ARG, "nalo_trk_track: coarsestLvl out of range");
    if (slot_new < 0 || slot_new >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_trk_track: frame slot out of range");
    if (c->slot_ref < 0 || !c->slots[slot_new].valid) return fail(c, NALO_ERR_STATE, "nalo_trk_track: no reference (nalo_trk_set_ref) / empty frame slot");
    if (c->xchg_failed) return fail(c, NALO_ERR_HIP, "nalo_trk_track: a cross-rank sum of this context failed earlier; rebuild on a new context");
    HostTimer ht(c, "trk_track");   // assert at :1083
    double lastRes[5] = {NAN, NAN, NAN, NAN, NAN}, flow[3] = {1000, 1000, 1000};
    SE3 cur = SE3::from(T_io);
    double aff_cur[2] = {aff_io[0], aff_io[1]};
    bool haveRepeated = false, good = true;
    int evals = 0, start_lvl = coarsestLvl;
    for (int& e : c->lm_evals_lvl) e = 0;
    // The whole pyramid descent runs in ONE persistent multi-block kernel (kernels_trk_lm.hip): ~10 us per LM evaluation against ~19 us for
    // the host-driven loop below (a launch, a finish kernel and a polled flag per evaluation), which is also what a caller gets by driving
    // nalo_trk_eval itself.
    {
        // a fixed affine parameter changes the system the LM solves (:1140-1162): those variants live in the host loop below
        const bool sharded = c->trk_world > 1 && c->trk_hook;          // the persistent kernel cannot exchange sums with other GPUs: a sharded tracker runs the host-driven loop
        const bool force_host = sharded || c->lm_host_only || c->set.affineOptModeA < 0 || c->set.affineOptModeB < 0;
        const int stop = 0;                                            // levels coarsestLvl..0 on the device
        if (!force_host) {
            if (c->slot_ref < 0 || slot_new < 0 || slot_new >= (int)c->slots.size() || !c->slots[slot_new].valid)
                return fail(c, NALO_ERR_STATE, "nalo_trk_track: no reference / empty frame slot");
            double o[32];
            int rc = trk_lm_launch(c, slot_new, T_io, aff_io, ref_aff, exposures, coarsestLvl, stop, minResForAbort, o);
            if (rc == NALO_LM_LOST_BLOCK) {
                // the persistent kernel's workgroups were not co-resident (another context holds the CUs): nothing was written back, so the frame is
                // redone by the host-driven loop below (same kernels per evaluation, same results to 1e-5), and so is every later frame of this context
                c->lm_host_only = true;
                for (int& e : c->lm_evals_lvl) e = 0;
                std::fprintf(stderr, "[nalo] trk_lm_kernel: a workgroup's partial never arrived; this context now drives the tracker's LM loop from the host\n");
            } else {
            if (rc) return rc;
            for (int l = stop; l <= coarsestLvl && l < 5; ++l) lastRes[l] = o[14 + l];
            flow[0] = o[19]; flow[1] = o[20]; flow[2] = o[21];
            evals = (int)o[23];
            if ((int)o[22] == 0) {                                          // aborted on minResForAbort (:1227): outputs untouched
                if (lastResiduals) std::memcpy(lastResiduals, lastRes, sizeof(lastRes));
                if (lastFlow) std::memcpy(lastFlow, flow, sizeof(flow));
                if (n_evals) *n_evals = evals;
                *ok = 0;
                return NALO_OK;
            }
            cur = SE3::from(o); aff_cur[0] = o[12]; aff_cur[1] = o[13];
            haveRepeated = o[25] != 0.0;
            start_lvl = (int)o[24];                                         // next level to process (-1: pyramid finished)
            }
        }
    }
    static const int maxIterations[5] = {10, 20, 50, 50, 50};
    const float lambdaExtrapolationLimit = 0.001f;
    auto eval = [&](int lvl, const SE3& T, const double aff[2], float cutoff, double st[6], double* H, double* b, double* aLL0) -> int {
        double aLL[2];
        aff_from_to(exposures[0], exposures[1], ref_aff[0], ref_aff[1], aff[0], aff[1], aLL);
        const float aLLf[2] = {(float)aLL[0], (float)aLL[1]};
        const double R[9] = {T.R(0, 0), T.R(0, 1), T.R(0, 2), T.R(1, 0), T.R(1, 1), T.R(1, 2), T.R(2, 0), T.R(2, 1), T.R(2, 2)};
        const double tt[3] = {T.t(0), T.t(1), T.t(2)};
        if (aLL0) *aLL0 = aLL[0];
        ++evals; ++c->lm_evals_lvl[lvl];
        return nalo_trk_eval(c, slot_new, lvl, R, tt, aLLf, (float)ref_aff[1], cutoff, 1, st, H, b);
    };
    if (start_lvl >= 0) {                                                     // the host-driven loop runs the frame: no persistent launch to describe
        for (int& v : c->trk_cfg) v = 0;
        c->trk_cfg[2] = 2;
    }
    for (int lvl = start_lvl; lvl >= 0; --lvl) {
        double H[64], b[8], Hn[64], bn[8], resOld[6], resNew[6];
        float levelCutoffRepeat = 1;
        int rc = eval(lvl, cur, aff_cur, kCoarseCutoffTH * levelCutoffRepeat, resOld, H, b, nullptr);
        if (rc) return rc;
        while (resOld[5] > 0.6 && levelCutoffRepeat < 50) {
            levelCutoffRepeat *= 2;
            rc = eval(lvl, cur, aff_cur, kCoarseCutoffTH * levelCutoffRepeat, resOld, H, b, nullptr);
            if (rc) return rc;
        }
        float lambda = 0.01f;
        for (int it = 0; it < maxIterations[lvl]; ++it) {
            double Hl[64], nb[8], inc[8];
            std::memcpy(Hl, H, sizeof(Hl));
            for (int i = 0; i < 8; ++i) { Hl[i * 8 + i] *= (1 + lambda); nb[i] = -b[i]; }
            ldlt_solve(8, Hl, nb, inc);
            {                                                                  // :1140-1162: a and/or b fixed
                const bool fa = c->set.affineOptModeA < 0, fb = c->set.affineOptModeB < 0;
                if (fa && fb) { double H6[36], x6[6]; for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) H6[i * 6 + j] = Hl[i * 8 + j];
                    ldlt_solve(6, H6, nb, x6); for (int i = 0; i < 6; ++i) inc[i] = x6[i]; inc[6] = inc[7] = 0; }
                if (!fa && fb) { double H7[49], x7[7]; for (int i = 0; i < 7; ++i) for (int j = 0; j < 7; ++j) H7[i * 7 + j] = Hl[i * 8 + j];
                    ldlt_solve(7, H7, nb, x7); for (int i = 0; i < 7; ++i) inc[i] = x7[i]; inc[7] = 0; }
                if (fa && !fb) {                                               // b takes a's slot: column 6 = column 7, then row 6 = row 7
                    double Hs[64], bs[8], H7[49], x7[7]; std::memcpy(Hs, Hl, sizeof(Hs)); std::memcpy(bs, nb, sizeof(bs));
                    for (int i = 0; i < 8; ++i) Hs[i * 8 + 6] = Hs[i * 8 + 7];
                    for (int j = 0; j < 8; ++j) Hs[6 * 8 + j] = Hs[7 * 8 + j];
                    bs[6] = bs[7];
                    for (int i = 0; i < 7; ++i) for (int j = 0; j < 7; ++j) H7[i * 7 + j] = Hs[i * 8 + j];
                    ldlt_solve(7, H7, bs, x7); for (int i = 0; i < 6; ++i) inc[i] = x7[i]; inc[6] = 0; inc[7] = x7[6];
                }
            }
            float extrapFac = 1;
            if (lambda < lambdaExtrapolationLimit) extrapFac = std::sqrt(std::sqrt(lambdaExtrapolationLimit / lambda));
            for (double& v : inc) v *= extrapFac;
            double incS[8];
            std::memcpy(incS, inc, sizeof(incS));
            for (int i = 0; i < 3; ++i) incS[i] *= kScaleXiRot;      // labels swapped vs. tangent order in the reference (:1172-1173)
            for (int i = 3; i < 6; ++i) incS[i] *= kScaleXiTrans;
            incS[6] *= kScaleA; incS[7] *= kScaleB;
            double s = 0; for (double v : incS) s += v;
            if (!std::isfinite(s)) std::memset(incS, 0, sizeof(incS));
            const SE3 Tn = se3_exp(incS) * cur;
            const double aff_new[2] = {aff_cur[0] + incS[6], aff_cur[1] + incS[7]};
            rc = eval(lvl, Tn, aff_new, kCoarseCutoffTH * levelCutoffRepeat, resNew, Hn, bn, nullptr);
            if (rc) return rc;
            const bool accept = (resNew[0] / resNew[1]) < (resOld[0] / resOld[1]);
            if (accept) {
                std::memcpy(H, Hn, sizeof(H)); std::memcpy(b, bn, sizeof(b)); std::memcpy(resOld, resNew, sizeof(resOld));
                aff_cur[0] = aff_new[0]; aff_cur[1] = aff_new[1]; cur = Tn;
                lambda *= 0.5f;
            } else { lambda *= 4; if (lambda < lambdaExtrapolationLimit) lambda = lambdaExtrapolationLimit; }
            double nrm = 0; for (double v : inc) nrm += v * v;
            if (!(std::sqrt(nrm) > 1e-3)) break;
        }
        lastRes[lvl] = std::sqrt((float)(resOld[0] / resOld[1]));
        flow[0] = resOld[2]; flow[1] = resOld[3]; flow[2] = resOld[4];
        if (minResForAbort && lastRes[lvl] > 1.5 * minResForAbort[lvl]) { good = false; break; }
        if (levelCutoffRepeat > 1 && !haveRepeated) { lvl++; haveRepeated = true; }
    }
    if (start_lvl >= 0) c->trk_cfg[8] = haveRepeated;
    if (lastResiduals) std::memcpy(lastResiduals, lastRes, sizeof(lastRes));
    if (lastFlow) std::memcpy(lastFlow, flow, sizeof(flow));
    if (n_evals) *n_evals = evals;
    if (!good) { *ok = 0; return NALO_OK; }
    std::memcpy(T_io, cur.m, sizeof(cur.m)); aff_io[0] = aff_cur[0]; aff_io[1] = aff_cur[1];
    {                                                                          // :1243-1256
        const double mA = c->set.affineOptModeA, mB = c->set.affineOptModeB;
        bool fine = !((mA != 0 && std::fabs((float)aff_io[0]) > 1.2f) || (mB != 0 && std::fabs((float)aff_io[1]) > 200.f));
        double rel[2]; aff_from_to(exposures[0], exposures[1], ref_aff[0], ref_aff[1], aff_io[0], aff_io[1], rel);
        if ((mA == 0 && std::fabs(logf((float)rel[0])) > 1.5f) || (mB == 0 && std::fabs((float)rel[1]) > 200.f)) fine = false;
        if (fine) { if (mA < 0) aff_io[0] = 0; if (mB < 0) aff_io[1] = 0; }
        *ok = fine;
    }
    return NALO_OK;
}

// FullSystem::trackNewCoarse's loop (FullSystem.cpp:595-666), see include/nalo_gpu.h. Everything is computed into locals and reaches the caller's struct only
// when the call succeeds.
namespace {
struct TriesResult {
    double T[12], aff[2], flow[3], ach[5];
    int have, run, winner, driver;
    std::vector<nalo_trk_try_record> rec;
};
// the literal loop over nalo_trk_track: the definition of the call, and its host-driven driver
int tries_host_loop(nalo_ctx* c, const nalo_trk_tries_args* a, double thr, TriesResult& r) {
    for (double& v : r.ach) v = NAN;
    std::memcpy(r.T, a->tries, sizeof(r.T)); r.aff[0] = a->aff_init[0]; r.aff[1] = a->aff_init[1];
    r.flow[0] = r.flow[1] = r.flow[2] = 0;
    r.have = 0; r.run = 0; r.winner = -1; r.driver = 2; r.rec.clear();
    int evl[5] = {};
    for (int i = 0; i < a->n_tries; ++i) {
        nalo_trk_try_record q = {};
        std::memcpy(q.T, a->tries + 12 * (size_t)i, sizeof(q.T)); q.aff[0] = a->aff_init[0]; q.aff[1] = a->aff_init[1];
        const int rc = nalo_trk_track(c, a->slot_new, q.T, q.aff, a->ref_aff, a->exposures, a->coarsestLvl, r.ach, q.lastResiduals, q.flow, &q.ok, &q.n_evals);
        if (rc) return rc;
        q.abort_lvl = -1;                                                           // the first level of the descent that fails :1227 is where it stopped
        if (!q.ok) for (int l = a->coarsestLvl; l >= 0; --l) if (q.lastResiduals[l] > 1.5 * r.ach[l]) { q.abort_lvl = l; break; }
        q.have_repeated = c->trk_cfg[8];
        for (int l = 0; l < 5; ++l) { q.evals[l] = c->lm_evals_lvl[l]; evl[l] += q.evals[l]; }
        q.taken = q.ok && std::isfinite((float)q.lastResiduals[0]) && !(q.lastResiduals[0] >= r.ach[0]);      // :633
        if (q.taken) { std::memcpy(r.T, q.T, sizeof(r.T)); r.aff[0] = q.aff[0]; r.aff[1] = q.aff[1]; std::memcpy(r.flow, q.flow, sizeof(r.flow)); r.have = 1; r.winner = i; }
        if (r.have) for (int l = 0; l < 5; ++l) if (!std::isfinite((float)r.ach[l]) || r.ach[l] > q.lastResiduals[l]) r.ach[l] = q.lastResiduals[l];   // :643-650
        r.rec.push_back(q);
        r.run = i + 1;
        if (r.have && r.ach[0] < thr) break;                                        // :653
    }
    for (int l = 0; l < 5; ++l) c->lm_evals_lvl[l] = evl[l];
    return NALO_OK;
}
}  // namespace

int nalo_trk_track_tries(nalo_ctx* c, nalo_trk_tries_args* a) {
    if (!c || !a || !a->tries) return fail(c, NALO_ERR_ARG, "nalo_trk_track_tries: bad argument");
    if (a->n_tries < 1 || a->n_tries > NALO_TRK_MAX_TRIES) return fail(c, NALO_ERR_ARG, "nalo_trk_track_tries: n_tries outside 1 .. NALO_TRK_MAX_TRIES (an empty list: pass one identity)");
    if (a->records_cap < 0 || (a->records_cap > 0 && !a->records)) return fail(c, NALO_ERR_ARG, "nalo_trk_track_tries: records_cap without records");
    if (!(a->coarsestLvl >= 0 && a->coarsestLvl < 5 && a->coarsestLvl < c->levels)) return fail(c, NALO_ERR_ARG, "nalo_trk_track_tries: coarsestLvl out of range");
    if (a->slot_new < 0 || a->slot_new >= (int)c->slots.size()) return fail(c, NALO_ERR_ARG, "nalo_trk_track_tries: frame slot out of range");
    for (size_t i = 0; i < 12 * (size_t)a->n_tries; ++i) if (!std::isfinite(a->tries[i])) return fail(c, NALO_ERR_ARG, "nalo_trk_track_tries: a try is not finite");
    if (c->slot_ref < 0 || !c->slots[a->slot_new].valid) return fail(c, NALO_ERR_STATE, "nalo_trk_track_tries: no reference (nalo_trk_set_ref) / empty frame slot");
    if (c->xchg_failed) return fail(c, NALO_ERR_HIP, "nalo_trk_track_tries: a cross-rank sum of this context failed earlier; rebuild on a new context");
    // ---- accepted
    HostTimer ht(c, "trk_track_tries");
    const float rt = a->reTrackThreshold > 0 ? (float)a->reTrackThreshold : kReTrackThreshold;
    const double thr = a->lastCoarseRMSE_io[0] * (double)rt;
    TriesResult r;
    const bool sharded = c->trk_world > 1 && c->trk_hook;
    bool host = sharded || c->lm_host_only || c->set.affineOptModeA < 0 || c->set.affineOptModeB < 0;
    if (!host) {
        double sum[32];
        std::vector<double> recs((size_t)a->n_tries * kLmRecDoubles);
        const int rc = trk_lm_tries_launch(c, a->slot_new, a->tries, a->n_tries, a->aff_init, a->ref_aff, a->exposures, a->coarsestLvl, thr, sum, recs.data());
        if (rc == NALO_LM_LOST_BLOCK) {                                             // as nalo_trk_track: nothing of the launch is used, the whole list is redone below
            c->lm_host_only = true; host = true;
            std::fprintf(stderr, "[nalo] trk_lm_kernel: a workgroup's partial never arrived; this context now drives the tracker's LM loop from the host\n");
        } else {
            if (rc) return rc;
            std::memcpy(r.T, sum, sizeof(r.T)); r.aff[0] = sum[12]; r.aff[1] = sum[13];
            for (int l = 0; l < 5; ++l) r.ach[l] = sum[14 + l];
            for (int k = 0; k < 3; ++k) r.flow[k] = sum[19 + k];
            r.have = (int)sum[23]; r.run = (int)sum[24]; r.winner = (int)sum[25]; r.driver = 1;
            r.rec.resize((size_t)r.run);
            for (int i = 0; i < r.run; ++i) {
                const double* s = recs.data() + (size_t)i * kLmRecDoubles;
                nalo_trk_try_record& q = r.rec[i];
                q.ok = (int)s[0]; q.taken = (int)s[1]; q.abort_lvl = (int)s[2]; q.have_repeated = (int)s[3]; q.n_evals = (int)s[4];
                std::memcpy(q.lastResiduals, s + 5, sizeof(q.lastResiduals)); std::memcpy(q.flow, s + 10, sizeof(q.flow));
                std::memcpy(q.T, s + 13, sizeof(q.T)); q.aff[0] = s[25]; q.aff[1] = s[26];
                for (int l = 0; l < 5; ++l) q.evals[l] = (int)s[27 + l];
            }
        }
    }
    if (host) { const int rc = tries_host_loop(c, a, thr, r); if (rc) return rc; }
    std::memcpy(a->T, r.T, sizeof(r.T)); a->aff[0] = r.aff[0]; a->aff[1] = r.aff[1];
    std::memcpy(a->flow, r.flow, sizeof(r.flow)); std::memcpy(a->achievedRes, r.ach, sizeof(r.ach));
    std::memcpy(a->lastCoarseRMSE_io, r.ach, sizeof(r.ach));                        // :666, NaNs included
    a->have_one_good = r.have; a->try_iterations = r.run; a->winner = r.winner; a->driver = r.driver;
    for (int i = 0; i < r.run && i < a->records_cap; ++i) a->records[i] = r.rec[i];
    return NALO_OK;
}

// FullSystem.cpp:535-579. Host code, no context.
int nalo_trk_motion_tries(const double slast_2_sprelast[12], const double lastF_2_slast[12], int poses_valid, double out[31 * 12]) {
    if (!slast_2_sprelast || !lastF_2_slast || !out) return NALO_ERR_ARG;
    if (!poses_valid) { const SE3 I = SE3::identity(); std::memcpy(out, I.m, sizeof(I.m)); return 1; }
    const SE3 fh_2_slast = SE3::from(slast_2_sprelast), lastF = SE3::from(lastF_2_slast), inv = fh_2_slast.inverse();
    double xi[6];
    se3_log(fh_2_slast, xi);
    for (double& v : xi) v *= 0.5;
    const SE3 constant = inv * lastF;
    const SE3 first[5] = {constant, inv * inv * lastF, se3_exp(xi).inverse() * lastF, lastF, SE3::identity()};
    int n = 0;
    for (const SE3& s : first) std::memcpy(out + 12 * n++, s.m, sizeof(s.m));
    const double d = (double)0.02f;                                                // `float rotDelta = 0.02`
    static const signed char sg[26][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}, {-1, 1, 0}, {0, -1, 1}, {-1, 0, 1},
                                          {1, -1, 0}, {0, 1, -1}, {1, 0, -1}, {-1, -1, 0}, {0, -1, -1}, {-1, 0, -1}, {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1},
                                          {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
    for (const auto& s3 : sg) {
        double q[4] = {1.0, s3[0] * d, s3[1] * d, s3[2] * d};                       // (w, x, y, z); SO3's constructor normalises
        const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (double& v : q) v /= qn;
        const double w = q[0], x = q[1], y = q[2], z = q[3];
        SE3 Rq = SE3::identity();
        const double Rm[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                              2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rq.m[i * 4 + j] = Rm[i * 3 + j];
        const SE3 t = constant * Rq;
        std::memcpy(out + 12 * n++, t.m, sizeof(t.m));
    }
    return n;
}

// ------------------------------------------------------------------------------------------------ immature points
int nalo_imm_create(nalo_ctx* c, int slot_host, int n, const int* u, const int* v, float* color, float* weights, float* gradH, float* energyTH) {
    if (!c || n < 0 || (n > 0 && (!u || !v || !color || !weights || !gradH || !energyTH))) return fail(c, NALO_ERR_ARG, "nalo_imm_create: bad argument");
    if (slot_host < 0 || slot_host >= (int)c->slots.size() || !c->slots[slot_host].valid) return fail(c, NALO_ERR_STATE, "nalo_imm_create: host slot has no pyramid");
    if (n == 0) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    for (int i = 0; i < n; ++i) if (u[i] < 2 || v[i] < 2 || u[i] >= c->w - 3 || v[i] >= c->h - 3) return fail(c, NALO_ERR_ARG, "nalo_imm_create: pattern leaves the image");
    // words: u(n) v(n) | color(8n) weights(8n) gradH(3n) energyTH(n)
    const size_t N = (size_t)n;
    int rc = imm_stage(c, 22 * N); if (rc) return rc;
    float* hst = c->imm_host.p;
    std::memcpy(hst, u, N * 4); std::memcpy(hst + N, v, N * 4);
    float* d = c->imm_dev.p;
    NALO_HIP(c, hipMemcpyAsync(d, hst, 2 * N * 4, hipMemcpyHostToDevice, c->stream));
    rc = imm_create_launch(c, c->slots[slot_host].dI[0].p, n, (const int*)d, (const int*)(d + N), d + 2 * N, d + 10 * N, d + 18 * N, d + 21 * N);
    if (rc) return rc;
    NALO_HIP(c, hipMemcpyAsync(hst + 2 * N, d + 2 * N, 20 * N * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(color, hst + 2 * N, 8 * N * 4); std::memcpy(weights, hst + 10 * N, 8 * N * 4);
    std::memcpy(gradH, hst + 18 * N, 3 * N * 4); std::memcpy(energyTH, hst + 21 * N, N * 4);
    return NALO_OK;
}

int nalo_imm_trace(nalo_ctx* c, int slot_new, int n, const float* u, const float* v, const float* color, const float* weights, const float* gradH,
                   const float* energyTH, const int* host_idx, int nh, const float* KRKi, const float* Kt, const float* aff,
                   float* idepth_min, float* idepth_max, int* status, float* quality, float* lastTraceUV, float* lastTracePixelInterval) {
    if (!c || n < 0 || nh < 0 || (n > 0 && (!u || !v || !color || !weights || !gradH || !energyTH || !host_idx || !KRKi || !Kt || !aff || !idepth_min || !idepth_max ||
                                             !status || !quality || !lastTraceUV || !lastTracePixelInterval)))
        return fail(c, NALO_ERR_ARG, "nalo_imm_trace: bad argument");
    if (slot_new < 0 || slot_new >= (int)c->slots.size() || !c->slots[slot_new].valid) return fail(c, NALO_ERR_STATE, "nalo_imm_trace: frame slot has no pyramid");
    if (n == 0) return NALO_OK;
    for (int i = 0; i < n; ++i) if (host_idx[i] < 0 || host_idx[i] >= nh) return fail(c, NALO_ERR_ARG, "nalo_imm_trace: host_idx out of range");
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "imm_trace");
    // words: [0,22n) u v color weights gradH energyTH | [22n,23n) host_idx | [23n,30n) idmin idmax status quality lastUV(2) lastInterval | [30n, +14nh) KRKi Kt aff
    const size_t N = (size_t)n, H = (size_t)nh;
    int rc = imm_stage(c, 30 * N + 14 * H); if (rc) return rc;
    float* hst = c->imm_host.p;
    std::memcpy(hst, u, N * 4); std::memcpy(hst + N, v, N * 4); std::memcpy(hst + 2 * N, color, 8 * N * 4); std::memcpy(hst + 10 * N, weights, 8 * N * 4);
    std::memcpy(hst + 18 * N, gradH, 3 * N * 4); std::memcpy(hst + 21 * N, energyTH, N * 4); std::memcpy(hst + 22 * N, host_idx, N * 4);
    std::memcpy(hst + 23 * N, idepth_min, N * 4); std::memcpy(hst + 24 * N, idepth_max, N * 4); std::memcpy(hst + 25 * N, status, N * 4); std::memcpy(hst + 26 * N, quality, N * 4);
    std::memcpy(hst + 27 * N, lastTraceUV, 2 * N * 4); std::memcpy(hst + 29 * N, lastTracePixelInterval, N * 4);     // untouched entries keep the caller's values
    std::memcpy(hst + 30 * N, KRKi, 9 * H * 4); std::memcpy(hst + 30 * N + 9 * H, Kt, 3 * H * 4); std::memcpy(hst + 30 * N + 12 * H, aff, 2 * H * 4);
    float* d = c->imm_dev.p;
    NALO_HIP(c, hipMemcpyAsync(d, hst, (30 * N + 14 * H) * 4, hipMemcpyHostToDevice, c->stream));
    rc = imm_trace_launch(c, c->slots[slot_new].dI[0].p, n, d, (const int*)(d + 22 * N), d + 30 * N, d + 30 * N + 9 * H, d + 30 * N + 12 * H,
                          d + 23 * N, d + 24 * N, (int*)(d + 25 * N), d + 26 * N, d + 27 * N, d + 29 * N);
    if (rc) return rc;
    NALO_HIP(c, hipMemcpyAsync(hst + 23 * N, d + 23 * N, 7 * N * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(idepth_min, hst + 23 * N, N * 4); std::memcpy(idepth_max, hst + 24 * N, N * 4); std::memcpy(status, hst + 25 * N, N * 4); std::memcpy(quality, hst + 26 * N, N * 4);
    std::memcpy(lastTraceUV, hst + 27 * N, 2 * N * 4); std::memcpy(lastTracePixelInterval, hst + 29 * N, N * 4);
    return NALO_OK;
}

// Device-resident immature points: the set is uploaded when it changes (makeNewTraces / activation, once per keyframe), every new frame then only sends
// its 14 floats per host frame and the trace updates the state in place; the state comes back when the host wants it (activatePointsMT).
int nalo_imm_resident_set(nalo_ctx* c, int n, const float* u, const float* v, const float* color, const float* weights, const float* gradH, const float* energyTH,
                          const int* host_idx, const float* idepth_min, const float* idepth_max, const int* status, const float* quality) {
    if (!c || n < 0 || (n > 0 && (!u || !v || !color || !weights || !gradH || !energyTH || !host_idx || !idepth_min || !idepth_max || !status || !quality)))
        return fail(c, NALO_ERR_ARG, "nalo_imm_resident_set: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    c->imm_res_n = n; c->imm_res_maxhost = -1; c->imm_type_set = false;
    c->act_pend_n = -1;                                                       // an activation result names points of the set it was made on
    c->imm_carry_have = false;                                                // and so does the map of the last nalo_imm_resident_carry
    c->imm_uv_h.clear(); c->imm_host_h.clear();
    if (n == 0) return NALO_OK;
    const size_t N = (size_t)n;
    c->imm_uv_h.assign(u, u + N); c->imm_uv_h.insert(c->imm_uv_h.end(), v, v + N); c->imm_host_h.assign(host_idx, host_idx + N);   // nalo_ba_carry_window's slot order of an inserted point
    int rc = imm_stage(c, 30 * N); if (rc) return rc;
    NALO_HIP(c, c->imm_res.reserve(30 * N + 256));
    float* hst = c->imm_host.p;
    for (int i = 0; i < n; ++i) { if (host_idx[i] < 0) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_set: negative host_idx"); c->imm_res_maxhost = std::max(c->imm_res_maxhost, host_idx[i]); }
    std::memcpy(hst, u, N * 4); std::memcpy(hst + N, v, N * 4); std::memcpy(hst + 2 * N, color, 8 * N * 4); std::memcpy(hst + 10 * N, weights, 8 * N * 4);
    std::memcpy(hst + 18 * N, gradH, 3 * N * 4); std::memcpy(hst + 21 * N, energyTH, N * 4); std::memcpy(hst + 22 * N, host_idx, N * 4);
    std::memcpy(hst + 23 * N, idepth_min, N * 4); std::memcpy(hst + 24 * N, idepth_max, N * 4); std::memcpy(hst + 25 * N, status, N * 4); std::memcpy(hst + 26 * N, quality, N * 4);
    for (size_t i = 0; i < 2 * N; ++i) hst[27 * N + i] = -1.f;                // ImmaturePoint ctor: lastTraceUV = (-1,-1), lastTracePixelInterval = 0
    std::memset(hst + 29 * N, 0, N * 4);
    NALO_HIP(c, hipMemcpyAsync(c->imm_res.p, hst, 30 * N * 4, hipMemcpyHostToDevice, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));                             // the staging buffer is shared with the other immature-point calls
    return NALO_OK;
}
// ImmaturePoint::my_type of every resident point (the selector's status 1 / 2 / 4, PixelSelector2.h:36): activation's threshold is currentMinActDist * my_type
int nalo_imm_resident_set_type(nalo_ctx* c, const float* my_type) {
    if (!c || (c->imm_res_n > 0 && !my_type)) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_set_type: bad argument");
    const size_t N = (size_t)c->imm_res_n;
    float mx = 0;
    for (size_t i = 0; i < N; ++i) { if (!std::isfinite(my_type[i])) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_set_type: my_type is not finite"); mx = std::max(mx, my_type[i]); }
    c->imm_type_set = false; c->imm_type_max = mx;
    if (N == 0) { c->imm_type_set = true; return NALO_OK; }
    NALO_HIP(c, hipSetDevice(c->device));
    int rc = imm_stage(c, N); if (rc) return rc;
    NALO_HIP(c, c->imm_type.reserve(N));
    std::memcpy(c->imm_host.p, my_type, N * 4);
    NALO_HIP(c, hipMemcpyAsync(c->imm_type.p, c->imm_host.p, N * 4, hipMemcpyHostToDevice, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));                             // the staging buffer is shared with the other immature-point calls
    c->imm_type_set = true;
    return NALO_OK;
}
int nalo_imm_activate_last(nalo_ctx* c, int stats[4]) {
    if (!c || !stats) return fail(c, NALO_ERR_ARG, "nalo_imm_activate_last: bad argument");
    std::memcpy(stats, c->imm_act_stats, sizeof(c->imm_act_stats));
    return NALO_OK;
}
int nalo_imm_resident_trace(nalo_ctx* c, int slot_new, int nh, const float* KRKi, const float* Kt, const float* aff) {
    if (!c || nh < 1 || nh > 16 || !KRKi || !Kt || !aff) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_trace: bad argument");
    if (slot_new < 0 || slot_new >= (int)c->slots.size() || !c->slots[slot_new].valid) return fail(c, NALO_ERR_STATE, "nalo_imm_resident_trace: frame slot has no pyramid");
    if (c->imm_res_n == 0) return NALO_OK;
    if (c->imm_res_maxhost >= nh) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_trace: a resident point's host_idx is out of range");
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "imm_resident_trace");
    const size_t N = (size_t)c->imm_res_n, H = (size_t)nh;
    float hk[224];
    std::memcpy(hk, KRKi, 9 * H * 4); std::memcpy(hk + 9 * H, Kt, 3 * H * 4); std::memcpy(hk + 12 * H, aff, 2 * H * 4);
    float* d = c->imm_res.p;
    int rc = imm_put_launch(c, d + 30 * N, hk, (int)(14 * H)); if (rc) return rc;
    return imm_trace_launch(c, c->slots[slot_new].dI[0].p, c->imm_res_n, d, (const int*)(d + 22 * N), d + 30 * N, d + 30 * N + 9 * H, d + 30 * N + 12 * H,
                            d + 23 * N, d + 24 * N, (int*)(d + 25 * N), d + 26 * N, d + 27 * N, d + 29 * N);
}
int nalo_imm_resident_get(nalo_ctx* c, float* idepth_min, float* idepth_max, int* status, float* quality, float* lastTraceUV, float* lastTracePixelInterval) {
    if (!c) return NALO_ERR_ARG;
    if (c->imm_res_n == 0) return NALO_OK;
    if (!idepth_min || !idepth_max || !status || !quality) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_get: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->imm_res_n;
    int rc = imm_stage(c, 7 * N); if (rc) return rc;
    float* hst = c->imm_host.p;
    NALO_HIP(c, hipMemcpyAsync(hst, c->imm_res.p + 23 * N, 7 * N * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(idepth_min, hst, N * 4); std::memcpy(idepth_max, hst + N, N * 4); std::memcpy(status, hst + 2 * N, N * 4); std::memcpy(quality, hst + 3 * N, N * 4);
    if (lastTraceUV) std::memcpy(lastTraceUV, hst + 4 * N, 2 * N * 4);
    if (lastTracePixelInterval) std::memcpy(lastTracePixelInterval, hst + 6 * N, N * 4);
    return NALO_OK;
}

// The resident set across a keyframe (include/nalo_gpu.h has the semantics; kernels_imm_carry.hip the device side). Everything resident is read on the device:
// a byte per old point (what (A) decides without the device's status), the host map and an explicit append list go down, the 4-byte map and the counts come up,
// behind ONE wait. The new set is written into a second buffer that then changes places with the first, so a refusal leaves the set as it was.
int nalo_imm_resident_carry(nalo_ctx* c, const nalo_imm_carry_args* a) {
    if (!c || !a) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: bad argument");
    const int n = c->imm_res_n;
    const size_t N = (size_t)n;
    if (n > 0 && (c->imm_host_h.size() != N || c->imm_uv_h.size() != 2 * N)) return fail(c, NALO_ERR_STATE, "nalo_imm_resident_carry: the resident set has no host copy");
    // ---- (C)
    int H = std::max(c->imm_res_maxhost + 1, 1), hmap[NALO_MAX_WINDOW];
    for (int h = 0; h < NALO_MAX_WINDOW; ++h) hmap[h] = h;
    if (a->host_map) {
        if (a->n_hosts_old < 0 || a->n_hosts_old > NALO_MAX_WINDOW) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: n_hosts_old outside [0, NALO_MAX_WINDOW]");
        int next = 0;
        for (int h = 0; h < a->n_hosts_old; ++h) {
            if (a->host_map[h] != -1 && a->host_map[h] != next) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: host_map's kept entries must be 0, 1, ... in increasing order");
            if (a->host_map[h] != -1) ++next;
            hmap[h] = a->host_map[h];
        }
        if (c->imm_res_maxhost >= a->n_hosts_old) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: a resident point's host_idx is outside host_map");
        H = std::max(a->n_hosts_old, 1);
        if (a->n_hosts_old == 0) hmap[0] = -1;
    }
    // ---- (B)
    const bool app = a->append_slot >= 0;
    if (app && n > 0 && !c->imm_type_set) return fail(c, NALO_ERR_STATE, "nalo_imm_resident_carry: the resident set has no types (nalo_imm_resident_set_type) and the appended points would bring theirs");
    const int *list_dev = nullptr, *list_live = nullptr;
    int m = 0, m_up = 0, n_live = 0;
    if (app) {
        if (a->append_host < 0 || a->append_host >= NALO_MAX_WINDOW) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: append_host outside the window");
        if (a->append_slot >= (int)c->slots.size() || !c->slots[a->append_slot].valid) return fail(c, NALO_ERR_STATE, "nalo_imm_resident_carry: the append slot has no pyramid");
        if (a->append_idx) {
            if (a->append_n < 0 || (a->append_n > 0 && !a->append_status)) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: bad append list");
            for (int k = 0; k < a->append_n; ++k) {
                if (a->append_idx[k] < 0 || a->append_idx[k] >= c->w * c->h || a->append_status[k] > 15) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: an append entry is outside the image or its status above 15");
                if (k > 0 && a->append_idx[k] <= a->append_idx[k - 1]) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: the append list must be in raster order, every pixel once (makeNewTraces walks the map)");
            }
            m = m_up = a->append_n;
        } else if (!pixsel_last_list(c, a->append_slot, &list_dev, &m, &list_live, &n_live))
            return fail(c, NALO_ERR_STATE, "nalo_imm_resident_carry: no selection map has been made on the append slot (nalo_pixsel_make_maps)");
    }
    if ((size_t)n + (size_t)m >= (size_t)0x3FFFFFFF) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: too many points");
    // ---- (A): what the host can decide per point. 0 stays, 1 deleted, 2 deleted when the resident status is IPS_OOB (FullSystem.cpp:908)
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "imm_resident_carry");
    const size_t code_w = a->fate ? (N + 3) / 4 : 0, up_w = 16 + (size_t)m_up + code_w, down_w = 32 + N + (size_t)m;
    int rc = imm_stage(c, up_w + down_w); if (rc) return rc;
    int* hst = reinterpret_cast<int*>(c->imm_host.p);
    static_assert(NALO_MAX_WINDOW <= 16 && 4 + NALO_MAX_WINDOW <= 32, "the staging block keeps 16 words for the host map and 32 for the counts");
    std::memcpy(hst, hmap, sizeof(hmap));
    for (int k = 0; k < m_up; ++k) hst[16 + k] = a->append_idx[k] | ((int)a->append_status[k] << 28);
    if (a->fate) {
        if (a->n_sel < 0 || (a->n_sel > 0 && (!a->sel || !a->result))) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: sel and result are required with n_sel > 0");
        uint8_t* code = reinterpret_cast<uint8_t*>(hst + 16 + m_up);
        int n1 = 0;
        for (int i = 0; i < n; ++i) {
            const int f = a->fate[i];
            if (f < -3 || f > 3) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: a fate outside [-3, 3]");
            code[i] = f < 0 ? 1 : (f == 1 ? 255 : 0);                           // 255: selected, waits for its verdict
            n1 += f == 1;
        }
        if (n1 != a->n_sel) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: sel must list exactly the points with fate 1");
        for (int k = 0; k < a->n_sel; ++k) {
            const int i = a->sel[k], r = a->result[k];
            if (i < 0 || i >= n || code[i] != 255) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: sel must list exactly the points with fate 1");
            if (r != 1 && r != 0 && r != -1) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry: a result outside {1, 0, -1}");
            code[i] = r == 0 ? 2 : 1;                                           // :898-907 became a PointHessian, :908 optimizeImmaturePoint's -1: both leave the set
        }
    }
    const int n_slots = n + m;
    int st[4 + NALO_MAX_WINDOW] = {};
    std::vector<int> map;
    if (n_slots > 0) {
        const size_t grow = (size_t)n_slots + n_slots / 2 + 1024;               // room for the sets of the next keyframes: nothing is allocated in steady state
        if (c->imm_res2.cap < 30 * (size_t)n_slots + 256) NALO_HIP(c, c->imm_res2.reserve(30 * grow + 256));
        if (c->imm_type2.cap < (size_t)n_slots) NALO_HIP(c, c->imm_type2.reserve(grow));
        ImmCarryParams P;
        std::memset(&P, 0, sizeof(P));
        P.n = n; P.nb = (n + 255) / 256; P.m = m; P.mb = (m + 255) / 256; P.H = H;
        P.w = c->w; P.h = c->h; P.append_host = app ? a->append_host : -1; P.rank_live = app && !a->append_idx;
        const size_t cnt_w = 2 * (size_t)H * P.nb + 2 * (size_t)P.mb + P.nb + 1, scr_w = cnt_w + 32 + (size_t)n_slots + N + (size_t)m;
        if (c->imm_carry_scr.cap < scr_w) NALO_HIP(c, c->imm_carry_scr.reserve(scr_w + scr_w / 2 + 1024));
        NALO_HIP(c, hipMemcpyAsync(c->imm_dev.p, hst, up_w * 4, hipMemcpyHostToDevice, c->stream));
        const int* dv = reinterpret_cast<const int*>(c->imm_dev.p);
        P.host_map = dv; P.list = a->append_idx ? dv + 16 : list_dev; P.code = a->fate ? reinterpret_cast<const uint8_t*>(dv + 16 + m_up) : nullptr;
        P.res = c->imm_res.p; P.type = (n > 0 && c->imm_type_set) ? c->imm_type.p : nullptr; P.res2 = c->imm_res2.p; P.type2 = c->imm_type2.p;
        P.dI = app ? c->slots[a->append_slot].dI[0].p : nullptr;
        P.cnt = c->imm_carry_scr.p; P.out = P.cnt + cnt_w; P.src = P.out + 32; P.mover = P.src + n_slots; P.arank = P.mover + n;
        rc = imm_carry_launch(c, P); if (rc) return rc;
        NALO_HIP(c, hipMemcpyAsync(hst + up_w, P.out, down_w * 4, hipMemcpyDeviceToHost, c->stream));
        NALO_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(st, hst + up_w, sizeof(st));
        if (st[0] < 0 || st[0] > n_slots) return fail(c, NALO_ERR_HIP, "nalo_imm_resident_carry: the device returned an impossible count");
        map.assign(hst + up_w + 32, hst + up_w + 32 + st[0]);
    }
    // ---- commit: the host copies nalo_ba_carry_window(insert_activated) orders inserted points by, then the buffers change places
    const int n_new = st[0];
    std::vector<float> uv(2 * (size_t)n_new); std::vector<int> hh((size_t)n_new);
    float tmax = (n > 0 && c->imm_type_set) ? c->imm_type_max : 0.f;
    for (int j = 0; j < n_new; ++j) {
        const int s = map[j];
        if (s >= 0) { uv[j] = c->imm_uv_h[s]; uv[(size_t)n_new + j] = c->imm_uv_h[N + s]; hh[j] = hmap[c->imm_host_h[s]]; continue; }
        const int k = -(s + 2);
        if (k < 0 || k >= (a->append_idx ? m : n_live)) return fail(c, NALO_ERR_HIP, "nalo_imm_resident_carry: the device named an append entry outside the list");
        const int e = a->append_idx ? (a->append_idx[k] | ((int)a->append_status[k] << 28)) : list_live[k], idx = e & 0x0FFFFFFF;
        uv[j] = (float)(idx % c->w); uv[(size_t)n_new + j] = (float)(idx / c->w); hh[j] = a->append_host;
        tmax = std::max(tmax, (float)((unsigned)e >> 28));
    }
    if (n_slots > 0) { std::swap(c->imm_res, c->imm_res2); std::swap(c->imm_type, c->imm_type2); }
    c->imm_uv_h.swap(uv); c->imm_host_h.swap(hh);
    c->imm_type_set = c->imm_type_set || n == 0;                              // carried points keep their types, appended ones bring theirs; a set without types stays without
    c->imm_type_max = tmax;                                                     // an upper bound: deleted points are not taken out of it
    c->imm_res_n = n_new; c->imm_res_maxhost = -1;
    for (int h = 0; h < NALO_MAX_WINDOW; ++h) if (st[4 + h] > 0) c->imm_res_maxhost = h;
    c->act_pend_n = -1;                                                       // an activation result names points of the set it was made on
    c->imm_carry_map.swap(map); std::memcpy(c->imm_carry_stats, st, sizeof(st)); c->imm_carry_have = true;
    return NALO_OK;
}
int nalo_imm_resident_carry_map(nalo_ctx* c, int* src) {
    if (!c || (c->imm_carry_have && !c->imm_carry_map.empty() && !src)) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry_map: bad argument");
    if (!c->imm_carry_have) return fail(c, NALO_ERR_STATE, "nalo_imm_resident_carry_map: the resident set does not come from nalo_imm_resident_carry");
    if (!c->imm_carry_map.empty()) std::memcpy(src, c->imm_carry_map.data(), c->imm_carry_map.size() * sizeof(int));
    return NALO_OK;
}
int nalo_imm_resident_carry_last(nalo_ctx* c, int stats[4 + NALO_MAX_WINDOW]) {
    if (!c || !stats) return fail(c, NALO_ERR_ARG, "nalo_imm_resident_carry_last: bad argument");
    if (!c->imm_carry_have) return fail(c, NALO_ERR_STATE, "nalo_imm_resident_carry_last: the resident set does not come from nalo_imm_resident_carry");
    std::memcpy(stats, c->imm_carry_stats, sizeof(c->imm_carry_stats));
    return NALO_OK;
}
int nalo_imm_resident_get_points(nalo_ctx* c, int* n, float* u, float* v, float* color, float* weights, float* gradH, float* energyTH, int* host_idx, float* my_type) {
    if (!c) return NALO_ERR_ARG;
    if (n) *n = c->imm_res_n;
    if (c->imm_res_n == 0 || !(u || v || color || weights || gradH || energyTH || host_idx || my_type)) return NALO_OK;
    if (my_type && !c->imm_type_set) return fail(c, NALO_ERR_STATE, "nalo_imm_resident_get_points: the resident set has no types (nalo_imm_resident_set_type)");
    NALO_HIP(c, hipSetDevice(c->device));
    const size_t N = (size_t)c->imm_res_n;
    int rc = imm_stage(c, 24 * N); if (rc) return rc;
    float* hst = c->imm_host.p;
    NALO_HIP(c, hipMemcpyAsync(hst, c->imm_res.p, 23 * N * 4, hipMemcpyDeviceToHost, c->stream));
    if (my_type) NALO_HIP(c, hipMemcpyAsync(hst + 23 * N, c->imm_type.p, N * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    if (u) std::memcpy(u, hst, N * 4);
    if (v) std::memcpy(v, hst + N, N * 4);
    if (color) std::memcpy(color, hst + 2 * N, 8 * N * 4);
    if (weights) std::memcpy(weights, hst + 10 * N, 8 * N * 4);
    if (gradH) std::memcpy(gradH, hst + 18 * N, 3 * N * 4);
    if (energyTH) std::memcpy(energyTH, hst + 21 * N, N * 4);
    if (host_idx) std::memcpy(host_idx, hst + 22 * N, N * 4);
    if (my_type) std::memcpy(my_type, hst + 23 * N, N * 4);
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ two-frame initialiser
int nalo_init_calc_res_and_gs(nalo_ctx* c, int slot_first, int slot_new, int lvl, int n, const float* u, const float* v, const float* idepth_new, const float* iR,
                              const uint8_t* isGood, const float* energy, const float* outlierTH, const double refToNew[12], const double aff[2],
                              float alphaW, float alphaK, float couplingWeight,
                              uint8_t* isGood_new, float* energy_new, float* maxstep, float* lastHessian_new, float* JbBuffer_new,
                              double* H_out, double* b_out, double* H_out_sc, double* b_out_sc, double E3[3]) {
    if (!c || n < 0 || !refToNew || !aff || !H_out || !b_out || !H_out_sc || !b_out_sc || !E3 ||
        (n > 0 && (!u || !v || !idepth_new || !iR || !isGood || !energy || !outlierTH || !isGood_new || !energy_new || !maxstep || !lastHessian_new || !JbBuffer_new)))
        return fail(c, NALO_ERR_ARG, "nalo_init_calc_res_and_gs: bad argument");
    if (lvl < 0 || lvl >= c->levels) return fail(c, NALO_ERR_ARG, "nalo_init_calc_res_and_gs: level out of range");
    for (int s : {slot_first, slot_new}) if (s < 0 || s >= (int)c->slots.size() || !c->slots[s].valid) return fail(c, NALO_ERR_STATE, "nalo_init_calc_res_and_gs: frame slot has no pyramid");
    NALO_HIP(c, hipSetDevice(c->device));
    const SE3 T = SE3::from(refToNew);
    InitParams P; InitPose X;
    init_pose_setup(c, lvl, n, T, aff, alphaW, alphaK, couplingWeight, P, X);
    double sums[96] = {};
    if (n > 0) {
        // words in: [u | v | idepth_new | iR | energy(2n) | outlierTH | isGood bytes]; out: [energy_new(2n) | maxstep | lastHessian_new | Jb(10n) | isGood_new bytes]; then 96 doubles
        const size_t N = (size_t)n, NB = (N + 3) / 4, in_w = 7 * N + NB, out_w = 14 * N + NB, tot = in_w + out_w + 2 * 96 + 2;
        int rc = imm_stage(c, tot); if (rc) return rc;
        float* hst = c->imm_host.p;
        std::memcpy(hst, u, N * 4); std::memcpy(hst + N, v, N * 4); std::memcpy(hst + 2 * N, idepth_new, N * 4); std::memcpy(hst + 3 * N, iR, N * 4);
        std::memcpy(hst + 4 * N, energy, 2 * N * 4); std::memcpy(hst + 6 * N, outlierTH, N * 4); std::memcpy(hst + 7 * N, isGood, N);
        float* ho = hst + in_w;
        std::memcpy(ho + 3 * N, lastHessian_new, N * 4); std::memcpy(ho + 4 * N, JbBuffer_new, 10 * N * 4);          // in/out members
        float* d = c->imm_dev.p;
        const size_t sums_off = (in_w + out_w + 1) & ~(size_t)1;                                                      // 8-byte aligned
        NALO_HIP(c, hipMemcpyAsync(d, hst, (in_w + out_w) * 4, hipMemcpyHostToDevice, c->stream));
        P.colorRef = c->slots[slot_first].dI[lvl].p; P.colorNew = c->slots[slot_new].dI[lvl].p;
        P.u = d; P.v = d + N; P.idepth = nullptr; P.idepth_new = d + 2 * N; P.iR = d + 3 * N; P.energy = d + 4 * N; P.outlierTH = d + 6 * N; P.isGood = (const uint8_t*)(d + 7 * N);
        float* outw = d + in_w;
        P.energy_new = outw; P.maxstep = outw + 2 * N; P.lastHessian_new = outw + 3 * N; P.Jb = outw + 4 * N; P.isGood_new = (uint8_t*)(outw + 14 * N);
        rc = init_calc_launch(c, P, lvl, (double*)(d + sums_off));
        if (rc) return rc;
        NALO_HIP(c, hipMemcpyAsync(ho, d + in_w, (sums_off - in_w + 2 * 96) * 4, hipMemcpyDeviceToHost, c->stream));
        NALO_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(energy_new, ho, 2 * N * 4); std::memcpy(maxstep, ho + 2 * N, N * 4); std::memcpy(lastHessian_new, ho + 3 * N, N * 4);
        std::memcpy(JbBuffer_new, ho + 4 * N, 10 * N * 4); std::memcpy(isGood_new, ho + 14 * N, N);
        std::memcpy(sums, hst + sums_off, 91 * 8);
    }
    init_sums_to_system(sums, T, n, P, X, H_out, b_out, H_out_sc, b_out_sc, E3);
    return NALO_OK;
}

int nalo_init_do_step(nalo_ctx* c, int n, const uint8_t* isGood, const float* JbBuffer, const float* maxstep, const float* idepth, float lambda, const float inc[8], float* idepth_new) {
    if (!c || n < 0 || !inc || (n > 0 && (!isGood || !JbBuffer || !maxstep || !idepth || !idepth_new))) return fail(c, NALO_ERR_ARG, "nalo_init_do_step: bad argument");
    if (n == 0) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    // words: [Jb(10n) | maxstep | idepth | idepth_new (in/out) | isGood bytes]
    const size_t N = (size_t)n, tot = 13 * N + (N + 3) / 4;
    int rc = imm_stage(c, tot); if (rc) return rc;
    float* hst = c->imm_host.p;
    std::memcpy(hst, JbBuffer, 10 * N * 4); std::memcpy(hst + 10 * N, maxstep, N * 4); std::memcpy(hst + 11 * N, idepth, N * 4); std::memcpy(hst + 12 * N, idepth_new, N * 4);
    std::memcpy(hst + 13 * N, isGood, N);
    float* d = c->imm_dev.p;
    NALO_HIP(c, hipMemcpyAsync(d, hst, tot * 4, hipMemcpyHostToDevice, c->stream));
    rc = init_do_step_launch(c, n, (const uint8_t*)(d + 13 * N), d, d + 10 * N, d + 11 * N, lambda, inc, d + 12 * N);
    if (rc) return rc;
    NALO_HIP(c, hipMemcpyAsync(hst + 12 * N, d + 12 * N, N * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(idepth_new, hst + 12 * N, N * 4);
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ profiling
static void prof_drain(nalo_ctx* c) {
    for (auto& kv : c->prof) {
        for (auto& ev : kv.second.pending) {
            float ms = 0;
            if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { kv.second.ms += ms; kv.second.n++; if (kv.second.samples.size() < (size_t)1 << 20) kv.second.samples.push_back(ms); }
            c->prof_pool.push_back(ev.first); c->prof_pool.push_back(ev.second);
        }
        kv.second.pending.clear();
    }
}
int nalo_profile_enable(nalo_ctx* c, int on) {
    if (!c) return NALO_ERR_ARG;
    c->prof_on = on != 0;
    if (on) while (c->prof_pool.size() < 4096) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) break; c->prof_pool.push_back(e); }
    return NALO_OK;
}
int nalo_profile_select(nalo_ctx* c, const char* kernel) { if (!c) return NALO_ERR_ARG; c->prof_only = kernel ? kernel : ""; return NALO_OK; }
int nalo_profile_sample(nalo_ctx* c, int every) { if (!c || every < 1) return NALO_ERR_ARG; c->prof_every = every; c->prof_tick = 0; return NALO_OK; }
int nalo_profile_reset(nalo_ctx* c) { if (!c) return NALO_ERR_ARG; prof_drain(c); c->prof.clear(); return NALO_OK; }
int nalo_profile_get(nalo_ctx* c, const char* kernel, double* total_ms, int* launches) {
    if (!c || !kernel) return NALO_ERR_ARG;
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    prof_drain(c);
    auto it = c->prof.find(kernel);
    if (total_ms) *total_ms = it == c->prof.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == c->prof.end() ? 0 : it->second.n;
    return NALO_OK;
}

// every bracketed launch of a scope since the last reset, in launch order (milliseconds): what a mean hides - the spread, and the position inside a keyframe
int nalo_profile_samples(nalo_ctx* c, const char* kernel, float* ms, int cap, int* n) {
    if (!c || !kernel || cap < 0 || (cap > 0 && !ms)) return NALO_ERR_ARG;
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    prof_drain(c);
    auto it = c->prof.find(kernel);
    const int have = it == c->prof.end() ? 0 : (int)it->second.samples.size();
    if (n) *n = have;
    if (ms && have) std::memcpy(ms, it->second.samples.data(), (size_t)std::min(cap, have) * sizeof(float));
    return NALO_OK;
}

int nalo_hbm_calibrate(nalo_ctx* c, size_t bytes, int iters, double* copy_GBs, double* triad_GBs) {
    bytes &= ~(size_t)15;
    if (!c || bytes < ((size_t)1 << 20) || iters < 1) return fail(c, NALO_ERR_ARG, "nalo_hbm_calibrate: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    const size_t n = bytes / 16;
    DevBuf<float4> a, b, d;
    Event e0, e1;
    if (a.reserve(n) != hipSuccess || b.reserve(n) != hipSuccess || d.reserve(n) != hipSuccess ||
        e0.create() != hipSuccess || e1.create() != hipSuccess) return fail(c, NALO_ERR_HIP, "nalo_hbm_calibrate: allocation failed");
    if (hipMemsetAsync(a.p, 0, bytes, c->stream) != hipSuccess || hipMemsetAsync(b.p, 0, bytes, c->stream) != hipSuccess) return fail(c, NALO_ERR_HIP, "nalo_hbm_calibrate: memset failed");
    for (int which = 0; which < 2; ++which) {
        double* out = which ? triad_GBs : copy_GBs;
        if (!out) continue;
        hbm_stream_launch(c->stream, a.p, b.p, d.p, n, which);                               // untimed: first touch, clocks
        (void)hipEventRecord(e0, c->stream);
        for (int i = 0; i < iters; ++i) hbm_stream_launch(c->stream, a.p, b.p, d.p, n, which);
        (void)hipEventRecord(e1, c->stream);
        if (hipEventSynchronize(e1) != hipSuccess) return fail(c, NALO_ERR_HIP, "nalo_hbm_calibrate: kernel failed");
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *out = (which ? 3.0 : 2.0) * (double)bytes * iters / ((double)ms * 1e-3) / 1e9;
    }
    return NALO_OK;
}

}  // extern "C"
