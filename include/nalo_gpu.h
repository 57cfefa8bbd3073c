/*
 * nalo_gpu.h — C ABI of the MI355X (gfx950) hot path of the NALO-SLAM direct photometric core.
 *
 * Drop-in boundary. The reference has no FFI: its hot path is plain C++ member calls.
 * Every entry point below names the reference call site it replaces (paths relative to the reference's
 * src/). A maintainer binds these from the reference's own FullSystem / CoarseTracker / EnergyFunctional
 * (see INTEGRATION.md for the stubs).
 *
 * Conventions
 *   - opaque nalo_ctx*, one per thread of use (the reference keeps two CoarseTracker instances and one
 *     EnergyFunctional, FullSystem/FullSystem.h:310-311; use one ctx per such owner);
 *   - every call returns 0 on success, <0 on error (nalo_last_error gives the message); no exceptions
 *     cross the ABI; all calls are synchronous on return unless suffixed _async;
 *   - plain pointers and sizes only; host buffers are caller-owned; matrices are row-major;
 *   - SE(3) is a row-major 3x4 [R|t] of doubles; the tangent order is Sophus' [translation(3), rotation(3)];
 *   - arithmetic is IEEE fp32 on the device exactly where the reference uses float, partial sums are
 *     finished in fp64, stitched systems and solves are fp64 (reference: Eigen double).
 *   - the library needs a gfx950 device; there is no CPU fallback (calls fail with NALO_ERR_NO_DEVICE).
 */
#ifndef NALO_GPU_H
#define NALO_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nalo_ctx nalo_ctx;

enum {
    NALO_OK = 0,
    NALO_ERR_ARG = -1,
    NALO_ERR_NO_DEVICE = -2,
    NALO_ERR_HIP = -3,
    NALO_ERR_STATE = -4,
    NALO_ERR_UNSUPPORTED = -5
};

#define NALO_MAX_LEVELS 6     /* PYR_LEVELS, util/settings.h:52 (tracker uses <= 5, CoarseTracker.cpp:1083) */
#define NALO_MAX_WINDOW 16    /* frames in the BA window; reference: setting_maxFrames+1 = 8 (util/settings.cpp:88) */

/* ------------------------------------------------------------------------------------------------
 * Context.  Replaces: setGlobalCalib (util/globalCalib.cpp:45-105) + the allocations in
 * CoarseTracker::CoarseTracker (FullSystem/CoarseTracker.cpp:58-95) / EnergyFunctional().
 * levels <= 0 -> use the reference's level rule (halve while both dims even and area > 5000).
 * K = {fx, fy, cx, cy} at level 0. n_slots = number of frame slots (pyramids resident in HBM).
 * ------------------------------------------------------------------------------------------------ */
int nalo_create(nalo_ctx** out, int device, int w, int h, int levels, const float K[4], int n_slots);
void nalo_destroy(nalo_ctx* ctx);
const char* nalo_last_error(nalo_ctx* ctx);
int nalo_levels(nalo_ctx* ctx);
int nalo_sync(nalo_ctx* ctx);
void* nalo_stream(nalo_ctx* ctx);                 /* hipStream_t every kernel of this ctx is launched on */

/* For tests only: arm one injected failure on this context. The count-th matching event from now fails once and the injector disarms itself;
 * count = 0 disarms. NALO_ERR_ARG for a null context, an unknown `what` or a negative count. Needs no window and makes no device call.
 *   NALO_INJECT_LM_LOST_BLOCK  a persistent LM launch of nalo_trk_track reports a lost workgroup after it has completed: the frame is redone by
 *                              the host-driven loop, which the context keeps to from then on;
 *   NALO_INJECT_GATED_SOLVE    a solve of nalo_ba_optimize that has pre-launched its back-substitution fails between the pre-launch and its gates.
 * The library reads one environment variable, NALO_HOST_TIMING, once per context in nalo_create (host-side accounting printed at nalo_destroy). */
#define NALO_INJECT_LM_LOST_BLOCK 1
#define NALO_INJECT_GATED_SOLVE   2
int nalo_test_inject(nalo_ctx* ctx, int what, int count);

/* ------------------------------------------------------------------------------------------------
 * Settings of the reference that change the arithmetic of this path (util/settings.cpp). Defaults = the reference's; nalo_set_settings before
 * nalo_ba_set_window / nalo_trk_track. Everything else in settings.cpp that this path reads is a compile-time constant here, as it is never changed by
 * the reference's CLI (main_dso_pangolin.cpp:400-460 changes exactly these: mode=1 sets the affine modes to 0, mode=2 to -1).
 *   forceAcceptStep   setting_forceAceptStep (:71, default 1). 0: FullSystem::optimize linearises WITHOUT applyRes, compares
 *                     E + calcLEnergy + calcMEnergy against the last accepted values and either applies the step or restores the backup
 *                     (FullSystemOptimize.cpp:511-541). On a sharded window the scalars of that test are summed over the ranks through the all-reduce hook
 *                     (three more calls of 1, 1 and 3 doubles per evaluation), so every rank takes the same branch.
 *   affineOptModeA/B  setting_affineOptModeA / B (:128-129, defaults 1e12 / 1e8): >= 0 = prior on a / b of every frame but the first
 *                     (FrameHessian::getPrior, HessianBlocks.h:286-312), < 0 = fixed: the prior becomes setting_initialAffAPrior / BPrior, JabF[0] / JabF[1]
 *                     are zeroed (Residuals.cpp:241-242), the tracker solves the reduced 6x6 / 7x7 system (CoarseTracker.cpp:1140-1162, host LM loop) and
 *                     zeroes the fixed output (:1255-1256); == 0 switches the tracker's plausibility test to relAff (:1249-1250).
 *   minOptIterations  setting_minOptIterations (:74, default 1).
 * ------------------------------------------------------------------------------------------------ */
/* The reference constants the library was compiled with (util/settings.cpp:56-160,297, util/settings.h:52,232-234, FullSystem/HessianBlocks.h:61-68,268,
 * util/NumType.h:41-53), under the reference's own names ("setting_huberTH", "SCALE_XI_TRANS", "patternP[3].x", ...). They come from the one table the host and
 * device code take their constexpr values from (csrc/ref_constants.h). Float settings carry the value the reference's `float` holds (setting_initialRotPrior =
 * 1e11 is 99999997952). Returns the number of entries; the first min(cap, n) names (static strings) / values are written; either array may be NULL. No device needed. */
int nalo_constants(int cap, const char** names, double* values);
/* the same table as the DEVICE code evaluates it (a one-lane kernel writes every entry): values[i] belongs to names[i] of nalo_constants. Returns the number of entries. */
int nalo_constants_device(nalo_ctx* ctx, int cap, double* values);
typedef struct nalo_settings {
    int forceAcceptStep;
    double affineOptModeA, affineOptModeB;
    int minOptIterations;
} nalo_settings;
int nalo_get_settings(nalo_ctx* ctx, nalo_settings* out);
int nalo_set_settings(nalo_ctx* ctx, const nalo_settings* in);

/* ------------------------------------------------------------------------------------------------
 * a1  FrameHessian::makeImages (FullSystem/HessianBlocks.cpp:127-190), called at FullSystem.cpp:1065.
 * Uploads level-0 irradiance (w*h floats, 0..255), builds all pyramid levels {I,dx,dy} + absSquaredGrad
 * in HBM. mask (w*h floats) and bgr (3*w*h bytes) are optional (densemap=1 only); gammaB[256] optional
 * (CalibHessian::B, HessianBlocks.h:397-406; NULL = identity).
 * ------------------------------------------------------------------------------------------------ */
int nalo_frame_upload(nalo_ctx* ctx, int slot, const float* irradiance, const float* mask, const uint8_t* bgr,
                      const float* gammaB);
/* The per-frame entry of a running pipeline (FullSystem::addActiveFrame -> makeImages, FullSystem.cpp:1053-1065): same as nalo_frame_upload, but the H2D
 * copies run on the context's copy stream — under the kernels the main stream is executing for the previous frame — and the pyramid kernels are queued
 * behind them. Returns immediately; irradiance / mask / bgr / gammaB must stay untouched until nalo_frame_wait(ctx, slot) or nalo_sync returns.
 * Asynchronous only from pinned host memory: nalo_host_alloc / nalo_host_free (= hipHostMalloc / hipHostFree) hand out such buffers. */
int nalo_frame_upload_async(nalo_ctx* ctx, int slot, const float* irradiance, const float* mask, const uint8_t* bgr,
                            const float* gammaB);
int nalo_frame_wait(nalo_ctx* ctx, int slot);
/* The sensor frame as the dataset holds it: Undistort::undistort<T> (util/Undistort.cpp:435-530) = PhotometricUndistorter::processFrame
 * (:214-251) + the bilinear remap, and the INTER_NEAREST resizes of Undistort::undistort_mask (:385-433, IOWrapper/OpenCV/ImageRW_OpenCV.cpp:55-85), fused
 * in front of makeImages; call site ImageFolderReader::getImage_internal (util/DatasetReader.h:270-298) -> FullSystem::addActiveFrame.
 * nalo_undist_set          the tables of the Undistort object, uploaded once: the response G (GDepth >= 256 entries, already rescaled to 0..255 as
 *                          Undistort.cpp:101-103 does: nalo_io_read_pcalib), vignetteMapInv [wOrg*hOrg] (nalo_io_make_vignette; NULL without a vignette),
 *                          photometricCalibration = setting_photometricCalibration (0 none, 1 response only, 2 response + vignette; util/settings.cpp:40),
 *                          remapX / remapY [w*h] in original-image pixels, -1 = outside (Undistort.cpp:998-1010); NULL = passthrough (wOrg x hOrg = w x h).
 *                          Every entry with remapX >= 0 needs 0 <= x < wOrg - 1 and 0 <= y < hOrg - 1 (NaN and infinities are refused); the whole table is
 *                          checked before anything is stored: a refused call (NALO_ERR_ARG) leaves the tables of the last accepted call in place.
 * nalo_frame_upload_raw    raw = wOrg*hOrg pixels of bytes_per_px 1 (uchar) or 2 (ushort); exposure_time <= 0 disables the photometric part for this frame
 *                          (data = factor * raw, :224-231); mask_org [wOrg*hOrg] / bgr_org [wOrg*hOrg*3] optional (dense=1 / densemap=1 inputs);
 *                          gammaB as in nalo_frame_upload. The frame crosses PCIe at 1-2 B/px instead of 4. Synchronous like nalo_frame_upload. */
int nalo_undist_set(nalo_ctx* ctx, int wOrg, int hOrg, const float* G, int GDepth, const float* vignetteMapInv, int photometricCalibration, const float* remapX,
                    const float* remapY);
int nalo_frame_upload_raw(nalo_ctx* ctx, int slot, const void* raw, int bytes_per_px, float exposure_time, float factor, const uint8_t* mask_org, const uint8_t* bgr_org,
                          const float* gammaB);
/* asynchronous form for tracked (non-key) frames, as nalo_frame_upload_async: the raw copy runs on the copy stream, ingest + pyramid are queued behind it; returns
 * at once, raw must stay untouched until nalo_frame_wait(ctx, slot) (pinned memory: nalo_host_alloc). No mask / colour (keyframe inputs). */
int nalo_frame_upload_raw_async(nalo_ctx* ctx, int slot, const void* raw, int bytes_per_px, float exposure_time, float factor, const float* gammaB);
/* Frames, masks and colour that already live on the device. The reference loads mask and colour with every frame (util/DatasetReader.h:296-315,
 * FullSystem.cpp:1053-1059) although only keyframes use them, and whether a frame becomes one is decided after it has been tracked (FullSystem.cpp:1113-1132);
 * the mask is the output of a network and a decoded frame is a tensor, both in device memory. These calls take such planes where they lie, in stream order, and
 * attach mask and colour to a slot whose pyramid exists already.
 * nalo_dev_plane            one plane by byte strides: element (x, y, ch) is at ptr + y * stride_y + x * stride_x + ch * stride_c. A pitched region of a larger
 *                           tensor, an x-strided view, interleaved (HWC) and planar (CHW) colour are all described this way. No byte outside the described
 *                           elements is read. A NALO_DT_F32 DEPTH plane whose w x h differ from the context's size is legal in nalo_tsdf_integrate_depth: its
 *                           intrinsics come with that call.
 * nalo_dev_plane_check      validates a descriptor and launches nothing. NALO_ERR_ARG for: a null descriptor or pointer; a pointer that hipPointerGetAttributes does
 *                           not report as device memory of the context's GPU (host, pinned host, managed and other devices' memory); a dtype outside NALO_DT_*;
 *                           channels other than 1 or 3; w or h < 1; a negative stride; a pointer or stride that is no multiple of the element size; stride_x
 *                           below the element size (w > 1), or a stride_c under which channels overlap inside a row (accepted: 2 * stride_c + element <= stride_x,
 *                           interleaved, or stride_c >= the bytes a row spans, planar); where hipMemGetAddressRange answers, an extent that leaves the allocation.
 *                           The runtime's sticky error is cleared after a failed query.
 * nalo_frame_ingest_device  image  NALO_DT_U8 / _U16: the sensor frame, und_wOrg x und_hOrg, treated exactly as nalo_frame_upload_raw treats raw (photometric modes,
 *                                  exposure_time <= 0, remap or passthrough; NALO_ERR_STATE before nalo_undist_set, NALO_ERR_ARG for a 16-bit frame over a response
 *                                  of less than 65536 entries). NALO_DT_F32: rectified irradiance, w x h, copied to level 0 bit for bit (NaN payloads included) as
 *                                  nalo_frame_upload takes it. The pyramid follows as in the host calls. NULL: attach only - the slot must hold a pyramid
 *                                  (NALO_ERR_STATE otherwise), which is left untouched.
 *                           mask   optional, one channel of U8 ((float)v * 1.0f), I32 ((float)v, round to nearest even) or F32 (bit for bit), any size >= 1x1;
 *                           colour optional, three channels of U8, any size; colour_is_rgb: channel 0 is R. Both are resized to w x h with
 *                                  cv::resize(INTER_NEAREST) exactly as Undistort::undistort_mask does (util/Undistort.cpp:385-433; at equal size the identity);
 *                                  the slot stores w*h floats and interleaved B,G,R bytes as after nalo_frame_upload_raw.
 *                           Stream order: the library lets its main stream wait, on the device, for everything queued on producer_stream at the time of the call
 *                           (skipped when that is the context's own stream, nalo_stream), queues its kernels on the main stream and records the slot's event
 *                           behind the last one that reads a caller's plane. nalo_frame_wait(slot) waits for that event on the host, nalo_frame_release lets
 *                           a stream wait for it on the device; after either the planes may be overwritten or freed. With its buffers sized and the gamma table of
 *                           the previous call, the call makes no host wait.
 *                           Every plane goes through nalo_dev_plane_check, and every other condition is tested, before anything is queued or reserved: a refused
 *                           call (NALO_ERR_ARG / NALO_ERR_STATE) leaves slot and context as they were.
 * nalo_frame_release        `stream` (NULL: the null stream) waits, on the device, until the slot's last ingest has read its planes. Nothing to wait for: NALO_OK.
 * nalo_frame_attach         the same attach from HOST memory in the sensor's size (mask_org [und_wOrg*und_hOrg], bgr_org [und_wOrg*und_hOrg*3], either may be
 *                           NULL, not both): for the frame that nalo_frame_upload_raw_async brought in and that tracking then made a keyframe. Synchronous like
 *                           nalo_frame_upload_raw; the pyramid stays. NALO_ERR_STATE before nalo_undist_set and on a slot without a pyramid.
 * After mask or colour changed under an unchanged image the last pixel-selection map made on the slot is dropped (nalo_pixsel_make_maps_lidar reads the mask);
 * the gradient histograms stay. */
#define NALO_DT_U8 1
#define NALO_DT_U16 2
#define NALO_DT_I32 3
#define NALO_DT_F32 4
typedef struct nalo_dev_plane {
    const void* ptr;                 /* device memory of the context's GPU */
    int dtype;                       /* NALO_DT_* */
    int w, h, channels;              /* channels 1, or 3 for colour */
    long long stride_y, stride_x, stride_c;   /* BYTES; >= 0; stride_c ignored when channels == 1 */
} nalo_dev_plane;
typedef struct nalo_frame_ingest_args {
    const nalo_dev_plane* image;     /* U8/U16: sensor frame und_wOrg x und_hOrg; F32: rectified irradiance w x h; NULL: attach only */
    float exposure_time, factor;     /* sensor frames only, as nalo_frame_upload_raw */
    const nalo_dev_plane* mask;      /* optional. U8 / I32 / F32, any size >= 1x1 */
    const nalo_dev_plane* colour;    /* optional. U8, 3 channels, any size */
    int colour_is_rgb;               /* channel 0 is R; the slot always stores B,G,R (img_bgr) */
    const float* gammaB;             /* host, 256 floats or NULL, as elsewhere */
    void* producer_stream;           /* hipStream_t whose queued work produces the planes; NULL = the null stream */
} nalo_frame_ingest_args;
int nalo_frame_ingest_device(nalo_ctx* ctx, int slot, const nalo_frame_ingest_args* args);
int nalo_frame_release(nalo_ctx* ctx, int slot, void* stream);
int nalo_dev_plane_check(nalo_ctx* ctx, const nalo_dev_plane* plane);
int nalo_frame_attach(nalo_ctx* ctx, int slot, const uint8_t* mask_org, const uint8_t* bgr_org);
void* nalo_host_alloc(size_t bytes);
void nalo_host_free(void* p);
/* makeImages again from the level-0 irradiance already resident in the slot (asynchronous on the ctx stream): the
 * HBM-resident form of a1, used when the caller's frames already live on the device */
int nalo_frame_rebuild(nalo_ctx* ctx, int slot);
/* test/inspection: level image as AoS {I,dx,dy} (3 floats/px) and absSquaredGrad (1 float/px); either may be NULL */
int nalo_frame_download(nalo_ctx* ctx, int slot, int lvl, float* dI3, float* abs_sq_grad);
/* test/inspection: the slot's level-0 mask (w*h floats) and colour (3*w*h bytes) as nalo_frame_upload[_async] stored them or nalo_frame_upload_raw resized them;
 * either may be NULL (not both). NALO_ERR_STATE when the slot holds no pyramid or lacks a plane that is asked for (nothing is written then), NALO_ERR_ARG on a bad slot. */
int nalo_frame_download_mask(nalo_ctx* ctx, int slot, float* mask, uint8_t* bgr);
/* Views of what is resident: the library describing its own device memory, the reverse of nalo_frame_ingest_device. Host code only: nothing is launched, copied or
 * waited for. The reference tracks on the caller's thread and maps on its own (FullSystem.cpp:1183-1252), so a binder keeps one context per thread; a view is
 * the plain struct that crosses between them (see also nalo_trk_ref_export / nalo_trk_ref_import below).
 * nalo_frame_plane   fills *out with a descriptor of one level-0 plane of the slot, which nalo_dev_plane_check accepts and nalo_frame_ingest_device reads:
 *                    NALO_PLANE_IRRADIANCE  F32, w x h, contiguous (what nalo_frame_download(slot, 0) returns as I, bit for bit)
 *                    NALO_PLANE_MASK        F32, w x h, contiguous        NALO_PLANE_COLOUR  U8 x 3, interleaved B,G,R
 *                    It refuses exactly where nalo_frame_download_mask refuses: NALO_ERR_ARG for a NULL ctx or out, a bad slot or a bad `which`; NALO_ERR_STATE
 *                    for a slot without a pyramid or without the plane asked for. On a refusal *out is untouched.
 *   The frame hand-off from a tracking context T to a mapping context M needs no more than this: nalo_frame_plane(T, slot, ...) for the irradiance (and mask and
 *   colour where the slot has them), then nalo_frame_ingest_device(M, slot', {image = the F32 plane, mask, colour, the same gammaB, producer_stream =
 *   nalo_stream(T)}). Level 0 is copied as words and the pyramid is rebuilt from it, so M's slot equals T's bit for bit on every level, at 4 bytes read per pixel
 *   where a copy of the pyramid would move 24 B x 1.33. nalo_frame_release(M, slot', nalo_stream(T)) is the back edge before T reuses its slot.
 * Lifetime of a view (a nalo_dev_plane from nalo_frame_plane, a nalo_trk_ref_view from nalo_trk_ref_export): a snapshot of pointers and counts that owns nothing.
 *   It describes what the source's main stream (nalo_stream) has produced once everything queued on that stream at the time of the call has run - a consumer on
 *   another stream waits for that stream first, which nalo_frame_ingest_device (producer_stream) and nalo_trk_ref_import (view->stream) do on the device. It stays
 *   good until the next call that rewrites what it names: an upload, ingest or attach into the slot; nalo_trk_set_ref*, nalo_trk_set_pc, nalo_trk_set_depth, the
 *   append calls (nalo_trk_append_plane_points, nalo_trk_fit_planes / nalo_trk_fit_ground with append) or nalo_trk_ref_import. It never outlives nalo_destroy.
 * Threads: the library takes no locks. A context is used by one thread at a time; nalo_frame_plane and nalo_trk_ref_export are called by the thread that owns the
 *   source (or under the lock that orders its rewriting calls - coarseTrackerSwapMutex in the reference), nalo_frame_ingest_device and nalo_trk_ref_import by the
 *   thread that owns the destination. A wait or a record on the other context's main stream goes through the raw stream handle only: neither the import's wait
 *   nor nalo_trk_ref_release / nalo_frame_release reads or writes the other nalo_ctx. */
#define NALO_PLANE_IRRADIANCE 0   /* level 0, F32, w x h, contiguous */
#define NALO_PLANE_MASK       1   /* F32, w x h */
#define NALO_PLANE_COLOUR     2   /* U8 x 3, interleaved B,G,R */
int nalo_frame_plane(nalo_ctx* ctx, int slot, int which, nalo_dev_plane* out);

/* ------------------------------------------------------------------------------------------------
 * Front-end tracker.
 * ------------------------------------------------------------------------------------------------ */
/* CoarseTracker::makeK (CoarseTracker.cpp:97-141): pyramid intrinsics from the current calibration */
int nalo_trk_make_k(nalo_ctx* ctx, float fx, float fy, float cx, float cy);

/* a2  CoarseTracker::setCoarseTrackingRef -> makeCoarseDepthL0 steps 1-5 (CoarseTracker.cpp:1053-1067, 382-538),
 * called at FullSystem.cpp:1404. One entry per IN residual targeting the reference keyframe:
 * centerProjectedTo = (Ku, Kv, new_idepth) and the point's HdiF. Builds idepth/weight pyramids and the
 * per-level point clouds pc_u/pc_v/pc_idepth/pc_color in raster order. */
int nalo_trk_set_ref(nalo_ctx* ctx, int slot_ref, int n, const float* Ku, const float* Kv,
                     const float* new_idepth, const float* HdiF);
/* The same with the four input arrays RESIDENT on the device (round 4): nalo_trk_ref_upload copies them into a block the context owns (one pinned staging copy + one
 * H2D copy, as nalo_trk_set_ref does on every call) and nalo_trk_set_ref_resident runs makeCoarseDepthL0 (CoarseTracker.cpp:382-538) from that block - for a caller whose
 * inputs do not change between calls, or who fills them ahead of time: the per-keyframe call then pays no host copy, no staging and no copy packet in front of its kernels.
 * The block stays valid until the next nalo_trk_ref_upload; nalo_trk_set_ref leaves it untouched. Results are those of nalo_trk_set_ref on the same arrays, bit for bit. */
int nalo_trk_ref_upload(nalo_ctx* ctx, int n, const float* Ku, const float* Kv, const float* new_idepth, const float* HdiF);
int nalo_trk_set_ref_resident(nalo_ctx* ctx, int slot_ref);
/* a2 fed from the window: makeCoarseDepthL0 (CoarseTracker.cpp:382-538) on the IN residuals that target the window's newest frame,
 * read on the device. The reference slot is frames[W-1].slot of the last nalo_ba_set_window.
 * One entry per point whose residual to frame W-1 is IN at the window's last linearizeAll(true) (lastResiduals[0]), with that residual's
 * centerProjectedTo and the HdiF nalo_ba_get_points would return at this moment, in the reference's loop order (window host index, then the
 * nalo_ba_set_points order inside a host). Results are those of nalo_trk_set_ref(ctx, frames[W-1].slot, ...) on those arrays, bit for bit; no window
 * data crosses to the host. NALO_ERR_STATE: no window or no points, no pyramid in the newest frame's slot, the window's last linearisation was not a
 * fix = 1 one (nalo_ba_optimize ends with one), or the window is sharded (a rank holds its own points only: collect the inputs and call
 * nalo_trk_set_ref). The block of nalo_trk_ref_upload is left alone. */
int nalo_trk_set_ref_from_window(nalo_ctx* ctx);
/* a2 fed from a depth plane that lies on the device: the ray-cast of the fused model (nalo_tsdf_raycast_view's depth), a depth sensor's plane, a densified
 * keyframe. DEFINED as nalo_trk_set_ref(ctx, slot_ref, n, Ku, Kv, new_idepth, HdiF) on the list of the passing pixels in raster order (v outer, u inner), with
 *     pass(u, v) = u % step == 0 && v % step == 0 && D >= min_depth && D <= max_depth && (min_grad == 0.0f || absg >= min_grad)
 *     D = the plane's element (u, v), absg = the level-0 absSquaredGrad of slot_ref at (u, v) (what nalo_frame_download(slot_ref, 0) returns), every comparison
 *     a float comparison on the values as they stand, before any conversion: a NaN D or absg fails, -0.0f and 0.0f fail min_depth > 0; min_grad == 0.0f (or
 *     -0.0f) switches the gradient test off and absg is not read
 *     Ku = (float)u, Kv = (float)v, new_idepth = 1.0f / D (one correctly rounded division), HdiF = hdi,
 *     hence weight = sqrtf((float)(1e-3 / ((double)hdi + 1e-12))) for every point (CoarseTracker.cpp:397)
 * Results are that call's, bit for bit, in both maps of every level, in pc_n, in the four cloud arrays of every level and in slot_ref; n_seeded = n. No pixel
 * passes (a ray-cast that hit nothing): legal, the result of nalo_trk_set_ref with n = 0. Nothing crosses to the host but pc_n and n_seeded; the list is never
 * formed: every pixel takes at most one hit, so one kernel writes idepth[0] and weightSums[0] and sums every coarser level in the same pass, in place of the zero
 * fill, the scatter, its ordered redo and the sum pyramid; dilation, count, scan and write follow as in every nalo_trk_set_ref*.
 * depth   F32, one channel, exactly the context's w x h, any strides nalo_dev_plane_check accepts (pitched, x-strided); no byte outside the described elements
 *         is read. It must not overlap the reference's own buffers (what nalo_trk_ref_export describes): as in nalo_trk_ref_import this is the caller's to keep,
 *         it is not checked.
 * Stream order as nalo_tsdf_integrate_depth: the main stream waits, on the device, for what producer_stream (NULL: the null stream) has queued at the time of
 *         the call - skipped when that is the context's own stream. The call ends with the host poll for pc_n that every nalo_trk_set_ref* ends with, and that
 *         poll lies behind the only kernel that reads the plane: when the call returns the plane HAS been read and may be overwritten or freed - there is no
 *         release call. No other host wait; with the buffers sized, no allocation.
 * Everything is checked before anything is queued or reserved; a refused call leaves the reference bit-identical - slot_ref included - and sets n_seeded = 0.
 *         NALO_ERR_ARG: a NULL ctx or args; a bad slot_ref; a plane nalo_dev_plane_check refuses; a dtype other than F32, or three channels; w or h that differ
 *         from the context's; min_depth not finite or <= 0; max_depth not finite, or min_depth > max_depth; hdi not finite or < 0; step < 1; a NaN min_grad.
 *         NALO_ERR_STATE: slot_ref holds no pyramid. */
typedef struct nalo_trk_depth_ref_args {
    nalo_dev_plane depth;        /* F32, one channel, exactly the context's w x h, any strides nalo_dev_plane_check accepts */
    float min_depth, max_depth;  /* D is usable iff D >= min_depth && D <= max_depth (a NaN fails); min_depth > 0 */
    float hdi;                   /* the HdiF every point gets; weight = sqrtf((float)(1e-3 / ((double)hdi + 1e-12))) as in step 1 */
    int step;                    /* >= 1: only pixels with u % step == 0 && v % step == 0 */
    float min_grad;              /* only pixels whose level-0 absSquaredGrad of slot_ref is >= min_grad; 0.0f switches the test off (absg is not read) */
    void* producer_stream;       /* whose queued work produces the plane; NULL = the null stream */
    int n_seeded;                /* out: the pixels that passed */
} nalo_trk_depth_ref_args;
int nalo_trk_set_ref_from_depth(nalo_ctx* ctx, int slot_ref, nalo_trk_depth_ref_args* args);
/* direct injection of one level's point cloud (synthetic stress windows) */
int nalo_trk_set_pc(nalo_ctx* ctx, int slot_ref, int lvl, int n, const float* u, const float* v,
                    const float* idepth, const float* color);
int nalo_trk_get_pc(nalo_ctx* ctx, int lvl, int* n, float* u, float* v, float* idepth, float* color);
/* dense=1: the plane-sampled points makeCoarseDepthL0 appends to the LEVEL-0 cloud after step 5 (CoarseTracker.cpp:600-655), one call per mask cluster, on
 * the device (no round trip of the cloud): dir / dis_plane = the cluster's fitted plane (fitPlane: nalo_trk_fit_planes below, or a PCL RANSAC on the caller's side), refMaskColor =
 * clusters[i][0][3], rect = {minx, maxx, miny, maxy} of the cluster's pixels. Uses the mask and I of the tracking reference's slot (frameHessians.back() is
 * lastRef). Appends, in the reference's x-outer / y-inner order, every (x % 5 == 0, y % 5 == 0) pixel of [minx,maxx) x [miny,maxy) whose mask equals
 * refMaskColor with new_idepth = dir^T Ki (x,y,1) / -dis_plane and colour I_ref(x,y) — INCLUDING the reference's off-by-one (the k-th point is stored at
 * pc_n + 1 + k while pc_n grows by one per point, :646-650): slot [old pc_n] is left unwritten by the reference (defined as zeros here) and the last
 * sampled point stays outside the count. Nothing is appended when the box touches the border, refMaskColor is 0 (:621-630). *n_added = growth of pc_n[0]. */
int nalo_trk_append_plane_points(nalo_ctx* ctx, const float dir[3], float dis_plane, int refMaskColor, const int rect[4], int* n_added);
int nalo_trk_get_depth(nalo_ctx* ctx, int lvl, float* idepth, float* weight_sums);
/* The counterpart of nalo_trk_get_depth (as nalo_trk_set_pc is of nalo_trk_get_pc): direct injection of one level's inverse-depth map and weight sums, w_lvl * h_lvl
 * floats each. Allocates the level's buffers when no reference was set (a half that is not given then reads as zeros) and sets slot_ref. Either array may be NULL: a NULL
 * idepth leaves the level's inverse depths untouched, a NULL weight_sums its weight sums. Nothing else is touched: no cloud, no other level. For tests (maps the scatter
 * and dilation of nalo_trk_set_ref never produce) and as the missing half of a tracker checkpoint. */
int nalo_trk_set_depth(nalo_ctx* ctx, int slot_ref, int lvl, const float* idepth, const float* weight_sums);
/* The tracking reference between contexts, on the device. The reference keeps two CoarseTracker objects: makeKeyFrame rebuilds the idle one on the mapping thread
 * under coarseTrackerSwapMutex (FullSystem.cpp:1401-1410) and addActiveFrame swaps it in on the tracking thread (:1094-1098). Here the mapping context builds the
 * reference where its window lives (nalo_trk_set_ref_from_window), describes it, and the tracking context clones it from device memory: no cloud or map visits
 * the host. Lifetime of a view and the thread contract: see nalo_frame_plane above.
 * nalo_trk_ref_export   fills *out with the context's current reference: per level the cloud's count and arrays, the idepth[] and weightSums[] maps (NULL where the
 *                       level has none, e.g. after nalo_trk_set_pc alone), CoarseTracker::makeK's intrinsics, and the context's main stream as the producer.
 *                       Host code only, no launch. NALO_ERR_ARG: NULL ctx / out. NALO_ERR_STATE: the context has no reference; *out is untouched then.
 * nalo_trk_ref_import   dst becomes a clone of the described reference: the first n[l] floats of u, v, idepth and color and both maps of every level are copied,
 *                       pc_n and the level intrinsics are taken over (the clouds mean nothing under another K; the reference calls makeK on the same object,
 *                       :1403), and dst's reference slot becomes slot_ref, which must hold the reference frame's pyramid in dst (nalo_trk_depth_image and the
 *                       append calls read it). A level whose map pointers are NULL has dst's maps zero-filled: dst never mixes two references. The view need not
 *                       come from nalo_trk_ref_export - pointers into a caller's device arrays make a reference of the caller's own; they must not overlap dst's.
 *                       Stream order, as in nalo_frame_ingest_device: dst's main stream waits, on the device, for what view->stream (NULL: the null stream) has
 *                       queued at the time of the call - skipped when that is dst's own stream -, ONE kernel copies every segment, and an event behind it
 *                       serves nalo_trk_ref_release. The counts arrive with the view: with its buffers sized, the call makes no host wait and no allocation.
 *                       Everything is checked before anything is queued or reserved; a refused call leaves dst's reference bit-identical. NALO_ERR_ARG: a NULL
 *                       ctx or view; w, h or levels that differ from dst's; n[l] < 0 or n[l] > (w>>l)*(h>>l); a NULL cloud pointer with n[l] > 0; a map pointer
 *                       given for one of the pair only; a pointer that is no multiple of 4 or that hipPointerGetAttributes does not report as device memory of
 *                       dst's GPU (nalo_dev_plane_check's test: host, pinned, managed and other devices' memory), or whose extent leaves its allocation; a bad
 *                       slot_ref. NALO_ERR_STATE: slot_ref holds no pyramid. NALO_ERR_HIP: a cross-rank exchange of dst failed earlier (as nalo_trk_track).
 * nalo_trk_ref_release  `stream` (NULL: the null stream) waits, on the device, until dst's last import has read its source: the back edge before the source
 *                       rewrites its reference - nalo_trk_ref_release(tracker, nalo_stream(mapper)). Nothing to wait for: NALO_OK. */
typedef struct nalo_trk_ref_view {
    int w, h, levels, slot_ref;                       /* of the context that made it */
    int n[NALO_MAX_LEVELS];                           /* pc_n */
    const float *u[NALO_MAX_LEVELS], *v[NALO_MAX_LEVELS], *idepth[NALO_MAX_LEVELS], *color[NALO_MAX_LEVELS];   /* n[l] floats each */
    const float *idepth_map[NALO_MAX_LEVELS], *weight_sums[NALO_MAX_LEVELS];   /* (w>>l) x (h>>l) floats; NULL: the level has none */
    float fx[NALO_MAX_LEVELS], fy[NALO_MAX_LEVELS], cx[NALO_MAX_LEVELS], cy[NALO_MAX_LEVELS];   /* CoarseTracker::makeK's */
    void* stream;                                     /* the producer: the source's main stream */
} nalo_trk_ref_view;
int nalo_trk_ref_export(nalo_ctx* src, nalo_trk_ref_view* out);
int nalo_trk_ref_import(nalo_ctx* dst, int slot_ref, const nalo_trk_ref_view* view);
int nalo_trk_ref_release(nalo_ctx* dst, void* stream);

/* CoarseTracker::debugPlotIDepthMap (CoarseTracker.cpp:1263-1359; FullSystem.cpp:1408 -> Output3DWrapper::pushDepthImage) on the device: the jet-coloured depth image
 * of the current tracking reference, from the level-0 inverse-depth map (what nalo_trk_get_depth(ctx, 0, ...) returns) and the planar irradiance I[0] of the reference's
 * slot. Runs on the context's stream behind whatever nalo_trk_set_ref* enqueued; the host waits once. The result equals the reference's loops byte for byte:
 *   - quantiles (:1271-1281): allID = every idepth[0][i] > 0 (NaN excluded, +inf included and last); with n = size - 1 the order statistics at ranks (int)(n * 0.05) and
 *     (int)(n * 0.95), the product in double. Found exactly by a radix select on the float bit patterns; the map is not sorted and the count does not visit the host.
 *   - smoothing (:1286-1313) against minmax_io = {minIdJetVisTracker, maxIdJetVisTracker}, which stay with the caller (start them at -1 as FullSystem.h does): float
 *     arithmetic as written, maxChange = (float)(0.3 * (double)(max - min)), the four ifs in the reference's order, the `< 0` initialisation; minmax_io is rewritten as the
 *     reference rewrites its pointers. NULL = the reference's NULL pointers: no smoothing, nothing written.
 *   - base image (:1318-1323): c = (int)(I * 0.9f), 255 if larger, the byte (unsigned char)c on all three channels (a negative c wraps: -1 -> 255).
 *   - plot rule (:1325-1344): source (x, y) with 3 <= x < w - 3, 3 <= y < h - 3 plots when bp[0] > 0 || nid >= 3 over the five-point stencil, colour
 *     makeJet3B(((sid / nid) - minID) / (maxID - minID)) (globalFuncs.h:350-367, branch arithmetic in double, bytes truncated).
 *   - setPixelCirc (MinimalImage.h:112-126): a plotting source colours the 40 pixels at Chebyshev distance 2 or 3 from it (not itself, not its eight neighbours);
 *     sources are visited in raster order, so where rings overlap the raster-last source wins. Computed as a gather, without atomics.
 * Three conversions the reference leaves undefined are DEFINED here:
 *   1. float -> int of the grey value outside int's range saturates, and NaN gives 0;
 *   2. a negative c wraps as C++'s int -> unsigned char does;
 *   3. a NaN id (maxID == minID: 0 / 0) paints the white pixel (255, 255, 255) that x86 produces.
 * NALO_ERR_ARG: NULL ctx / args / bgr. NALO_ERR_HIP: a cross-rank exchange of this context failed earlier. NALO_ERR_STATE: no tracking reference (the reference's
 * `w[1] == 0` return), or the map holds no positive value (the reference indexes an empty vector): then n_positive = 0, nothing is painted and bgr / idepth /
 * minmax_io are left as they were. A sharded tracker (nalo_trk_set_shard) holds the whole reference on every rank: the call works there unchanged.
 * debugSaveImages' PNG write stays with the caller. */
typedef struct nalo_depth_image_args {
    float*   minmax_io;          /* in/out {minID, maxID}; NULL = the reference's NULL pointers */
    uint8_t* bgr;                /* out, 3 * w * h bytes, raster order, the three bytes of a pixel in Vec3b's order: the MinimalImageB3 handed to pushDepthImage */
    float*   idepth;             /* out, optional, w * h: idepth[0] for pushDepthImageFloat, from the same call and the same wait */
    int      n_positive;         /* out: allID.size() */
    float    min_new, max_new;   /* out: allID[(int)(n*0.05)], allID[(int)(n*0.95)] */
    float    min_used, max_used; /* out: minID / maxID the image was painted with (after the smoothing) */
} nalo_depth_image_args;
int nalo_trk_depth_image(nalo_ctx* ctx, nalo_depth_image_args* args);

/* Sharded tracker (the reference's analogue is the per-thread sum of calcGSSSE, CoarseTracker.cpp:828-885): with world > 1 every rank evaluates
 * points [n rank / world, n (rank + 1) / world) of every pyramid level and the 52 sums of an evaluation (45 H entries, E and the six counters, as doubles) are summed
 * over the ranks by hook(user, device_buf, 52) - same contract as nalo_ba_set_allreduce; stream_ordered != 0: the hook enqueues on nalo_stream(ctx) and returns.
 * nalo_trk_set_ref stays replicated (every rank passes all reference points). nalo_trk_eval and nalo_trk_track both honour it; nalo_trk_track then runs its
 * host-driven LM loop (one launch + one all-reduce per evaluation), every rank ends with the same pose. world = 1 switches it off. */
typedef void (*nalo_allreduce_fn)(void* user, double* device_buf, int n);
int nalo_trk_set_shard(nalo_ctx* ctx, int rank, int world, nalo_allreduce_fn hook, void* user, int stream_ordered);

/* a3+a4 fused  CoarseTracker::calcRes (CoarseTracker.cpp:891-1049) + calcGSSSE (:828-885), call sites
 * CoarseTracker.cpp:1104,1109,1115,1184,1204. R,t = refToNew; affLL = fromToVecExposure(ref,new) as float;
 * b0 = lastRef_aff_g2l.b. stats6 = {E, numTermsInE, shiftT/(n+.1), 0, shiftRT/(n+.1), saturatedRatio}.
 * If want_gs: H (8x8) and b (8) as calcGSSSE returns them (divided by the PADDED count, scaled by SCALE_*). */
int nalo_trk_eval(nalo_ctx* ctx, int slot_new, int lvl, const double R[9], const double t[3],
                  const float affLL[2], float b0, float cutoffTH, int want_gs,
                  double stats6[6], double H[64], double b[8]);

/* CoarseTracker::trackNewestCoarse (CoarseTracker.cpp:1073-1259), call site FullSystem.cpp:594-597.
 * T_io = lastToNew_out, aff_io = aff_g2l_out (a,b), ref_aff = lastRef_aff_g2l, exposures = {ref,new}.
 * *ok = the bool the reference returns. n_evals (optional) = number of fused evaluations launched. */
int nalo_trk_track(nalo_ctx* ctx, int slot_new, double T_io[12], double aff_io[2], const double ref_aff[2],
                   const float exposures[2], int coarsestLvl, const double minResForAbort[5],
                   double lastResiduals[5], double lastFlowIndicators[3], int* ok, int* n_evals);

/* measurement aid: LM evaluations per pyramid level (evals[l]) and point-cloud sizes (n[l]) of the last nalo_trk_track; the algorithmic bytes of that frame are
 * sum_l evals[l] * n[l] * 64 B. Either array may be NULL. An evaluation is one calcRes: the first one of a level, its cutoff repeats and every LM
 * candidate; a level re-run through haveRepeated adds both runs to its entry. */
int nalo_trk_last_evals(nalo_ctx* ctx, int evals[5], int n[5]);
/* how the last nalo_trk_track ran (read only, no side effect): {lanes per workgroup, workgroups, driver (1: the persistent LM kernel, 2: the host-driven loop,
 * 0: no track yet), rounds per level 0..4 (ceil(n_l / (workgroups * lanes)): 1 = the level's points stay in registers for all its evaluations; 0 for levels
 * not run), haveRepeated (a level was re-run)}. With the host-driven loop only the driver and haveRepeated are set. */
int nalo_trk_get_launch_config(nalo_ctx* ctx, int cfg[9]);

/* FullSystem::trackNewCoarse's loop over motion hypotheses (FullSystem.cpp:595-666) in ONE call: the tries run one after the other, each bounded by the best
 * residuals so far, with every decision of the loop taken on the device inside one persistent launch (driver 1). Literally:
 *   achievedRes = five NaNs; for each try i: T = tries[i], aff = aff_init, trackNewestCoarse(T, aff, coarsestLvl, minResForAbort = achievedRes), including its
 *   tail (CoarseTracker.cpp:1239-1256); taken when ok && isfinite((float)lastRes[0]) && !(lastRes[0] >= achievedRes[0]) (:633); once a try has been taken,
 *   after EVERY try achievedRes[l] takes over lastRes[l] where it is not finite (as float) or larger (:643-650); the loop ends at
 *   have_one_good && achievedRes[0] < lastCoarseRMSE[0] * (double)reTrackThreshold (:653).
 *   No good try (:658-664): T = tries[0], aff = aff_init, flow = 0, winner = -1, achievedRes stays NaN - and is still written to lastCoarseRMSE_io, as the
 *   reference does (its next frames then never leave the loop early until one tracks).
 * lastCoarseRMSE_io: in, the caller's FullSystem::lastCoarseRMSE (only [0] is read); out, achievedRes (:666). firstCoarseRMSE and the shell update stay with
 * the caller. reTrackThreshold <= 0 (or NaN): the compiled-in setting_reTrackThreshold (1.5).
 * records (optional): min(try_iterations, records_cap) entries, one per try that ran, in order. T / aff of a record: what the try wrote (:1239-1240, also when
 * the tail then returned false); its input when it aborted on minResForAbort (:1227, abort_lvl >= 0), as nalo_trk_track leaves T_io untouched then.
 * driver: 1 = one persistent launch; 2 = the literal loop over nalo_trk_track's host-driven form: a sharded tracker, a fixed affine parameter
 * (affineOptModeA / B < 0), a context that lost a workgroup earlier - or in this call: the WHOLE list is then redone from the host and the context keeps to
 * the host-driven loop, as with nalo_trk_track. Both drivers honour the same outputs contract. One call over K tries gives the bits of K nalo_trk_track calls
 * driven by the loop above. nalo_trk_last_evals afterwards: the sums over the tries that ran.
 * Refusals, each before anything is queued, leaving every output, lastCoarseRMSE_io and the context untouched: NALO_ERR_ARG for a NULL ctx / args / tries,
 * n_tries < 1 or > NALO_TRK_MAX_TRIES, a non-finite entry of tries, records_cap < 0 or records == NULL with records_cap > 0, coarsestLvl or slot_new out of
 * range; NALO_ERR_STATE / NALO_ERR_HIP where nalo_trk_track returns them (no reference, an empty slot; a failed cross-rank exchange).
 * n_tries < 1: the reference's allFrameHistory.size() == 2 branch builds an EMPTY list and then indexes it; pass one identity instead, as
 * upstream DSO does (nalo_trk_motion_tries with poses_valid = 0 writes it). */
#define NALO_TRK_MAX_TRIES 64
typedef struct nalo_trk_try_record {
    int ok;                      /* the bool trackNewestCoarse returned */
    int taken;                   /* this try became the winner (:633) */
    int abort_lvl;               /* level whose residual exceeded 1.5 * achievedRes (:1227); -1: none */
    int have_repeated, n_evals;
    int evals[5];                /* evaluations per level of this try */
    double lastResiduals[5], flow[3], T[12], aff[2];
} nalo_trk_try_record;
typedef struct nalo_trk_tries_args {
    int slot_new, n_tries, coarsestLvl;
    const double* tries;         /* n_tries x 12, row-major [R|t]: lastF_2_fh_tries */
    double aff_init[2];          /* aff_last_2_l: every try starts from it (:602) */
    double ref_aff[2];
    float  exposures[2];         /* {ref, new} */
    double lastCoarseRMSE_io[5];
    double reTrackThreshold;
    /* out */
    double T[12], aff[2], flow[3], achievedRes[5];
    int have_one_good, try_iterations, winner;
    int driver;
    nalo_trk_try_record* records; int records_cap;
} nalo_trk_tries_args;
int nalo_trk_track_tries(nalo_ctx* ctx, nalo_trk_tries_args* args);

/* The hypothesis list of FullSystem::trackNewCoarse (FullSystem.cpp:535-572), in the reference's order: constant motion, double motion, half motion
 * (exp(0.5 log)), zero motion, identity, then the 26 variants constant_motion * SE3(Quaterniond(1, +-d, +-d, +-d)), d = 0.02, the quaternion normalised as
 * Sophus' constructor does (the reference's `rotDelta++` loop runs once: SURVEY App. C.8). Inputs: slast_2_sprelast and lastF_2_slast as row-major [R|t].
 * poses_valid == 0: the single identity of :575-579. Returns the count (31 or 1), written to out as count x 12; NALO_ERR_ARG for a NULL pointer. Host code. */
int nalo_trk_motion_tries(const double slast_2_sprelast[12], const double lastF_2_slast[12], int poses_valid, double out[31 * 12]);

/* ------------------------------------------------------------------------------------------------
 * Back-end: sliding-window photometric bundle adjustment.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_frame_state {
    int slot;                 /* frame slot holding the pyramid (nalo_frame_upload) */
    int frame_id;             /* FrameHessian::frameID (0 gets the gauge priors, HessianBlocks.h:321-350) */
    double worldToCam_evalPT[12];
    double state[10];         /* FrameHessian::state (unscaled); [0:6] relative to evalPT, [6:8] = a,b / SCALE */
    double state_zero[10];
    float ab_exposure;
    float frameEnergyTH;
} nalo_frame_state;

/* EnergyFunctional::insertFrame / FullSystem::setPrecalcValues / EnergyFunctional::setAdjointsF, setDeltaF
 * (OptimizationBackend/EnergyFunctional.cpp:429-461, 46-106, 171-194; FullSystem.cpp:1694-1704).
 * The newest keyframe must be the last entry (frameHessians.back()). calib = {fx,fy,cx,cy} value_scaled. */
int nalo_ba_set_window(nalo_ctx* ctx, int W, const nalo_frame_state* frames, const double calib[4],
                       const double calib_zero[4]);
/* EnergyFunctional::insertPoint (EnergyFunctional.cpp:462-474) for all active points: SoA, P entries.
 * color/weights are P x 8 (PointHessian::color/weights, HessianBlocks.h:424-425). idepth_zero may be NULL (= idepth). */
int nalo_ba_set_points(nalo_ctx* ctx, int P, const int* host, const float* u, const float* v,
                       const float* idepth, const float* idepth_zero, const float* color, const float* weights,
                       const int* has_depth_prior);
/* EnergyFunctional::insertResidual (EnergyFunctional.cpp:417-428): exists[p*W + t] != 0 creates the
 * PointFrameResidual (point p -> target frame t) in the resetOOB state (FullSystem/Residuals.h:88-94). */
int nalo_ba_set_residuals(nalo_ctx* ctx, const uint8_t* exists);
/* marginalisation prior HM/bM ((8W+4)^2, 8W+4), EnergyFunctional.h; NULL = zero */
int nalo_ba_set_prior(nalo_ctx* ctx, const double* HM, const double* bM);
int nalo_ba_get_prior(nalo_ctx* ctx, double* HM, double* bM);

/* a5+a6 (+ the accumulation side of a7, a9)  FullSystem::linearizeAll(fix) + applyRes_Reductor
 * (FullSystem/FullSystemOptimize.cpp:144-211, 90-94, call sites :436,:460,:511,:524,:562) =
 * PointFrameResidual::linearize + applyRes + EFResidual::takeDataF (Residuals.cpp:78-274,306-328,
 * EnergyFunctionalStructs.cpp:39-50) + setNewFrameEnergyTH (:95-143). Valid because
 * setting_forceAceptStep=true (util/settings.cpp:71): every linearisation is committed.
 * energy = lastEnergyP (the stats[0] sum). fix != 0 drops residuals that are not IN, as linearizeAll(true). */
int nalo_ba_linearize(nalo_ctx* ctx, int fix, double* energy);
/* a7+a8  EnergyFunctional::accumulateAF_MT (mode 0) / accumulateLF_MT (mode 1)  (EnergyFunctional.cpp:197-238,
 * call sites :788,:791): stitched H ((8W+4)^2) and b. Mode 1 adds the priors (usePrior=true); linearised
 * residuals never exist at this call in the reference flow (they live only inside flagPointsForRemoval ->
 * marginalizePointsF, FullSystem.cpp:975-990,1453) so mode 1 carries priors only. */
int nalo_ba_accumulate(nalo_ctx* ctx, int mode, double* H, double* b);
/* a9+a10  EnergyFunctional::accumulateSCF_MT (EnergyFunctional.cpp:244-261, call site :795) */
int nalo_ba_accumulate_sc(nalo_ctx* ctx, int shiftPriorToZero, double* H_sc, double* b_sc);
/* a11+a12  EnergyFunctional::solveSystemF (EnergyFunctional.cpp:776-914, call site FullSystemOptimize.cpp:616):
 * accumulate A, L, SC; assemble; Jacobi-scaled LDL^T; orthogonalise x for iteration >= 2; resubstituteF_MT.
 * x_out (8W+4) optional. */
int nalo_ba_solve_system(nalo_ctx* ctx, int iteration, double lambda, double* x_out);
/* FullSystem::backupState + doStepFromBackup (FullSystemOptimize.cpp:304-349, 217-299) */
int nalo_ba_backup_state(nalo_ctx* ctx);
int nalo_ba_do_step(nalo_ctx* ctx, float stepfacC, float stepfacT, float stepfacR, float stepfacA, float stepfacD,
                    int* canbreak);
/* FullSystem::optimize (FullSystemOptimize.cpp:398-602, call site FullSystem.cpp:1362). never_break != 0 disables
 * the early exit at :544 so a benchmark keyframe always runs mnumOptIts iterations. */
int nalo_ba_optimize(nalo_ctx* ctx, int mnumOptIts, int never_break, double* rmse);
/* a13  EnergyFunctional::calcLEnergyF_MT + calcLEnergyPt (EnergyFunctional.cpp:332-415) and calcMEnergyF (:320-329) at the CURRENT states, as
 * FullSystem::calcLEnergy / calcMEnergy return them when setting_forceAceptStep is false (FullSystemOptimize.cpp:351, 371-379; they return 0 otherwise —
 * these two entry points always compute). L = frame priors + calibration prior + per point deltaF^2 priorF (device reduction); the inner loop of
 * calcLEnergyPt runs over linearised residuals, which never exist while optimize() runs (they live only inside nalo_ba_marginalize_points).
 * M = delta . (2 bM + HM delta) on the host in fp64. *rejected (nalo_ba_optimize_stats) = steps the last nalo_ba_optimize restored from the backup. */
int nalo_ba_calc_l_energy(nalo_ctx* ctx, double* E);
/* planeOpt=1, call sites FullSystem.cpp:1440-1441, without Ceres:
 * nalo_ba_plane_scale_fix    FullSystem::planeOptimize's active part (FullSystem/PlaneOptimize.cpp:183-301) for the newest keyframe: camToWorld =
 *     trackingRef.camToWorld * [R | localscale * t](camToTrackingRef), its own points' idepth /= localscale (idepth_zero alike), setEvalPT at the new pose, adjoints,
 *     precalc. localscale = getlocalgh() / groundP[3] is the caller's (nalo_ground_local_scale on the state nalo_trk_fit_ground + nalo_ground_update keep, or a RANSAC of its own); the caller skips the call when scaleFixed / no ground.
 * nalo_ba_sw_gray_optimize   FullSystem::SWGrayOptimize_J (:307-454). The reference's Ceres cost functor multiplies every Jacobian by an image gradient it never
 *     reads (a shadowed variable, PlaneOptimize.h:378-381): the gradient is identically zero, Ceres returns its initial point. The call therefore
 *     (a) evaluates the Huber(100) cost 1/2 sum rho(r^2) over all (point, target != host) centre-pixel residuals with 1e-4 <= idepth <= 1e3 on the device
 *     (*cost, *n_residual_blocks: what Ceres' summary reports as initial = final cost), and (b) applies the post-solve state changes with the unchanged
 *     parameters: newest frame PRE_worldToCam = [exp(log R) | t] and re-linearised there, idepth_zero = idepth for the points of frames 0 .. W-3, adjoints and
 *     precalc values recomputed. Read the result with nalo_ba_get_frames / nalo_ba_get_points. */
int nalo_ba_plane_scale_fix(nalo_ctx* ctx, double localscale, const double camToTrackingRef[12], const double trackingRef_camToWorld[12]);
int nalo_ba_sw_gray_optimize(nalo_ctx* ctx, double* cost, int* n_residual_blocks);
int nalo_ba_calc_m_energy(nalo_ctx* ctx, double* E);
int nalo_ba_optimize_stats(nalo_ctx* ctx, int* iterations, int* rejected);
/* a13 + a7<2> + a9  flagPointsForRemoval's relinearise/fixLinearizationF (FullSystem.cpp:975-990,
 * EnergyFunctionalStructs.cpp:89-115) + EnergyFunctional::marginalizePointsF (EnergyFunctional.cpp:615-676).
 * flags[p] != 0 marks PS_MARGINALIZE. Adds 0.25*(M - Msc) into HM/bM and removes the points.
 * M, Mb, Msc, Mbsc (optional outputs) are the stitched systems. */
int nalo_ba_marginalize_points(nalo_ctx* ctx, const uint8_t* flags, double* M, double* Mb, double* Msc, double* Mbsc);

/* The point lifecycle of FullSystem::makeKeyFrame between optimize() and marginalizeFrame, resident on the device.
 *
 * nalo_ba_set_point_history / nalo_ba_get_point_history   what the decisions read besides the residuals, per point in submission order:
 *     numGood          PointHessian::numGoodResiduals (FullSystem/HessianBlocks.h:452), an int at full range
 *     last_target[2]   the window index of the frame lastResiduals[k].first targets (HessianBlocks.h:476; [0] = latest), -1 when .first == 0
 *     last_state[2]    lastResiduals[k].second: 0 IN, 1 OOB, 2 OUTLIER
 *   Call nalo_ba_set_point_history after nalo_ba_set_residuals. numGood NULL = zeros. last_target and last_state NULL (both) = what optimizeImmaturePoint leaves
 *   on a freshly activated point (FullSystemOptPoint.cpp:173-199): [0] = (W-1, IN) if the residual to frame W-1 exists, else (-1, OOB); [1] alike for W-2.
 *   The shift at keyframe insertion ([1] = [0]; [0] = (new residual, IN), FullSystem.cpp:1344-1345) is the caller's, who re-issues the window there anyway.
 *   While the window carries a history every linearizeAll(true) - nalo_ba_linearize(fix = 1) and the final pass of nalo_ba_optimize - updates it once:
 *   numGood += the point's residuals that end the pass active (FullSystemOptimize.cpp:63-77; isNew is never cleared in this fork, Residuals.cpp:72),
 *   last_state[k] = state_state of the residual last_target[k] names when it took part in the pass (:172-179), last_target[k] = -1 when the pass removed
 *   it (:187-194). nalo_ba_marginalize_frame(idx) remaps the targets (== idx -> -1, > idx -> one down: FullSystemMarginalize.cpp:174-177; read them back
 *   before the next nalo_ba_set_points); nalo_ba_snapshot / nalo_ba_restore include the history; nalo_ba_set_points drops it.
 *   A pointer to a residual that has been deleted is kept as -1: it compares unequal to every live residual, which is all the reference does with it. So
 *   where last_target[0] == last_target[1] (the ABI allows it, the reference never produces it) and a pass removes that residual, BOTH become -1, where the
 *   reference's else-if (FullSystemOptimize.cpp:191-194) would leave [1] dangling; last_state[1] is not rewritten in that case, as in the reference.
 *
 * nalo_ba_flag_points   removeOutliers' predicate (FullSystemOptimize.cpp:631-653) and FullSystem::flagPointsForRemoval (FullSystem.cpp:937-1031) with
 *   PointHessian::isOOB / isInlierNew (HessianBlocks.h:484-514), one kernel. frame_flagged[W] = FrameHessian::flaggedForMarginalization. Per point
 *   (all outputs optional, submission order): decision 0 keep, 1 drop (idepth_scaled < 0 or no residuals), 2 drop, 3 marginalise; idepth_hessian = the
 *   float PointHessian::idepth_hessian that is compared with setting_minIdepthH_marg: H of AccumulatedSCHessianSSE::addPoint at the last accumulation
 *   (AccumulatedSCHessian.cpp:36-50), 0 when the point had no active residual then - NOT 1 / HdiF, which is rounded twice. counts[W][4] = {kept,
 *   drop (no residuals), drop, marginalised} of every host: the addends of flagFramesForMarginalization's in / out (FullSystemMarginalize.cpp:76-77).
 *   idepth_hessian is that of the last accumulation: after nalo_ba_optimize its last solveSystemF's; after an explicit nalo_ba_linearize the accumulation
 *   of that linearisation, which the call runs itself if nalo_ba_get_points / nalo_ba_accumulate_sc have not yet.
 *   The decisions stay on the device. Needs a history (NALO_ERR_STATE without one). On a sharded window the call is local to the rank's points.
 *
 * nalo_ba_marginalize_flagged   nalo_ba_marginalize_points for the points nalo_ba_flag_points decided to marginalise (EnergyFunctional::marginalizePointsF,
 *   EnergyFunctional.cpp:615-676), then dropPointsF / removePoint (:678-714) of all three removed classes on the device: no residual state crosses the bus. */
int nalo_ba_set_point_history(nalo_ctx* ctx, const int* numGood /* P */, const int8_t* last_target /* P x 2 */, const int8_t* last_state /* P x 2 */);
int nalo_ba_get_point_history(nalo_ctx* ctx, int* numGood, int8_t* last_target, int8_t* last_state);
int nalo_ba_flag_points(nalo_ctx* ctx, const uint8_t* frame_flagged /* W */, uint8_t* decision /* P */, float* idepth_hessian /* P */, int* counts /* W x 4 */);
int nalo_ba_marginalize_flagged(nalo_ctx* ctx, double* M, double* Mb, double* Msc, double* Mbsc);

/* EnergyFunctional::marginalizeFrame (OptimizationBackend/EnergyFunctional.cpp:498-610), call site FullSystem::marginalizeFrame
 * (FullSystem/FullSystemMarginalize.cpp:155). Host fp64 on HM/bM: the frame `idx` (window index) is permuted to the end, its prior is added,
 * the scaled 8x8 block is inverted and eliminated by a Schur complement; HM/bM shrink to 8(W-1)+4. The frame must not host active points any more
 * (the reference asserts it: marginalise or drop them with nalo_ba_marginalize_points / by not re-submitting them). The frame leaves the window:
 * W decreases by one, nalo_ba_get_frames / nalo_ba_get_prior return the remaining frames, and the device window must be re-issued with
 * nalo_ba_set_window (+ set_points, set_residuals), or carried with nalo_ba_carry_window, before the next linearisation — FullSystem::marginalizeFrame likewise drops every residual
 * that targets the frame and recomputes the precalc values and adjoints (:161-212). The shrunk HM/bM are handed to exactly that NEXT nalo_ba_set_window:
 * kept if it names the remaining frames, extended by a zero block if it appends one keyframe (EnergyFunctional::insertFrame, :437-442); any other size
 * resets the prior to zero.
 * Prior ownership in general: nalo_ba_set_window starts from a ZERO prior unless (a) it directly follows nalo_ba_marginalize_frame (above) or (b) the context
 * was declared one continuing EnergyFunctional with nalo_ba_set_prior_carry(ctx, 1): then every nalo_ba_set_window keeps HM/bM (same frames) or extends them
 * (one frame appended), as the reference's single EnergyFunctional does over a session. A caller that keeps HM/bM itself needs neither:
 * it calls nalo_ba_set_prior after every nalo_ba_set_window. */
int nalo_ba_marginalize_frame(nalo_ctx* ctx, int idx);
int nalo_ba_set_prior_carry(nalo_ctx* ctx, int on);

/* The seam between two keyframes on the device: the window re-issued from what is resident, instead of nalo_ba_get_* -> nalo_ba_set_window + nalo_ba_set_points
 * + nalo_ba_set_residuals + nalo_ba_set_point_history. The result is, in everything a caller can read or compute from, the window that re-issue would build.
 *
 * nalo_ba_carry_window(ctx, entering, insert_activated)
 *   Frames    those nalo_ba_get_frames returns now, in their order - what remains after any number of nalo_ba_marginalize_frame calls since the last issue -
 *             with their host state (evalPT, state, state_zero, frameEnergyTH); `entering` (NULL: none) is appended as the newest frame
 *             (EnergyFunctional::insertFrame, EnergyFunctional.cpp:429-461). HM / bM are always kept, and extended by a zero block for an entering frame;
 *             the CalibHessian continues (value and value_zero as they are). Adjoints and precalc values are recomputed as nalo_ba_set_window does.
 *             More than NALO_MAX_WINDOW frames: NALO_ERR_ARG. An entering slot without a pyramid: NALO_ERR_STATE.
 *   Points    the valid points in their old submission order, renumbered densely, each with u, v, idepth, idepth_zero, color, weights and its depth-prior flag.
 *             A frame that left must host no valid point (nalo_ba_marginalize_frame sees to it on its first call; NALO_ERR_STATE otherwise).
 *   Residuals a carried point keeps the residual to target t iff it has one now and t remains; with an entering frame every carried point gets one to it
 *             (FullSystem.cpp:1335-1348). All come out as nalo_ba_set_residuals leaves them (IN, energies zero, resetOOB); accumulators, steps, backups and
 *             relBS are zero as after nalo_ba_set_points; decisions of a nalo_ba_flag_points nobody consumed are dropped.
 *   History   (a window that carries one) numGood and both last_* pairs are carried - the targets as nalo_ba_marginalize_frame remapped them -, and with an
 *             entering frame shifted: [1] = [0]; [0] = (W_new - 1, IN) (FullSystem.cpp:1344-1345).
 *   insert_activated != 0   step 4 of activatePointsMT (FullSystem.cpp:893-917) with the tail of optimizeImmaturePoint (FullSystemOptPoint.cpp:170-200) for the
 *             last nalo_imm_resident_activate that was asked for its optimisation outputs: every selected point k with result[k] == 1 becomes a window point
 *             behind the carried ones, in toOptimize order; host = its host_idx; u, v, color, weights from the resident immature record (read on the device);
 *             idepth = idepth_zero = idepth_out[k]; no depth prior; a residual to t iff res_in[k][t]; the history of a fresh point (numGood 0, the defaults
 *             above). The resident immature set is not modified. The pending result is consumed by this call and dropped by nalo_imm_resident_set, a later
 *             activation, nalo_ba_set_window and nalo_ba_set_points. NALO_ERR_STATE when none is pending, when the window's frames (or points) changed since
 *             the activation, or together with an entering frame (the reference appends the frame, activates, then inserts: two calls).
 *   Layout    exactly nalo_ba_set_points' for the new point list (one shared function): slot order per host in stable Hilbert-cell order - a new point is merged
 *             between carried ones -, padding, block tables, work distribution, partial sizes; nalo_ba_get_launch_config reports it. nalo_trk_set_ref_from_window's
 *             map and the snapshot are invalidated: nalo_ba_restore after a carry gives NALO_ERR_STATE.
 *   Allowed with points and residuals set, or with them unset only because nalo_ba_marginalize_frame was called since the last issue (the device arrays still
 *             stand). Refused with NALO_ERR_STATE on a sharded window and on a context whose exchange failed. A refusal leaves the window as it was.
 *   Bus       per call the two integer maps and the block tables go down in stream-ordered copies from pinned memory: 4 bytes per new slot for the map,
 *             under 5 with the tables (at most 8). Nothing comes up, no float array of points or residuals goes either way, and the call does not wait for
 *             the stream. In steady state it allocates nothing: the gather writes a second set of buffers that then changes places with the first.
 * nalo_ba_carry_map   old_p[p_new] = the submission index before the last carry, or -(k + 1) for the k-th selected point of the activation: what the caller
 *             re-keys its PointHessian objects with.
 * nalo_ba_carry_last  {points carried, points inserted, P_new, Ppad_new} of the last carry. */
int nalo_ba_carry_window(nalo_ctx* ctx, const nalo_frame_state* entering /* NULL: none */, int insert_activated);
int nalo_ba_carry_map(nalo_ctx* ctx, int* old_p /* P_new */);
int nalo_ba_carry_last(nalo_ctx* ctx, int stats[4]);

/* The beginning of that chain: the first window issued from the initialiser's level-0 points on the device, instead of nalo_init_get_points -> the host loop of
 * FullSystem::initializeFromInitializer (FullSystem.cpp:1567-1654) -> nalo_imm_create -> nalo_ba_set_window + nalo_ba_set_points + nalo_ba_set_residuals +
 * nalo_ba_set_point_history. A window holds at least two frames, and the reference inserts the second one right after initializeFromInitializer
 * (deliverTrackedFrame(fh, true) -> makeKeyFrame, FullSystem.cpp:1327-1348): the call does both steps and issues the window {firstFrame, newFrame}. The result is,
 * in everything a caller can read or compute from, the window that re-issue would build. Arithmetic is the reference's, operation for operation.
 *
 * nalo_ba_window_from_initializer(ctx, a)
 *   Scale     (:1589-1595) on the initialiser's current level-0 state (the host mirror is uploaded first when it is the newer side): sumID = 1e-5f, then
 *             sumID += iR[i] for i = 0 .. n-1 in float and in index order - one wave on the device, no tree and no atomics, the bits are the sequential loop's -;
 *             numID = 1e-5f, then += 1 n times in float; rescaleFactor = 1 / (sumID / numID).
 *   Keep rule (:1598, 1607) keepPercentage = desired_point_density / n (float / int); point i is skipped iff (float)draws[i] / 2147483648.0f > keepPercentage.
 *             draws[i] is the rand() of the caller's libc stream that the reference consumes for point i: every level-0 point consumes exactly one, in index
 *             order, whatever becomes of it. 2147483648.0f is (float)RAND_MAX of a libc with 31-bit rand(); other values of RAND_MAX are the caller's to rescale.
 *   Points    (:1610-1626) a kept point i is constructed at ui = (int)(u[i] + 0.5f), vi = (int)(v[i] + 0.5f) on level 0 of first.slot as the slot holds it at call
 *             time (ImmaturePoint::ImmaturePoint, as nalo_imm_create) and rejected when its energyTH is not finite. The others become window points in index
 *             order: host 0, u = (float)ui, v = (float)vi, color and weights from the constructor, idepth = idepth_zero = iR[i] * rescaleFactor (the idepth of
 *             nalo_ba_set_points), the depth prior set. Layout: exactly nalo_ba_set_points' for that point list (one shared function).
 *   Frames    (:1631-1648, setEvalPT_scaled) first: worldToCam_evalPT = identity; entering: thisToNext with its translation divided by rescaleFactor (promoted to
 *             double), inverted to camToWorld and inverted again; state = state_zero = 0 for both. slot, frame_id, ab_exposure and frameEnergyTH are the caller's;
 *             evalPT, state and state_zero are written back into *a. calib / calib_zero as nalo_ba_set_window; HM / bM start at zero whatever
 *             nalo_ba_set_prior_carry says; adjoints and precalc values as nalo_ba_set_window computes them.
 *   Residuals (:1335-1348) every point gets one residual, to frame 1, as nalo_ba_set_residuals leaves it.
 *   History   numGood = 0, last_target = {1, -1}, last_state = {IN, IN}. The IN of entry [1] is the reference's: PointHessian never initialises lastResiduals, so
 *             the pair is value-initialised to (0, ResState(0) = IN) and then shifted - not the (-1, OOB) nalo_ba_set_point_history's NULL default gives.
 *   The initialiser is not modified; a second call gives the same window. nalo_init_set_first must have been called; `snapped` is the caller's decision.
 *   Bus       no float array of points or residuals crosses in either direction. Up: one byte per level-0 point (the non-finite rejections) and sumID, in one
 *             copy the call waits for - its only wait besides what nalo_ba_set_window's frame half does -; down: the integer map (4 bytes per window slot) and
 *             the block tables, stream-ordered from pinned memory as in nalo_ba_carry_window.
 *   NALO_ERR_ARG: a NULL argument; n_draws != numPoints[0]; desired_point_density not finite or <= 0; first.slot is not the initialiser's first slot;
 *             first.slot == entering.slot. NALO_ERR_STATE: no initialiser; an entering slot without a pyramid; no point kept; a sharded context; a context
 *             whose exchange failed. A refused call leaves the context's window exactly as it was.
 * nalo_ba_init_window_map    src[p] = the level-0 index of window point p (submission order; strictly increasing).
 * nalo_ba_init_window_last   scale = {sumID, numID, rescaleFactor}, stats = {n, skipped by their draw, rejected as non-finite, P} of the last call; either may be NULL. */
typedef struct nalo_init_window_args {
    nalo_frame_state first, entering;  /* in: slot, frame_id, ab_exposure, frameEnergyTH.  out: worldToCam_evalPT, state, state_zero as the call set them */
    double calib[4], calib_zero[4];    /* as nalo_ba_set_window */
    float desired_point_density;       /* setting_desiredPointDensity */
    int n_draws; const int* draws;     /* draws[i] = rand() of the caller's libc stream, one per level-0 point, in index order (FullSystem.cpp:1607) */
} nalo_init_window_args;
int nalo_ba_window_from_initializer(nalo_ctx* ctx, nalo_init_window_args* a);
int nalo_ba_init_window_map(nalo_ctx* ctx, int* src /* P: level-0 index of window point p, submission order */);
int nalo_ba_init_window_last(nalo_ctx* ctx, float scale[3] /* sumID, numID, rescaleFactor */, int stats[4] /* n, skipped by draw, rejected non-finite, P */);

/* read-back of window state (host pointers, any may be NULL) */
int nalo_ba_get_frames(nalo_ctx* ctx, nalo_frame_state* frames /* W */, double* worldToCam /* W x 12 PRE_worldToCam */,
                       double calib[4]);
/* Hdd_accAF / bd_accAF / Hcd_accAF / HdiF / bdSumF are values of the last ACCUMULATION, as in the reference (addPoint<0>, AccumulatedSCHessianSSE::addPoint):
 * after nalo_ba_optimize those of its last solveSystemF — what CoarseTracker::makeCoarseDepthL0 reads as HdiF (CoarseTracker.cpp:396), so read them
 * BEFORE nalo_ba_marginalize_points (which re-accumulates); after an explicit nalo_ba_linearize the accumulation of that linearisation is run on demand. */
int nalo_ba_get_points(nalo_ctx* ctx, float* idepth, float* step, float* HdiF, float* bdSumF, float* Hdd_accAF,
                       float* bd_accAF, float* Hcd_accAF /* P x 4 */, float* maxRelBaseline);
/* PointHessian::idepth_zero of every point (the linearisation point SWGrayOptimize_J / loadSateBackup / doStepFromBackup move) */
int nalo_ba_get_idepth_zero(nalo_ctx* ctx, float* idepth_zero);
/* per residual slot [p*W + t]: state (-1 none, 0 IN, 1 OOB, 2 OUTLIER), active flag, JpJdF (8), state_NewEnergyWithOutlier,
 * centerProjectedTo (3) */
int nalo_ba_get_residuals(nalo_ctx* ctx, int8_t* state, uint8_t* active, float* JpJdF, float* energy_new,
                          float* center_projected);
/* per (host,target) bin 13x13 accumulator of the last linearisation (AccumulatorApprox::H, MatrixAccumulators.h:600),
 * index h + t*W, fp64 */
int nalo_ba_get_acc13(nalo_ctx* ctx, double* H13 /* W*W x 169 */);
int nalo_ba_counts(nalo_ctx* ctx, int* resInA, int* resInL, int* resInM);
/* the kernel variants the window setup chose (read only, no side effect): {nblocks, Ppad, lin_sub, sc_split, sc_bpw, T,
 * precalc records pulled by a kernel (0/1), threshold by the radix select (0/1), back-substitution mode (1: xAd as kernel
 * arguments, 2: built on the device from x), eligible for the pre-launch of optimize() (0/1)} */
int nalo_ba_get_launch_config(nalo_ctx* ctx, int cfg[10]);

/* bench/test utility (no reference counterpart): snapshot / restore the mutable window state (idepths, residual states,
 * frame states, calibration, HM/bM) on the device, so the same synthetic keyframe can be replayed without host uploads */
int nalo_ba_snapshot(nalo_ctx* ctx);
int nalo_ba_restore(nalo_ctx* ctx);

/* multi-GPU: the active-point set is sharded by the caller (each rank sets only its points); the stitched
 * buffers {H_A, b_A, H_sc, b_sc, energy, counters} are summed across ranks through this hook before every solve (the replica sum of
 * AccumulatedTopHessian.h:144-149 across GPUs), and so are the three radix histograms of setNewFrameEnergyTH (FullSystemOptimize.cpp:95-143) after every
 * linearisation: the newest frame's energy threshold is the exact order statistic over ALL ranks' residuals, i.e. what one GPU holding the whole window
 * computes. Per pass the hook is called THREE times, in the same order on every rank: level A and level B of the radix select (1024 doubles each: 2048 bins, two
 * per double as a + b * 2^26; on the side stream when a side hook is set), then one buffer [stitched systems | tail | level C] (2 (8W+5)^2 + 2 W^2 + 5 doubles
 * padded to a multiple of 16, + 256) = 166 KB + 2 KB at W = 12; a pass whose systems are never fetched sums level C alone (256) when the threshold is next
 * needed; a second fetch of a pass (the Schur complement after the top system, or the reverse) sums ONLY the block it stitched - everything else already holds
 * the window's totals. buf is a DEVICE pointer to n doubles. hook == NULL = single GPU.
 * A hook returns nothing: when its collective fails it calls nalo_ba_exchange_failed(ctx, message) before returning (the built-in RCCL hooks of
 * nalo_ba_rccl_init do the same). The call that issued the hook and every later nalo_ba_* call of the context then return NALO_ERR_HIP - a rank must not
 * solve with sums the others never received; the window has to be rebuilt on a new context. */
/* nalo_allreduce_fn: declared with nalo_trk_set_shard above */
int nalo_ba_set_allreduce(nalo_ctx* ctx, nalo_allreduce_fn hook, void* user);
int nalo_ba_exchange_failed(nalo_ctx* ctx, const char* what);
/* stream_ordered = 1: the hook ENQUEUES its collective on nalo_stream(ctx) (e.g. ncclAllReduce(..., (hipStream_t)nalo_stream(ctx))) and returns
 * without waiting; the library then neither synchronises before nor after the hook. Default 0: the library synchronises the stream the buffer was
 * produced on before the call and the hook returns when the sum is complete. */
int nalo_ba_set_allreduce_mode(nalo_ctx* ctx, int stream_ordered);
/* optional, stream-ordered mode: a second hook that enqueues the same sum on nalo_side_stream(ctx). The histogram sums then run on the side stream,
 * under the Schur-complement / reduce / stitch kernels of the main stream, instead of in line before them. */
int nalo_ba_set_allreduce_side(nalo_ctx* ctx, nalo_allreduce_fn hook, void* user);
void* nalo_side_stream(nalo_ctx* ctx);
/* The native form of the exchange: the library calls ncclAllReduce (RCCL over xGMI) itself, stream-ordered on nalo_stream / nalo_side_stream — no
 * callback into the caller per Gauss-Newton iteration. librccl is opened with dlopen when the first of these is called (NALO_ERR_UNSUPPORTED if absent).
 *   nalo_rccl_unique_id    ncclGetUniqueId: rank 0 draws one id per communicator and ships it to the other ranks (MPI, a file, torch.distributed ...)
 *   nalo_ba_rccl_init      ncclCommInitRank for the main and (id_side != NULL) the side communicator on this context's device; collective over the ranks;
 *                          the context owns and destroys the communicators
 *   nalo_ba_set_rccl_comm  the same with ncclComm_t handles the caller owns (comm_side may be NULL: the histogram sums then run in line on the main
 *                          stream); comm_main == NULL returns to single-GPU operation
 * Two communicators because the stitched systems (main stream) and the two radix histograms of setNewFrameEnergyTH (side stream, under the
 * Schur-complement kernels) are in flight at the same time, and RCCL serialises the operations of one communicator. Call after nalo_ba_set_window. */
int nalo_rccl_unique_id(char id[128]);
int nalo_ba_rccl_init(nalo_ctx* ctx, int nranks, int rank, const char id_main[128], const char id_side[128]);
int nalo_ba_set_rccl_comm(nalo_ctx* ctx, void* comm_main, void* comm_side);
/* ncclCommCount of the context's two communicators (0 = none installed): the number of ranks the exchange REALLY spans, for a launcher to print beside the
 * number of processes it started (the per-thread replica count the reference sums over at stitch, AccumulatedTopHessian.h:144-149, is NUM_THREADS there). */
int nalo_ba_rccl_ranks(nalo_ctx* ctx, int* ranks_main, int* ranks_side);
/* The partition a sharded window uses: which of the P active points rank `rank` of `world` keeps. Every rank gets the same share of every
 * host frame (all (host, target) bins stay evenly populated) as a contiguous range of the host's points in Hilbert order of their 8x8-pixel cells — a
 * spatially compact part of the image, so a rank's texel gathers keep the locality of the unsharded window. keep[] (capacity P) receives the ascending
 * point indices; the return value is their number (< 0: NALO_ERR_ARG). Host code, needs no device. */
int nalo_shard_points(int P, int W, const int* host, const float* u, const float* v, int img_w, int img_h, int rank, int world, int* keep);

/* ------------------------------------------------------------------------------------------------
 * a14  DenseMapping::updateMap bbox scan + makeMap (FullSystem/MapPoint.cpp:300-310, 334-407), call site
 * FullSystem.cpp:1494. plane = (pi1..pi4) from nalo_dense_fit_planes or the caller's RANSAC. rect_out = {minx,maxx,miny,maxy}.
 * Outputs at most cap points in raster order; *n = count; *accept = the extent test of MapPoint.cpp:403.
 * ------------------------------------------------------------------------------------------------ */
int nalo_dense_make_map(nalo_ctx* ctx, int slot, const float plane[4], float mask_value, const double camToWorld[12],
                        int cap, int rect_out[4], int* out_u, int* out_v, float* out_idepth, float* out_color,
                        uint8_t* out_bgr, int* n, int* accept);

/* ------------------------------------------------------------------------------------------------
 * dense=1 / densemap=1: DenseMapping::makeMaskDistMap (FullSystem/MapPoint.cpp:445-513) + fitPlane (:522-584) on the device, for both call sites:
 * CoarseTracker.cpp:559,591 (nalo_trk_fit_planes) and MapPoint.cpp:261,280 (nalo_dense_fit_planes). The points are grouped by the mask value under them and a
 * plane is fitted to every group; the records come back in the reference's cluster order. One wait, at the end of the call; `draws` go down, cap records come up.
 *
 * Clustering - exact. For every input point xx = (int)u, yy = (int)v: the reference's `if(dx<0.5) xx = ix; else xx = ix++;` (:469-472) post-increments, so xx
 *   NEVER rounds up; reproduced. A point is a member when xx>2 && xx<w-2 && yy>2 && yy<h-2 (:477). The reference reads the mask BEFORE that test (out of bounds
 *   for a point outside the image); here the read is guarded and a point that fails the test has no mask value; a coordinate that is not finite or outside
 *   int's range fails the test. Two points share a cluster when their mask values compare equal as floats: -0 equals +0 (the record carries +0). DIFFERENCE: a
 *   point under a NaN mask value is dropped (in the reference every such point is a cluster of its own, NaN != NaN).
 *   Discovery order and member order are those of the reference's alternating sweeps (:482-505): cluster 1 is the value under the LAST member, its members in
 *   descending input index; cluster 2 the value under the FIRST remaining member, in ascending index; and so on alternating. The clusters are then ordered by
 *   size, descending (:509). DEFINED READ: the reference's std::sort leaves the order of equal sizes unspecified; here ties keep discovery order.
 *   More than 2048 clusters: NALO_ERR_UNSUPPORTED (REFUSED, not computed; *n_clusters holds their number).
 * Fit - a defined algorithm (PCL's RANSAC is unseeded: no fit can be compared with it bit for bit). All fp32, IEEE division and square root, no FMA:
 *   cloud     per member, in member order: X = (fxi*xx + cxi) / id, Y = (fyi*yy + cyi) / id, Z = 1 / id with Ki[0] = {fxi = 1/fx, cxi = -cx/fx, fyi = 1/fy,
 *             cyi = -cy/fy} of the context's level-0 calibration (fitPlane :542-543). A member with a coordinate that is not finite is left out of the cloud
 *             (:544-548) but stays in n and rect. fitted = 0 when n_cloud < max(min_points, 3) (:560).
 *   triplets  sample i over the m cloud points, d = draws[3i .. 3i+2]: i0 = d0 % m; i1 = d1 % (m-1), plus one if >= i0; i2 = d2 % (m-2), plus one if >= the
 *             smaller of i0, i1, then plus one if >= the larger. The caller owns the random stream (as nalo_pixsel_set_random); all clusters share it.
 *   model     n = (p1-p0) x (p2-p0), every product rounded; len = sqrtf((nx*nx + ny*ny) + nz*nz); a zero or non-finite len is a degenerate sample: it scores
 *             nothing and never wins (all samples degenerate: fitted = 0). (a, b, c) = n / len, d = -((a*x0 + b*y0) + c*z0).
 *   score     the cloud points with fabsf(((a*x + b*y) + c*z) + d) < threshold. ALL n_samples candidates are scored (PCL's adaptive stop only saves serial
 *             time); the first with the largest count wins: best_sample, inliers.
 *   refine    (setOptimizeCoefficients(true)) with more than 3 inliers: centroid and 3x3 scatter of the winner's inliers about it in fp64 from their fp32
 *             coordinates, the eigenvector of its smallest eigenvalue (cyclic Jacobi, fp64, on the device) normalised, signed so that its dot product with the
 *             sample normal is >= 0, dis_plane = -n . centroid; rounded to float at the end. With 3 inliers or fewer the sample model is the result.
 * nalo_trk_fit_planes   input: the level-0 cloud as it stands (pc_u, pc_v, pc_idepth, pc_n[0]); mask: the tracking reference's slot. append = 1 also runs the
 *   loop of CoarseTracker.cpp:582-666 on the device with the fitted planes, through the code of nalo_trk_append_plane_points: nothing with fewer than 4 clusters
 *   (:563); per cluster, in order: skipped when not fitted (:591), when its rect touches the border (:627: maxx>w-1||minx<1||maxy>h-1||miny<1) or when
 *   (int)mask_value == 0 (:635); else appended (the off-by-one slot included), `appended` = the growth of pc_n[0]. The clusters are formed before the first
 *   append, as in the reference. The ground choice by `score` (:609-625) is nalo_trk_fit_ground below: CoarseTracker::fitPlane, the one this call site uses,
 *   writes `score` on every path that returns true (:362-376); it is DenseMapping::fitPlane (MapPoint.cpp:522-584) that never does.
 * nalo_dense_fit_planes input: what updateMap collects for the window's frame host_frame (MapPoint.cpp:246-259): its valid window points in submission order
 *   with idepth, then the resident immature points with that host_idx in resident order with (idepth_max + idepth_min) * 0.5f; mask: the frame's slot. The caller
 *   loops nalo_dense_make_map over the fitted clusters as before, or calls nalo_dense_update_map, which does both. Read on the device; the slot map of the window's points (4 bytes per point) goes down once
 *   per issued point list, shared with nalo_trk_set_ref_from_window.
 * nalo_plane_fit_members the last completed call's member lists: cluster_of[i] = the record index of input point i or -1 (cap >= the input count), order = the
 *   members of cluster 0, then 1, ... each in the reference's vector order (sum of n entries): what clusters[i][k] held, for tests and callers that keep objects.
 * Refusals: NALO_ERR_STATE no level-0 cloud / no window or points; no mask in the slot; a sharded window (dense). NALO_ERR_ARG cap < the number of clusters
 *   (*n_clusters still reports the need; nothing is appended), n_samples < 1 or > 4096, draws == NULL, a negative or NaN threshold. A refused call leaves the
 *   cloud and the context usable.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_plane_cluster {
    float mask_value;      /* clusters[i][0][3] */
    int   n;               /* members after the border test */
    int   n_cloud;         /* members whose back-projection is finite (fitPlane's cloud) */
    int   rect[4];         /* minx, maxx, miny, maxy over the members' (xx, yy), CoarseTracker.cpp:597-607 */
    int   fitted;          /* 1: n_cloud >= min_points and at least one non-degenerate sample */
    float plane[4];        /* dir_vector, dis_plane (zeros when not fitted) */
    int   best_sample;     /* index of the winning triplet (-1 when not fitted) */
    int   inliers;         /* its count */
    int   appended;        /* tracker variant with append = 1: growth of pc_n[0] for this cluster, else 0 */
} nalo_plane_cluster;
typedef struct nalo_plane_fit_args {
    float threshold;       /* the reference's setDistanceThreshold(0.01) */
    int   min_points;      /* DenseMapping::fitPlane's 10 (MapPoint.cpp:560); CoarseTracker::fitPlane, the tracker's, has 20 (CoarseTracker.cpp:336) */
    int   n_samples;       /* triplets; PCL's SACSegmentation default of 50 iterations is the documented default */
    const uint32_t* draws; /* 3 * n_samples values of the caller's stream, shared by all clusters */
    int   append;          /* tracker variant only */
} nalo_plane_fit_args;
int nalo_trk_fit_planes(nalo_ctx* ctx, const nalo_plane_fit_args* args, int cap, nalo_plane_cluster* out, int* n_clusters);
int nalo_dense_fit_planes(nalo_ctx* ctx, int host_frame, const nalo_plane_fit_args* args, int cap, nalo_plane_cluster* out, int* n_clusters);
int nalo_plane_fit_members(nalo_ctx* ctx, int cap, int* cluster_of, int* order);

/* ------------------------------------------------------------------------------------------------
 * dense_track = 1 with setPlaneOptimize: the ground plane of setCoarseTrackingRef (CoarseTracker.cpp:582-625), the window points on it (:669-693) and the
 * scale_fix / scale_rate state machine it feeds (:696-816), then makeKeyFrame's global plane and local scale (FullSystem.cpp:1420-1443, 1911-1976;
 * PlaneOptimize.cpp:203-211). The device half is one call; the state machine is plain host C over caller-owned structs and needs no device.
 *
 * nalo_trk_fit_ground   nalo_trk_fit_planes(ctx, fit, cap, out, n_clusters) with the ground pass enqueued behind the refinement: records, member lists, appended
 *   cloud and *n_clusters are those of nalo_trk_fit_planes on the same inputs, bit for bit; still one wait, at the end; the call is the "last completed call" of
 *   nalo_plane_fit_members. All fp32, no FMA.
 *   score     (CoarseTracker::fitPlane :299-378) a cluster takes part iff fitted && n_cloud == n: fitPlane returns false on a member that does not back-project
 *             to finite values (:320-324) and on fewer than fit->min_points cloud points (:336 - 20 for the tracker, not DenseMapping's 10).
 *             mid_z = the float sum, IN MEMBER ORDER, of Z_k / (float)n (:332; a chain of dependent adds, run in order by one wave).
 *             score = 9999999.0f when n < 100 || mid_z < 0 || mask_value < 200 (:363-368), else ((a + c) * 1000.0f + fabsf(d) * 100.0f) + (float)(100 / n)
 *             with the reference's INTEGER 100 / n (1 at n == 100, 0 above). The `abs` of :373 and :615 is the float one: CoarseTracker.h includes <math.h> and
 *             <cstdlib> under `using namespace std`. DEFINED: x_axis . dir + z_axis . dir is a + c for finite planes.
 *   choice    (:574-625) nothing at all with fewer than 4 clusters (:563-567): pick->ran = 0 and NOTHING else is written (pick's other fields, scores, onground).
 *             Otherwise ran = 1 and the first cluster in record order with the strictly smallest score below FLT_MAX wins (a NaN score never wins, as with
 *             the reference's `<`; a cluster scored 9999999 can win): cluster = its record index or -1 when none took part; gp_raw = (-a,-b,-c,-d) when b > 0,
 *             (a,b,c,d) otherwise (b == -0.0 is not > 0), zeros without a winner; ground_height = fabsf(d), valid only with a winner. The border and
 *             mask_value == 0 tests (:627,635) come after the choice in the reference and only gate the append: a cluster can be chosen and not appended.
 *   marking   (:669-693) with g->mark_window_points: the winner's members (xx, yy) set bits in a w x h bitmap (cleared again by a walk over the same members: no
 *             fill of the plane in steady state); one lane per window point, in the loop order of nalo_trk_set_ref_from_window (host, then submission order):
 *             a point is tested when lastResiduals[0] (the window's point history) names frame W-1 with state IN and that residual is IN at the window's last
 *             linearizeAll(true) - in a history the fix passes maintain, the set nalo_trk_set_ref_from_window gathers; u = (int)(cpt.x + 0.5f), v =
 *             (int)(cpt.y + 0.5f) of its centerProjectedTo (DEFINED as elsewhere: saturating, NaN -> 0; outside the image matches nothing).
 *             n_ground_points = temp_gp_num; g->onground (optional, onground_cap >= P): one byte per point in nalo_ba_set_points' submission order. The
 *             reference's flag is sticky on the PointHessian: the caller ORs the byte into its objects, the library keeps no per-point state. Without a
 *             winner every byte is 0 and the count 0.
 *   Refusals  those of nalo_trk_fit_planes, plus NALO_ERR_ARG for g == NULL, pick == NULL or onground given with onground_cap < P; with mark_window_points
 *             NALO_ERR_STATE before anything is queued: no window or no points, no point history (nalo_ba_set_point_history), the window's last linearisation
 *             was not a fix = 1 one, the window is sharded. A refused call leaves the cloud, *pick and every context state as they were.
 *             NOT a refusal: with append = 1, NALO_ERR_STATE "the level-0 cloud would outgrow its w*h buffer" is nalo_trk_fit_planes' partial failure - the
 *             clusters before the overflowing one were appended and the records are written; the ground pass does not depend on the append, so *pick, the
 *             scores and onground are written as well and are valid.
 *
 * Host state, caller-owned, in/out; it mirrors where the reference keeps it:
 *   nalo_ground_tracker  per CoarseTracker OBJECT - the reference has two, swapped every keyframe (coarseTracker, coarseTracker_forNewKF), so a caller keeps two
 *                        and alternates them. Starts at {-1, -1, 0} (CoarseTracker.cpp:104-106).
 *   nalo_ground_globals  the globals of util/settings.cpp:36-40: {scale_fix 0, init_height -1, last_ScaleRate -1, last_gp {-1,-1,-1,-1}, old_rate empty}.
 *   nalo_ground_frame    one per window frame, in window order, starts at zero (last_ground is uninitialised in the reference: DEFINED as zeros).
 * nalo_ground_*_init set those values.
 * nalo_ground_update        :609-616 (ground_height taken over when there is a winner; without one the tracker's old ground_height and a zero gp_raw run the
 *   machine) and :696-816 as written, float arithmetic as written: the first scale_fix call only primes last_ScaleRate / last_gp / old_rate; the outlier branch
 *   (all five relative differences > 0.25) rewrites groundP from last_gp WITHOUT setting haveground; old_rate is a 7-deep window; with scale_fix and W > 6,
 *   last_ground of the newest frame = groundP of the first frame from W-2 down to 1 whose groundP[3] != 0. The assert of :794 is not reproduced.
 *   pick->ran == 0: nothing is touched (the reference returns at :566). NALO_ERR_ARG: a null pointer or W < 1.
 * nalo_ground_set_global_plane  FullSystem::setglobalplane (FullSystem.cpp:1911-1976): returns 1 and writes gplane, backup_gplane, *lgh when the plane is fixed,
 *   0 (nothing written) otherwise, NALO_ERR_ARG (negative) on a null pointer. W < max_frames (setting_maxFrames, 7): 0; DEFINED: W < 2: 0 as well (the
 *   reference would index fhs[W-2]). worldToCam_frame1 = PRE_worldToCam of window frame 1. DEFINED: the norm of the 4-vector difference pi - lastpi
 *   (lpNorm<2>, :1939: the Euclidean norm over its four components) and the M^T * pih product (all four rows, the last one (0,0,0,1)) are
 *   accumulated left to right in double; Eigen's order is not observable except at the 0.2 tie.
 * nalo_ground_local_scale   PlaneOptimize.cpp:203-211: *localscale = (double)lgh / (double)groundP[3], returns 1; 0 (nothing written) when !haveground. The
 *   caller's condition around it is makeKeyFrame's (:1420,1438): haveground && groundP[3] != 0 && scale_fix && gplanefixed.
 * nalo_ground_reset_global_plane  FullSystem::resetGlobalPlane (:1979-2001, uncalled in the reference): the newest frame before W-1 with haveground, its plane in
 *   the world frame; returns that frame's index or -1. worldToCam: W matrices of 12.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_ground_score {
    float mid_z;           /* 0 when the cluster took no part */
    float score;
    int   scored;          /* 1: fitted && n_cloud == n */
} nalo_ground_score;
typedef struct nalo_ground_pick {
    int   ran;             /* 0: fewer than 4 clusters, nothing else is written */
    int   cluster;         /* record index of the ground, -1: no cluster took part */
    float gp_raw[4];
    float ground_height;   /* valid only with a winner */
    int   n_ground_points; /* temp_gp_num (0 without mark_window_points) */
} nalo_ground_pick;
typedef struct nalo_ground_args {
    int      mark_window_points;
    uint8_t* onground;     /* optional: one byte per window point, submission order */
    int      onground_cap; /* >= P when onground is given */
    nalo_ground_score* scores;   /* optional: cap entries, the first *n_clusters are written */
} nalo_ground_args;
int nalo_trk_fit_ground(nalo_ctx* ctx, const nalo_plane_fit_args* fit, const nalo_ground_args* g, int cap, nalo_plane_cluster* out, int* n_clusters,
                        nalo_ground_pick* pick);

typedef struct nalo_ground_tracker { float ground_height, last_height; int suc_num; } nalo_ground_tracker;
typedef struct nalo_ground_globals { int scale_fix; float init_height, last_ScaleRate, last_gp[4]; int n_old; float old_rate[7]; } nalo_ground_globals;
typedef struct nalo_ground_frame { float groundP[4], last_ground[4]; int haveground, scaleFixed; } nalo_ground_frame;
void nalo_ground_tracker_init(nalo_ground_tracker* t);
void nalo_ground_globals_init(nalo_ground_globals* g);
void nalo_ground_frame_init(nalo_ground_frame* f);
int nalo_ground_update(const nalo_ground_pick* pick, nalo_ground_tracker* tracker, nalo_ground_globals* globals, nalo_ground_frame* frames, int W);
int nalo_ground_set_global_plane(const nalo_ground_frame* frames, int W, int max_frames, const double worldToCam_frame1[12], double gplane[4],
                                 double backup_gplane[4], float* lgh);
int nalo_ground_local_scale(const nalo_ground_frame* frame_newest, float lgh, double* localscale);
int nalo_ground_reset_global_plane(const nalo_ground_frame* frames, int W, const double* worldToCam, double gplane[4]);

/* ------------------------------------------------------------------------------------------------
 * the immature-point depth filter and point activation that run either side of the BA.
 * Point state is caller-owned (the reference keeps it in ImmaturePoint objects): arrays of n points in, updated arrays out.
 * color/weights are [n][8] (pattern order), gradH is [n][3] = {xx, xy, yy}.
 *
 * nalo_imm_create    ImmaturePoint::ImmaturePoint (FullSystem/ImmaturePoint.cpp:32-60), call site FullSystem::makeNewTraces
 *                    (FullSystem.cpp:1596-1625): color, weights, gradH, energyTH (NaN = point rejected) from the host frame's slot.
 * nalo_imm_trace     ImmaturePoint::traceOn (ImmaturePoint.cpp:76-435) for every immature point of every host against the frame in
 *                    slot_new, replaces the loops of FullSystem::traceNewCoarse (FullSystem.cpp:702-744), which computes per host
 *                    KRKi = K R K^-1 (row-major 3x3), Kt = K t and the affine pair (AffLight::fromToVecExposure): pass them as [nh][9],
 *                    [nh][3], [nh][2] with host_idx[n] selecting the host of each point.
 *                    In/out: idepth_min, idepth_max, status (ImmaturePointStatus: 0 GOOD, 1 OOB, 2 OUTLIER, 3 SKIPPED, 4 BADCONDITION,
 *                    5 UNINITIALIZED), quality. Out: lastTraceUV [n][2], lastTracePixelInterval [n].
 * nalo_imm_optimize  FullSystem::optimizeImmaturePoint (FullSystem/FullSystemOptPoint.cpp:51-206) incl. ImmaturePoint::linearizeResidual
 *                    (ImmaturePoint.cpp:497-564), call site FullSystem::activatePointsMT_Reductor (FullSystem.cpp:748-762). Uses the
 *                    frames, current states (PRE_RTll / PRE_tTll / PRE_aff_mode) and calibration of the window set by nalo_ba_set_window;
 *                    host[n] = window index of each point's host frame.
 *                    result[n]: 0 = not well constrained (the point stays immature), -1 = drop the point, 1 = activated with
 *                    idepth_out[n]; res_in[n][W] = 1 where a PointFrameResidual is created (state IN).
 * ------------------------------------------------------------------------------------------------ */
/* CoarseDistanceMap::makeDistanceMap + growDistBFS (FullSystem/CoarseTracker.cpp:1410-1561), call site FullSystem::activatePointsMT
 * (FullSystem.cpp:797-798). Uses the ACTIVE POINTS of the window set by nalo_ba_set_points (already on the device); frame = window index of the newest frame
 * (its own points are skipped); KRKi[W][9] = K[1] R Ki[0] and Kt[W][3] = K[1] t per host (floats, as :1424-1425). out = fwdWarpedIDDistFinal [w1*h1]
 * (level-1 size), 1000 = farther than 39. addIntoDistFinal (:1556-1561, one seed per newly activated point, sequential) stays on the caller's copy. */
/* ---- PixelSelector (FullSystem/PixelSelector2.cpp), SURVEY 8(f) rank 3. The selector's state (randomPattern, the block thresholds of
 * gradHistFrame, the last status map) lives in the context, as it lives in the PixelSelector object.
 *  nalo_pixsel_set_random       the constructor's randomPattern[w*h] (:40-45: srand(3141592); rand() & 0xFF) and, for FusedWithMask, the first w*h
 *                               rand() values after srand(3141592) (:496-501; NULL if makeMaps_lidar is not used). Both are libc streams, so the
 *                               caller draws them and the selection stays identical to the reference built on the same libc.
 *  nalo_pixsel_make_hists       makeHists (:78-142): block thresholds of the frame in `slot`; ths / thsSmoothed [(w/32)*(h/32)] may be NULL.
 *  nalo_pixsel_select           select (:564-711) with potential `pot` on the frame make_hists ran on: n = {n2, n3, n4} (its return value),
 *                               map_out[w*h] (may be NULL) = 0 / 1 / 2 / 4 per pixel like PixelSelectorStatus.
 *  nalo_pixsel_make_maps        makeMaps (:144-291): makeHists if the frame changed, select, up to recursionsLeft re-selections with the adapted
 *                               potential, the random sub-selection; *currentPotential is PixelSelector::currentPotential (in/out),
 *                               *numHaveSub the return value. Call sites: CoarseInitializer.cpp:811, FullSystem.cpp:1663.
 *  nalo_pixsel_make_maps_lidar  makeMaps_lidar (:293-428) = makeHists + select + FusedWithMask (:431-560) with the mask the frame was uploaded
 *                               with; *numHave the return value. Call site FullSystem.cpp:1668. (The reference reads mhist[256], one past its
 *                               array, in the last quantile iteration: taken as 0 here.)
 *  nalo_pixsel_get_selected     the non-zero pixels of the last map in raster order (idx = x + y*w, status), i.e. what makeNewTraces' loop over
 *                               the map visits (FullSystem.cpp:1672-1690): *n = their number, the first min(cap, *n) are written. The list
 *                               lives in one pinned block from the select / make_maps / make_maps_lidar that made the map until the next of
 *                               them; nalo_pixsel_make_hists with a non-NULL ths or thsSmoothed reads the thresholds back through that block,
 *                               and nalo_pixsel_get_selected then answers NALO_ERR_STATE until a new map is made. make_hists(NULL, NULL) and
 *                               a frame upload (to this or another slot) leave the list as it is. */
int nalo_pixsel_set_random(nalo_ctx* ctx, const uint8_t* randomPattern, const int* mask_draws);
int nalo_pixsel_make_hists(nalo_ctx* ctx, int slot, float* ths, float* thsSmoothed);
int nalo_pixsel_select(nalo_ctx* ctx, int slot, int pot, float thFactor, float* map_out, int n[3]);
int nalo_pixsel_make_maps(nalo_ctx* ctx, int slot, float density, int recursionsLeft, float thFactor, int* currentPotential, float* map_out, int* numHaveSub);
int nalo_pixsel_make_maps_lidar(nalo_ctx* ctx, int slot, float thFactor, int currentPotential, float* map_out, int* numHave);
int nalo_pixsel_get_selected(nalo_ctx* ctx, int cap, int* idx, uint8_t* status, int* n);
int nalo_dist_make_map(nalo_ctx* ctx, int frame, const float* KRKi, const float* Kt, float* out);
int nalo_imm_create(nalo_ctx* ctx, int slot_host, int n, const int* u, const int* v, float* color, float* weights, float* gradH, float* energyTH);
int nalo_imm_trace(nalo_ctx* ctx, int slot_new, int n, const float* u, const float* v, const float* color, const float* weights, const float* gradH,
                   const float* energyTH, const int* host_idx, int nh, const float* KRKi, const float* Kt, const float* aff,
                   float* idepth_min, float* idepth_max, int* status, float* quality, float* lastTraceUV, float* lastTracePixelInterval);
/* Device-resident form of the tracing state (what a running system uses: ImmaturePoints live across frames, traceNewCoarse touches all of them on
 * every frame, the host only looks at them when it activates points). nalo_imm_resident_set uploads the whole set (after makeNewTraces / activation,
 * once per keyframe; lastTraceUV = (-1,-1), lastTracePixelInterval = 0 as the constructor leaves them), nalo_imm_resident_trace = traceNewCoarse for one
 * new frame: only the nh x {KRKi, Kt, aff} cross PCIe, the call returns without waiting; nalo_imm_resident_get brings the state back (sync inside;
 * lastTraceUV / lastTracePixelInterval may be NULL). Arrays as in nalo_imm_trace. */
int nalo_imm_resident_set(nalo_ctx* ctx, int n, const float* u, const float* v, const float* color, const float* weights, const float* gradH, const float* energyTH,
                          const int* host_idx, const float* idepth_min, const float* idepth_max, const int* status, const float* quality);
int nalo_imm_resident_trace(nalo_ctx* ctx, int slot_new, int nh, const float* KRKi, const float* Kt, const float* aff);
int nalo_imm_resident_get(nalo_ctx* ctx, float* idepth_min, float* idepth_max, int* status, float* quality, float* lastTraceUV, float* lastTracePixelInterval);
int nalo_imm_optimize(nalo_ctx* ctx, int n, const int* host, const float* u, const float* v, const float* color, const float* weights,
                      const float* energyTH, const float* idepth_min, const float* idepth_max, int minObs,
                      int* result, float* idepth_out, uint8_t* res_in);
/* The same for points of the device-resident set (nalo_imm_resident_set, kept up to date by nalo_imm_resident_trace): sel[n] = their indices in that set (NULL: all of
 * them, n = the set's size). Pattern colours, weights, energyTH, host frame (host_idx must index the window's frames) and the inverse-depth interval [idepth_min,
 * idepth_max] - as the device's last trace left it, FullSystem.cpp:700-760 activates right after traceNewCoarse - are read on the device; 4 bytes per point cross PCIe
 * on the way down instead of 88. Outputs as nalo_imm_optimize. */
int nalo_imm_resident_optimize(nalo_ctx* ctx, int n, const int* sel, int minObs, int* result, float* idepth_out, uint8_t* res_in);
/* FullSystem::activatePointsMT's steps 1-3 (FullSystem.cpp:794-889) for the resident set, on the device: makeDistanceMap of the window's active points for the
 * newest keyframe `frame` (as nalo_dist_make_map; KRKi[W][9], Kt[W][3] host -> frame at level 1), the loop :805-876 that deletes / keeps / selects every immature
 * point against that map and adds each selected point into it (addIntoDistFinal) before the next is looked at, and optimizeImmaturePoint of the selected points
 * (as nalo_imm_resident_optimize). The loop's order is the reference's: by host_idx, and inside a host by index in the resident set. The result is the
 * sequential loop's for every input; the host waits once, at the end (more often only when the selection needs more than 12 dependent rounds).
 *   nalo_imm_resident_set_type   my_type[n] (ImmaturePoint::my_type, 1 / 2 / 4) of the resident points, once after nalo_imm_resident_set (which invalidates it).
 *   nalo_imm_resident_activate   host_flagged[W]: FrameHessian::flaggedForMarginalization; currentMinActDist as the reference keeps it, in [0, 4].
 *       fate[n] per resident point:  1 selected;  0 kept (cannot activate yet);  2 kept (too close to an active or an earlier selected point);
 *                                   -1 deleted (never traced, or OUTLIER: :820);  -2 deleted (not ready and host flagged or OOB: :843);
 *                                   -3 deleted (projects outside the frame: :870);  3 not visited (hosted by `frame`: :807).
 *       *n_sel, sel[n]: the selected points' indices in the resident set in the order of the reference's toOptimize (the first *n_sel are written);
 *       result / idepth_out / res_in[n][W]: rows k < *n_sel as nalo_imm_resident_optimize(sel) returns them; all three NULL = selection only.
 *       NALO_ERR_STATE: no window / points, no resident set or no types, a sharded window (a rank holds only part of the map's seeds), a resident host_idx
 *       outside the window. NALO_ERR_ARG: NULL pointers, frame outside the window, currentMinActDist negative or not finite, and currentMinActDist * my_type
 *       above 16 for any resident point (REFUSED, not computed: the parallel selection looks 16 level-1 pixels around a point, the reference's ranges give <= 16).
 *   nalo_imm_activate_last       of the last call: stats = {points that pass the test on the initial map, selected, rejected because of an earlier selected
 *                                point, dependent rounds run}. */
int nalo_imm_resident_set_type(nalo_ctx* ctx, const float* my_type);
int nalo_imm_resident_activate(nalo_ctx* ctx, int frame, const float* KRKi, const float* Kt, const int* host_flagged, float currentMinActDist, int minObs,
                               int* fate, int* n_sel, int* sel, int* result, float* idepth_out, uint8_t* res_in);
int nalo_imm_activate_last(nalo_ctx* ctx, int stats[4]);
/* The resident immature set across a keyframe, on the device: what the caller otherwise rebuilds once per keyframe through nalo_imm_resident_get, its own
 * bookkeeping, nalo_imm_create and nalo_imm_resident_set / _set_type. All of a resident point's state is carried, lastTraceUV and lastTracePixelInterval
 * included (nalo_imm_resident_set resets both; the reference keeps them on the ImmaturePoint and canActivate reads the interval, FullSystem.cpp:833).
 * nalo_imm_resident_carry applies up to three parts, in the order A, C, B; each is optional and any combination may come in one call:
 *   (A) the end of activatePointsMT for the immature set. fate[n] as nalo_imm_resident_activate returned it, sel[n_sel] its toOptimize list, result[n_sel]
 *       optimizeImmaturePoint's verdicts. A point is removed when its fate is -1, -2 or -3 (FullSystem.cpp:820-826, :840-851, :870-874), when it is selected
 *       and result == 1 (it became a PointHessian, :898-907) or result == -1 (:908-912), and when it is selected, result == 0 and its resident status is IPS_OOB
 *       (:908, read on the device). Every other point stays: fates 0, 2 and 3, and selected points with result == 0 that are not OOB (:913). Then every host's
 *       vector - the host's points in ascending resident index - is compacted by the loop :920-931 exactly as written there: a hole takes the vector's back and
 *       is looked at again, so the order after the call is the reference's swap-with-back order, which decides what the next activation selects.
 *       NALO_ERR_ARG: sel does not list exactly the points with fate 1; result missing with n_sel > 0; a fate outside [-3, 3], a result outside {1, 0, -1}.
 *       fate == NULL skips the part.
 *   (C) frames that left the window: host_map[h_old] = h_new, or -1 for a frame that left; its points go with it (FrameHessian's destructor,
 *       HessianBlocks.cpp:117), the others are renumbered, order inside a host is untouched. The kept entries must be 0 .. W_new-1 in increasing order and every
 *       resident host_idx must be < n_hosts_old (NALO_ERR_ARG otherwise). host_map == NULL: identity.
 *   (B) makeNewTraces (FullSystem.cpp:1677-1687) for the frame in append_slot, hosted by append_host (NEW numbering; append_slot < 0: no append). The list is
 *       append_idx / append_status[append_n] (idx = x + y*w, status = the selection map's value), or with append_idx == NULL the raster-ordered list of the
 *       selector's last map, which is already on the device. The walk is the loop's: entries with status 0 and entries outside
 *       patternPadding+1 <= x < w-patternPadding-2 (y likewise, :1677-1678) are skipped, not refused; every other entry gets the ImmaturePoint constructor
 *       (ImmaturePoint.cpp:32-60, the arithmetic of nalo_imm_create); a point whose energyTH is not finite is dropped (:1684); the others are appended behind the
 *       host's carried points, in list order, with my_type = status, idepth_min = 0, idepth_max = NaN, status IPS_UNINITIALIZED, quality 10000,
 *       lastTraceUV = (-1,-1), lastTracePixelInterval = 0. NALO_ERR_STATE: append_idx == NULL and no map was made on append_slot (or the slot was uploaded to
 *       since, or
 *       nalo_pixsel_make_hists read its thresholds back since); a slot without a pyramid; a resident set without types (nalo_imm_resident_set_type). NALO_ERR_ARG:
 *       append_host outside [0, NALO_MAX_WINDOW), an entry outside the image, a status above 15, an explicit list that is not in raster order with every pixel once.
 * The new set is ordered by new host index, ascending; inside a host it is the reference's vector. It may be empty. The set's size, its largest host index and
 * the host copies nalo_ba_carry_window(insert_activated) orders inserted points by are updated; a set with types keeps them (the bound that
 * nalo_imm_resident_activate checks currentMinActDist * my_type against keeps the types of deleted points). A pending activation result is DROPPED: call
 * nalo_ba_carry_window(..., insert_activated) before this call. A refusal leaves the set as it was. Down go one byte per old point, the host map and an explicit
 * append list; up come the 4-byte map and the counts; the call waits for the stream once and, once its buffers have grown to the set, allocates nothing.
 *   nalo_imm_resident_carry_map   src[n_new]: the old index of every point of the new set, or -(k + 2) for the k-th entry of the append list (of the caller's
 *                                 list, or of nalo_pixsel_get_selected's). NALO_ERR_STATE when the resident set does not come from a carry.
 *   nalo_imm_resident_carry_last  {n_new, deleted by (A), dropped with their host by (C), appended, points per new host [NALO_MAX_WINDOW]} of the last call.
 *   nalo_imm_resident_get_points  the resident points' constant part and my_type (any pointer NULL; arrays as nalo_imm_resident_set takes them): with
 *                                 nalo_imm_resident_get the whole state, for tests and a debugging caller. */
typedef struct {
    const int* fate;                                  /* (A) [n]; NULL: skip */
    int n_sel; const int* sel; const int* result;
    const int* host_map; int n_hosts_old;             /* (C) NULL: identity */
    int append_slot, append_host;                     /* (B) append_slot < 0: none; append_host in the NEW numbering */
    int append_n; const int* append_idx; const unsigned char* append_status;   /* append_idx NULL: the selector's last map */
} nalo_imm_carry_args;
int nalo_imm_resident_carry(nalo_ctx* ctx, const nalo_imm_carry_args* args);
int nalo_imm_resident_carry_map(nalo_ctx* ctx, int* src /* n_new */);
int nalo_imm_resident_carry_last(nalo_ctx* ctx, int stats[4 + NALO_MAX_WINDOW]);
int nalo_imm_resident_get_points(nalo_ctx* ctx, int* n, float* u, float* v, float* color, float* weights, float* gradH, float* energyTH, int* host_idx, float* my_type);

/* ------------------------------------------------------------------------------------------------
 * the two-frame initialiser's Gauss-Newton pass.
 * nalo_init_calc_res_and_gs  CoarseInitializer::calcResAndGS (FullSystem/CoarseInitializer.cpp:338-610), call sites :129,163 (trackFrame), for one
 *     pyramid level lvl between the pyramids in slot_first (firstFrame) and slot_new. Pnt members are caller-owned arrays of n points:
 *     in  u, v, idepth_new, iR, isGood[n] (0/1), energy[n][2], outlierTH;
 *     out isGood_new, energy_new[n][2], maxstep; in/out lastHessian_new, JbBuffer_new[n][10] (entries the reference leaves untouched stay).
 *     refToNew = 3x4 row-major [R|t], aff = {a, b} of refToNew_aff; alphaW, alphaK, couplingWeight as in the constructor (:92-95: 150^2, 2.5^2, 1).
 *     H_out/H_out_sc are 8x8 row-major, b_out/b_out_sc 8, E3 = {E.A, alphaEnergy, E.num} exactly as returned (:609), including the reference's
 *     behaviour that the regulariser loop feeds E instead of EAlpha (:560-572).
 * nalo_init_do_step          CoarseInitializer::doStep (:910-938): idepth_new[i] for the good points from JbBuffer (the applied buffer), inc[8], lambda.
 * applyStep (:939-956) is a member copy on the caller's arrays (or use nalo_init_track_frame below, which runs the whole loop).
 * ------------------------------------------------------------------------------------------------ */
int nalo_init_calc_res_and_gs(nalo_ctx* ctx, int slot_first, int slot_new, int lvl, int n, const float* u, const float* v, const float* idepth_new, const float* iR,
                              const uint8_t* isGood, const float* energy, const float* outlierTH, const double refToNew[12], const double aff[2],
                              float alphaW, float alphaK, float couplingWeight,
                              uint8_t* isGood_new, float* energy_new, float* maxstep, float* lastHessian_new, float* JbBuffer_new,
                              double* H_out, double* b_out, double* H_out_sc, double* b_out_sc, double E3[3]);
int nalo_init_do_step(nalo_ctx* ctx, int n, const uint8_t* isGood, const float* JbBuffer, const float* maxstep, const float* idepth, float lambda,
                      const float inc[8], float* idepth_new);
/* The whole initialiser behind the boundary (the CoarseInitializer object lives in the context; Pnt arrays on the host side of the library, the two
 * per-point image passes and both point selections on the device):
 * nalo_init_set_first    CoarseInitializer::setFirst (FullSystem/CoarseInitializer.cpp:785-880), call site FullSystem::addActiveFrame (FullSystem.cpp:1101):
 *     makeK from the context's calibration, level 0 selected by a fresh PixelSelector (makeMaps(., 0.03 w h, 1, false, 2), currentPotential 3: needs
 *     nalo_pixsel_set_random), levels >= 1 by makePixelStatus / gridMaxSelection (FullSystem/PixelSelector.h:38-253) with densities {0.05, 0.15, 0.5, 1} w h,
 *     Pnt construction, makeNN (:992-1069; the reference's nanoflann k-d tree, tie order included). *sparsityFactor is the reference's GLOBAL of that name
 *     (util/settings.cpp:223, initially 5; makePixelStatus keeps adapting it from call to call): in/out. numPoints[lvl] (optional) = points per level.
 * nalo_init_track_frame  CoarseInitializer::trackFrame (:81-285), call site FullSystem.cpp:1106: the coarse-to-fine LM over pose, (fixed) affine and the
 *     inverse depths with propagateDown / resetPoints / calcResAndGS / doStep / calcEC / applyStep / optReg / propagateUp; exposures are
 *     firstFrame->ab_exposure and newFrame->ab_exposure. *ok = its return value (snapped && frameID > snappedAt + 5).
 * nalo_init_get_state    thisToNext (3x4), thisToNext_aff {a, b}, snapped, frameID, snappedAt (+ the number of calcResAndGS evaluations so far); any may be NULL.
 * nalo_init_get_points   the Pnt members FullSystem::initializeFromInitializer reads (FullSystem.cpp:1601-1660: u, v, iR, my_type of level 0) and the rest
 *     of the state, for one level: *n = numPoints[lvl], the first min(cap, *n) entries are written; energy2 is [n][2], neighbours / neighboursDist [n][10];
 *     any output may be NULL. */
int nalo_init_set_first(nalo_ctx* ctx, int slot_first, int* sparsityFactor, int numPoints[NALO_MAX_LEVELS]);
int nalo_init_track_frame(nalo_ctx* ctx, int slot_new, float exposure_first, float exposure_new, int* ok);
int nalo_init_get_state(nalo_ctx* ctx, double thisToNext[12], double aff[2], int* snapped, int* frameID, int* snappedAt, int* n_evals);
/* nalo_init_set_state / nalo_init_set_points: write back what trackFrame carries from frame to frame (thisToNext, thisToNext_aff, snapped, frameID, snappedAt; per
 *     level the Pnt members idepth, idepth_new, iR, isGood, lastHessian, energy, maxstep and the *_new / iRSumNum members stale entries of which survive a frame; NULL = leave as is): resume of a checkpointed initialisation, and what
 *     the teacher-forced parity test uses to start every frame from the oracle's state. n must equal the level's point count. */
int nalo_init_set_state(nalo_ctx* ctx, const double thisToNext[12], const double aff[2], int snapped, int frameID, int snappedAt);
int nalo_init_set_points(nalo_ctx* ctx, int lvl, int n, const float* idepth, const float* idepth_new, const float* iR, const uint8_t* isGood, const float* lastHessian,
                         const float* energy2, const float* maxstep, const float* lastHessian_new, const float* energy_new2, const uint8_t* isGood_new, const float* iRSumNum);
/* nalo_init_sweep: one of trackFrame's per-level sweeps on its own, on the initialiser's current state (replaces CoarseInitializer::optReg :656-691, ::propagateUp
 *     :695-734 (lvl = srcLvl, 0 .. levels-2), ::propagateDown :736-766 (lvl = srcLvl, 1 .. levels-1), ::resetPoints :882-909; optReg reads `snapped` as set by
 *     nalo_init_set_state / trackFrame). trackFrame calls the same code; the entry point exists so that each sweep can be checked against the reference's alone. */
/* nalo_init_get_carried: the read side of nalo_init_set_points for the members nalo_init_get_points does not return (iRSumNum is recomputed by propagateUp before
 *     anything reads it and is not kept); the first min(cap, n) entries, any output may be NULL. */
int nalo_init_get_carried(nalo_ctx* ctx, int lvl, int cap, float* idepth_new, float* maxstep, float* lastHessian_new, float* energy_new2, uint8_t* isGood_new);
#define NALO_INIT_SWEEP_OPT_REG 0
#define NALO_INIT_SWEEP_PROPAGATE_UP 1
#define NALO_INIT_SWEEP_PROPAGATE_DOWN 2
#define NALO_INIT_SWEEP_RESET_POINTS 3
int nalo_init_sweep(nalo_ctx* ctx, int which, int lvl);
int nalo_init_get_points(nalo_ctx* ctx, int lvl, int cap, int* n, float* u, float* v, float* idepth, float* iR, uint8_t* isGood, float* lastHessian, float* energy2,
                         float* my_type, float* outlierTH, int* parent, float* parentDist, int* neighbours, float* neighboursDist);

/* ------------------------------------------------------------------------------------------------
 * The initialiser's depth panel: CoarseInitializer::debugPlot(lvl, wraps) (FullSystem/CoarseInitializer.cpp:287-335, called at the end of every trackFrame, :280;
 * on by default with the Pangolin viewer and the only thing the depth panel shows until the system has initialised) on the device: the MinimalImageB3 handed to
 * Output3DWrapper::pushDepthImage. It reads the initialiser's CURRENT state where it lies - u, v, iR, isGood of the level, after the same "upload the host
 * mirror if it is the newer side" step nalo_init_sweep takes behind nalo_init_set_points - and the irradiance of the first frame's slot at that level, channel 0
 * of its texels (firstFrame->dIp[lvl][i][0], what nalo_frame_download returns; the slot's planar I[] is filled at level 0 only by the one-pass pyramid); nothing
 * of the Pnt arrays visits the host (the route it replaces, nalo_init_get_points, refreshes the host mirror of every member of every level). The call changes
 * nothing of the initialiser, and a context that never calls it enqueues exactly what it did before. Kernels on the context's stream, ONE wait; results and image
 * come up through a pinned block and reach the caller only on success.
 *   Base      (:300-301) Vec3b(I, I, I) from the float, no 0.9f factor. The float -> unsigned char conversion is DEFINED as (unsigned char)__float2int_rz(I):
 *             truncation toward zero, saturating to int, NaN -> 0, then it wraps - nalo_trk_depth_image's rules, and what x86 produces for values int holds.
 *   Scale     (:306-316) n_good counts the points with isGood != 0 (`nid`, a float counter in the reference, exact below 2^24). sum_iR (`sid`) is the chain of
 *             dependent float adds of iR over the good points IN INDEX ORDER, starting from 0.f: no tree, no atomic, no fp64. fac = (float)n_good / sum_iR in
 *             float: NaN for a level without a good point, +-inf for sum_iR = 0 with good points. A NaN sum_iR or fac is a NaN; its sign and payload are not defined.
 *   Squares   (:320-329) per point setPixel9((int)(u + 0.5f), (int)(v + 0.5f), c): the 3x3 block around the centre; c is black for a point that is not good, else
 *             makeRainbow3B(iR * fac) with freeDebugParam3 = rainbow_scale, as nalo_map_window_plot's Rainbow (its DEFINED difference 3 included).
 *   Overlap   points are painted in ascending index, so the LAST index wins a pixel - exactly so here, on every run: an integer maximum of index + 1 per covered
 *             pixel, then a pass that paints the winner or the base. No float atomic.
 * DEFINED differences from the reference: MinimalImage::at() has no bounds check, here pixels of a block outside the image are skipped; (int)(u + 0.5f) of a value
 *   int cannot hold saturates, NaN gives 0.
 * A level with no points (the base image) or with no good point (black squares only) is legal.
 * Refusals, each leaving bgr, the other outputs and the context as they were. NALO_ERR_ARG: NULL ctx / args / bgr; lvl outside the initialiser's levels;
 *   rainbow_scale not finite. NALO_ERR_STATE: no nalo_init_set_first yet; the first frame's slot has no pyramid. NALO_ERR_HIP: a cross-rank exchange of this
 *   context failed earlier.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_init_plot_args {
    int      lvl;             /* the reference passes 0; every level the initialiser holds is legal */
    float    rainbow_scale;   /* freeDebugParam3 (settings.cpp:191), 1 in the reference */
    uint8_t* bgr;             /* out: [h][w][3] of the level (at most 3 * w * h bytes of level 0), bytes of a pixel in Vec3b's order */
    int      w, h;            /* out: the level's size */
    int      n_points;        /* out: numPoints[lvl] */
    int      n_good;          /* out: nid */
    float    sum_iR, fac;     /* out: sid, fac */
} nalo_init_plot_args;
int nalo_init_depth_image(nalo_ctx* ctx, nalo_init_plot_args* args);

/* ------------------------------------------------------------------------------------------------
 * The map side of the device chain: the points nalo_ba_marginalize_flagged removes stay resident in a device archive, and what the reference publishes
 * per keyframe is produced from resident data. In the reference the removed points ARE the map: flagPointsForRemoval pushes them onto
 * host->pointHessiansMarginalized / host->pointHessiansOut (FullSystem/FullSystem.cpp:968, 996, 1001, 1008) and publishKeyframes, SampleOutputWrapper and
 * KeyFrameDisplay read those two vectors. Opt-in: a context that never calls nalo_map_enable enqueues exactly what it did before.
 *
 * nalo_map_enable(ctx, on, chunk_points)   while on, nalo_ba_marginalize_flagged appends every point it removes (marginalised and dropped) to the archive
 *   before the slots are cleared. Call it BEFORE the nalo_ba_flag_points whose decisions are to be archived (the record keeps that call's decision and
 *   idepth_hessian; nalo_ba_marginalize_flagged returns NALO_ERR_STATE, touching nothing, for decisions made while the map was off). The archive grows
 *   in chunks of chunk_points records (0 = 65536; the value in force when the first chunk is allocated holds for the context): a new chunk is a new allocation,
 *   archived records never move; in steady state the call allocates nothing. Room is reserved for every valid point of the window before anything is
 *   touched (the count of removed points is only known on the device), so a refusal for lack of memory leaves archive and window as they were. NALO_ERR_STATE on a sharded window and on a context whose exchange failed.
 *   Record    nalo_map_record, 64 bytes: the values the reference's PointHessian holds when it is published. maxRelBaseline is that of the last
 *             linearizeAll(true). idepth_hessian of a dropped point (status 3) is what nalo_ba_flag_points reports; that of a marginalised point (status 2)
 *             is rewritten by marginalizePointsF's addPoint (AccumulatedSCHessian.cpp:36-50): H of the re-accumulated Hdd and the scaled prior, and
 *             idepth_hessian = maxRelBaseline = 0 for a point whose re-linearisation left no active residual.
 *   Order     per call: host frame in window order, then submission order inside the host (the order of nalo_trk_set_ref_from_window and
 *             nalo_dense_fit_planes) - an ordered compaction, never an atomic. The reference's pointHessiansOut holds removeOutliers' points before
 *             flagPointsForRemoval's inside one keyframe and permutes by swap-with-back; the sets and every value are equal, the order inside a keyframe's
 *             run is the library's.
 *   frame_id  the caller's, from nalo_frame_state: the archive is keyed by it, so the frames of a session need distinct ids.
 *   Not archived: points removed by nalo_ba_marginalize_points (host flags). nalo_ba_snapshot / nalo_ba_restore do not include the archive (nor the graph of
 *   nalo_map_graph_enable).
 * nalo_map_reset      empties the archive (and the dense archive of nalo_map_dense_enable) and keeps its chunks; empties the graph of nalo_map_graph_enable.
 *                     It does not touch the TSDF volume (nalo_tsdf_reset does that).
 * nalo_map_counts     counts = {pointHessiansMarginalized.size(), pointHessiansOut.size()} of the frame: the addends of flagFramesForMarginalization's
 *                     `out` (FullSystemMarginalize.cpp:77). NALO_ERR_ARG for a frame_id the archive has never seen.
 * nalo_map_get_frame  the frame's records: its status-2 records in archive order, then its status-3 records. *n = their number; cap < *n: NALO_ERR_ARG
 *                     (with *n set), as is an unknown frame_id.
 *
 * nalo_map_world_points   SampleOutputWrapper::publishKeyframes(final = true) for the frame's marginalised points (SampleOutputWrapper.h:110-118), one lane
 *   per status-2 record, in archive order: xyz [n][3] doubles = camToWorld * back-projection with the float inverse calibration {1/fx, 1/fy, -cx/fx, -cy/fy}
 *   of the window's current CalibHessian (value_scaledf). The arithmetic is nalo_io_write_pcd_points' (one shared function): equal bit for bit.
 *   cap < *n: NALO_ERR_ARG with *n set. One wait.
 * nalo_map_world_points_host  that one function on host arrays (no device, no context): the numbers nalo_io_write_pcd_points formats for the same points.
 *   calib_inv = {fxi, fyi, cxi, cyi}.
 *
 * nalo_map_frame_cloud    KeyFrameDisplay::setFromKF + refreshPC (IOWrapper/Pangolin/KeyFrameDisplay.cpp:92-177, 297-410) for one frame, from resident data.
 *   Records   [immature | active | marginalised | out], status 0 / 1 / 2 / 3. Status 0: the resident immature points (nalo_imm_resident_*) whose host_idx is
 *             the frame's window index, in storage order, idepth = (idepth_max + idepth_min) * 0.5f, idepth_hessian = 1000, relObsBaseline = 0; left out
 *             when with_immature == 0. Status 1: the frame's valid window points in submission order, idepth_hessian by nalo_ba_flag_points' formula.
 *             Statuses 2, 3: the archive. A frame that has left the window has only the last two classes. NALO_ERR_ARG for a frame_id that is neither in
 *             the window nor in the archive; NALO_ERR_STATE for a window frame whose points are unset (between nalo_ba_marginalize_frame and the carry).
 *   Filter    as written at :313-331, mixed precision included: display_mode (0 all, colour-coded; 1 statuses 1, 2; 2 status 1; > 2 nothing); idepth < 0
 *             skips; depth = 1.0f / idepth; depth4 = (depth * depth)^2; var = (float)(1.0 / ((double)idepth_hessian + 0.01)); var * depth4 > scaledTH skips;
 *             var > absTH skips; relObsBaseline < minRelBS skips. NaNs take the branch the comparisons give them.
 *   Vertices  each survivor gives 8, pnt = 0..7, (dx, dy) = patternP[pnt]: x = ((u + dx) * fxi + cxi) * depth, y = ((v + dy) * fyi + cyi) * depth,
 *             z = depth * (1 + 2 * fxi * (r / (float)RAND_MAX - 0.5f)), RAND_MAX = 2^31 - 1, r = draws[j] for output vertex j (the caller's libc rand()
 *             stream, as with nalo_pixsel_set_random). draws == NULL is the library's no-jitter form: the bracket is exactly 1, z = depth. With draws,
 *             n_draws >= 8 x records of the frame is required (NALO_ERR_ARG, *n_needed set), and cap >= 8 x records always (alike).
 *   Colour    display_mode 0: the constant triples of :349-372; else three times color[pnt], float -> byte by truncation toward zero, saturated to 0..255,
 *             NaN -> 0 (the reference's conversion is undefined outside that range).
 *   sparsity > 1 is refused (NALO_ERR_ARG): its rand() % factor makes every later draw index depend on earlier draw values. The pcl::PointXYZ branch of the
 *             second refreshPC overload (:534-550) reads the vertex after the one it wrote and is not reproduced.
 *   Output order is record order, then pnt. records[4] / survivors[4]: per status. One wait per call.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_map_record {
    float u, v, idepth, idepth_hessian;     /* idepth = PointHessian::idepth_scaled (SCALE_IDEPTH is 1) */
    float maxRelBaseline;
    int status;                             /* 2 marginalised, 3 out */
    int decision;                           /* nalo_ba_flag_points' class: 1, 2 or 3 */
    int frame_id;
    float color[8];
} nalo_map_record;                          /* 64 bytes, 16-byte aligned on the device */
typedef struct nalo_map_cloud_args {
    int frame_id, display_mode, with_immature, sparsity;
    float scaledTH, absTH, minRelBS;
    int n_draws; const int* draws;          /* NULL: no jitter */
    int cap; float* xyz; uint8_t* rgb;      /* cap vertices: [cap][3] each */
    int n, n_needed;                        /* out: vertices written; 8 x records (what cap and n_draws must reach) */
    int records[4], survivors[4];           /* out */
} nalo_map_cloud_args;
int nalo_map_enable(nalo_ctx* ctx, int on, int chunk_points);
int nalo_map_reset(nalo_ctx* ctx);
int nalo_map_counts(nalo_ctx* ctx, int frame_id, int counts[2]);
int nalo_map_get_frame(nalo_ctx* ctx, int frame_id, nalo_map_record* records, int cap, int* n);
int nalo_map_world_points(nalo_ctx* ctx, int frame_id, const double camToWorld[12], double* xyz /* n x 3 */, int cap, int* n);
int nalo_map_world_points_host(int n, const float* u, const float* v, const float* idepth, const float calib_inv[4], const double camToWorld[12], double* xyz /* n x 3 */);
int nalo_map_frame_cloud(nalo_ctx* ctx, nalo_map_cloud_args* args);

/* ------------------------------------------------------------------------------------------------
 * The keyframe graph: EnergyFunctional::connectivityMap, the argument of Output3DWrapper::publishGraph (FullSystem.cpp:1498-1502), for a caller that holds no
 * PointFrameResidual objects. The map's key is (host->frameID << 32) + target->frameID and its value {[0], [1]}; four events touch it in the reference:
 * insertFrame sets (new, f2) and (f2, new) to {0, 0} for every frame f2 of the window, (new, new) included (EnergyFunctional.cpp:453-458); insertResidual is [0]++
 * (:423); dropResidual is [0]-- (:493: removePoint of dropped and marginalised points, the removals of linearizeAll(true), FullSystem::marginalizeFrame for every
 * residual that targets the leaving frame); marginalizePointsF is [1]++ for every residual of a PS_MARGINALIZE point that isActive() after its re-linearisation
 * (:628-634). Entries are never erased: [0] is the number of residual objects that exist for the pair, in any state, 0 once one of its frames has left; [1] only
 * grows. Here the keys and [1] (marg) are a host table keyed by the caller's frame_id, and [0] (act) is counted from the resident slots when the graph is read.
 *
 * nalo_map_graph_enable(ctx, on)   opt-in and independent of nalo_map_enable: a context that never calls it enqueues and allocates exactly what it did before.
 *   Pairs     created when frames become co-resident, for every ordered pair of window frames without an entry, (f, f) included; an existing entry keeps its
 *             counts. nalo_ba_set_window (W frames leave what W insertFrames would: re-issuing the window every keyframe works as well), nalo_ba_carry_window with
 *             an entering frame and nalo_ba_window_from_initializer create them; turning the graph on while a window is set creates that window's.
 *             nalo_ba_marginalize_frame erases nothing. nalo_map_reset empties the table and leaves the pairs of the frames then in the window, as a fresh
 *             EnergyFunctional that has inserted them would. nalo_ba_snapshot / nalo_ba_restore do not include the table.
 *   marg      added by nalo_ba_marginalize_flagged and nalo_ba_marginalize_points alike, from the per-pair residual counts of the marginalisation pass the call
 *             fetches anyway (no launch, no wait of its own). Marginalisations made while the graph was off are not counted.
 *   frame_id  while on, a frame with a negative frame_id is refused by the call that would enter it - nalo_ba_set_window, nalo_ba_carry_window,
 *             nalo_ba_window_from_initializer: NALO_ERR_ARG, the window as it was (the reference asserts >= 0, PangolinDSOViewer.cpp:542) -, and so is turning the
 *             graph on over a window that holds one. The frames of a session need distinct ids.
 *   NALO_ERR_STATE on a sharded window and on a context whose exchange failed, as with nalo_map_enable.
 * nalo_map_graph   every entry in ascending key order (std::map's iteration order), the (f, f) entries {0, 0} included: *n is connectivity.size(), what
 *   SampleOutputWrapper::publishGraph prints. act of a pair of frames nalo_ba_get_frames returns now: the slots with a residual that belong to valid points hosted
 *   by the first frame, in the row of the second, counted by one kernel over the resident arrays; of any other pair: 0. Between nalo_ba_marginalize_frame and the
 *   carry the arrays stand in the old layout: the departed row is not read, which is what FullSystem::marginalizeFrame's drops leave. One launch, one 1 KB copy,
 *   one wait per call. cap < *n: NALO_ERR_ARG with *n set. NALO_ERR_STATE, outputs untouched: the graph is off; no window; the window's points are neither set
 *   nor carriable (nalo_ba_set_window with another size, a frame that left while it hosted points); a sharded window.
 * nalo_map_graph_connections   PangolinDSOViewer::publishGraph's list (IOWrapper/Pangolin/PangolinDSOViewer.cpp:528-571): the keys with host_id < target_id in
 *   key order, {fwdAct, fwdMarg} from the key and {bwdAct, bwdMarg} from the inverse key; *n is the viewer's runningID. from_id / to_id are the frame ids (the
 *   viewer looks its KeyFrameDisplays up by them). Cost and refusals as nalo_map_graph.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_graph_edge { int host_id, target_id, act, marg; } nalo_graph_edge;                       /* one entry of connectivityMap */
typedef struct nalo_graph_connection { int from_id, to_id, fwdAct, bwdAct, fwdMarg, bwdMarg; } nalo_graph_connection;   /* GraphConnection, ids instead of KeyFrameDisplay* */
int nalo_map_graph_enable(nalo_ctx* ctx, int on);
int nalo_map_graph(nalo_ctx* ctx, nalo_graph_edge* edges, int cap, int* n);
int nalo_map_graph_connections(nalo_ctx* ctx, nalo_graph_connection* conn, int cap, int* n);

/* ------------------------------------------------------------------------------------------------
 * The window panel: FullSystem::debugPlot (FullSystem/FullSystemDebugStuff.cpp:109-358, called from makeKeyFrame at FullSystem.cpp:1412 with
 * setting_render_renderWindowFrames = true and freeDebugParam5 = 1 by default) on the device: one image per window frame, the frame's level-0 irradiance (the
 * slot's planar I[0]) with a ring per point, the argument of IOWrap::displayImageStitch. Everything it reads is resident: the window's valid points, the archive
 * of removed points (nalo_map_enable), the resident immature set (nalo_imm_resident_*). The call has no side effect on window, archive, immature set, tracker or
 * graph, and a context that never calls it enqueues exactly what it did before. Kernels on the context's stream, ONE wait; the images come up through a pinned
 * block of the context and reach bgr only on success.
 *   Frames    bit i of frame_mask selects window frame i (the order of nalo_ba_get_frames); 0 selects every frame. The selected frames are painted in window
 *             order: n_frames images of h x w x 3 bytes, frame_id[j] the id of image j.
 *   Base      every mode (:180-185): c = (int)(I * 0.9f), 255 if larger, the byte (unsigned char)c on all three channels - nalo_trk_depth_image's base image, with
 *             its conversions (saturating float -> int, NaN -> 0, a negative c wraps).
 *   Lists     of a window frame, in painting order. active: its valid window points in submission order (status 1 of nalo_map_frame_cloud), idepth_scaled = the
 *             current inverse depth. marginalised / out: its status-2 / status-3 archive records in archive order, idepth_scaled = the record's idepth; both empty
 *             without an archive. immature: the resident points whose host_idx is the frame's window index, in storage order; empty without a resident set.
 *   Ring      setPixelCirc((int)(u + 0.5f), (int)(v + 0.5f), colour) (MinimalImage.h:112-126): the 40 pixels at Chebyshev distance 2 or 3 from the centre, not
 *             the centre and not its eight neighbours.
 *   Modes     mode = (int)(freeDebugParam5 + 0.5f). 0: active and marginalised makeRainbow3B(idepth_scaled), out white. 1: active rainbow, marginalised black,
 *             out white. 2, 8, 9: the base image only (no branch matches, as in the reference). 3: immature points with status IPS_GOOD, IPS_SKIPPED or
 *             IPS_BADCONDITION, black when idepth_max is not finite, else makeRainbow3B((idepth_min + idepth_max) * 0.5f). 4: the six status colours of :245-256.
 *             5: immature points that are not IPS_UNINITIALIZED, d = quality_scale * (sqrtf(quality) - 1) clamped to [0, 1] (sqrtf correctly rounded), colour
 *             Vec3b(0, d * 255, (1 - d) * 255). 6 (PointHessian::my_type, which the resident window does not hold): NALO_ERR_UNSUPPORTED. 7: active
 *             makeJet3B((idepth_scaled - minID) / (maxID - minID)), marginalised black; out points are not drawn but count in allID.
 *   Rainbow   makeRainbow3B (globalFuncs.h:334-348): id *= rainbow_scale (freeDebugParam3); !(id > 0) is white; icP = (int)id, ifP = id - icP, icP % 3 selects
 *             the branch; bytes 255 * (1 - ifP), 255 * ifP in float, truncated.
 *   Overlap   the reference paints the lists one after another, so the LAST writer of a pixel wins: list order (active, marginalised, out; immature alone), and
 *             inside a list ascending index. Exactly so here, on every run: a source raises a per-pixel key to its position in the frame's painting order with
 *             an integer maximum, and a second pass paints the winner. No float atomic, no atomic append.
 *   Mode 7    range (:118-158): allID = idepth_scaled of every active, marginalised and out point of ALL window frames, whatever frame_mask says; n_values is its
 *             size. With n = size - 1, minID / maxID are the order statistics at ranks (int)(n * 0.05) and (int)(n * 0.95), the products in double, found exactly
 *             by a radix select on the float bit patterns (-0 orders before +0); nothing is sorted and the count does not visit the host. Smoothing against
 *             minmax_io = {minIdJetVisDebug, maxIdJetVisDebug}, which stay with the caller (start them at -1 as FullSystem.cpp does): maxChange =
 *             (float)(0.1 * (double)(max - min)), 1e5 when either stored value is < 0, the four ifs in the reference's order, minmax_io rewritten. NULL: no
 *             smoothing, nothing written. minmax_io is read and written in mode 7 only.
 *   sources   sources[j] = rings painted into image j from {immature, active, marginalised, out} (clipped rings included).
 * DEFINED differences from the reference:
 *   1. MinimalImage::at() has no bounds check; here ring pixels outside the image are skipped (a ring wholly outside paints nothing).
 *   2. (int)(u + 0.5f) of a value int cannot hold saturates, NaN gives 0 (as the base image's conversion).
 *   3. makeRainbow3B of an id that int cannot hold (>= 2^31, +inf) paints the white pixel x86 produces (INT_MIN % 3 matches no branch); a NaN argument of
 *      makeJet3B paints white (as nalo_trk_depth_image).
 *   4. The bytes of mode 5 are truncated toward zero, saturated to 0..255, NaN -> 0 (nalo_map_frame_cloud's conversion).
 *   5. NaNs are left out of allID (the reference's std::sort is undefined on them).
 *   6. The order INSIDE a list is the library's (submission / archive / storage order); the reference's pointHessians is permuted by swap-with-back - the
 *      difference nalo_map_* documents. It shows only where two rings of one list with different colours overlap.
 * Where to call it: after nalo_ba_marginalize_flagged the lists are those of the reference at FullSystem.cpp:1453. Right after nalo_ba_optimize (the reference's
 *   place, :1412) the points removeOutliers has already moved to pointHessiansOut are still active in the chain - it decides them in nalo_ba_flag_points - and are
 *   drawn coloured instead of white.
 * Refusals, each leaving bgr, minmax_io and the context as they were. NALO_ERR_ARG: NULL ctx / args / bgr; mode outside 0..9; a frame_mask bit at or above the
 *   window size; rainbow_scale or quality_scale not finite. NALO_ERR_UNSUPPORTED: mode 6; more sources than a 32-bit key can index. NALO_ERR_STATE: no window; the
 *   window's point arrays are unset (between nalo_ba_marginalize_frame and the carry); a selected frame's slot without a pyramid; a sharded window (a rank holds
 *   only its own points); mode 7 with an empty allID (the reference indexes an empty vector; n_values = 0). NALO_ERR_HIP: a cross-rank exchange of this context
 *   failed earlier.
 * Out of scope: displayImageStitch's tiling, the dead `debugSaveImages && false` block. (debugPlotTracking: nalo_ba_residual_plot below; CoarseInitializer::debugPlot:
 *   nalo_init_depth_image.)
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_window_plot_args {
    int      mode;            /* (int)(freeDebugParam5 + 0.5f) of the reference: 0..9 */
    float    rainbow_scale;   /* freeDebugParam3 (settings.cpp:191), 1 in the reference */
    float    quality_scale;   /* freeDebugParam1 (mode 5), 1 in the reference */
    unsigned frame_mask;      /* bit i = window frame i is painted; 0 = every frame */
    float*   minmax_io;       /* mode 7: {minIdJetVisDebug, maxIdJetVisDebug}, caller-kept, start at -1 (FullSystem.cpp); NULL = no smoothing */
    uint8_t* bgr;             /* out: [n_frames][h][w][3], selected frames in window order, bytes of a pixel in Vec3b's order */
    int      n_frames;        /* out */
    int      frame_id[NALO_MAX_WINDOW];      /* out: of the painted frames */
    int      sources[NALO_MAX_WINDOW][4];    /* out: per painted frame, sources drawn from {immature, active, marginalised, out} */
    int      n_values;        /* out, mode 7: allID.size() */
    float    min_new, max_new, min_used, max_used;   /* out, mode 7, as in nalo_depth_image_args */
} nalo_window_plot_args;
int nalo_map_window_plot(nalo_ctx* ctx, nalo_window_plot_args* args);

/* ------------------------------------------------------------------------------------------------
 * The residual panel: one outer iteration of FullSystem::debugPlotTracking (FullSystem/FullSystemDebugStuff.cpp:52-107, call sites FullSystemOptimize.cpp:471,598)
 * with PointFrameResidual::debugPlot (Residuals.cpp:278-302), for host frame `host`, on the device: every window frame brightness-transferred into the host's
 * photometric frame, the pattern pixels of every residual of the host's points coloured by energy or by state on their TARGET's image, and a 3x3 square per point
 * on the host's own image - the argument of IOWrap::displayImageStitch. The diagnostic that shows where residuals land and which are outliers. It has no side
 * effect on the window, and a context that never calls it enqueues exactly what it did before. Kernels on the context's stream, ONE wait; the images come up
 * through a pinned block of the context and reach bgr only on success.
 *
 * nalo_ba_get_pattern_projections(ctx, projected, state_energy): what the painter draws from, for a caller (or a test) that wants the numbers. projected is
 *   [P*W][8][2], state_energy [P*W], slot order p*W + t as nalo_ba_get_residuals; either may be NULL. projected = PointFrameResidual::projectedTo[idx]
 *   (Residuals.cpp:186-200): projectPoint (ResidualProjections.h:47-57) of the eight pattern pixels with the precalc record of the (host, target) pair the last
 *   linearisation read (PRE_KRKiTll, PRE_KtTll) and the point's CURRENT inverse depth - ptp = (KRKi(i,0) x + KRKi(i,1) y + KRKi(i,2)) + Kt(i) idepth per row, in
 *   float, without FMA contraction; Ku = ptp[0] / ptp[2], Kv = ptp[1] / ptp[2]. One device function computes it for this call and for the painter.
 *   state_energy = PointFrameResidual::state_energy. A slot that does not exist, whose point has been removed, or whose state is OOB holds the sentinel 2.f in
 *   all sixteen coordinates (what the linearisation initialises them with) and 0 in state_energy. Preconditions and refusals are nalo_ba_get_residuals' own.
 *
 * nalo_ba_residual_plot:
 *   Frames    bit i of frame_mask selects window frame i (the order of nalo_ba_get_frames) to be RETURNED; 0 selects every frame. n_frames images of h x w x 3
 *             bytes in window order, frame_id[j] the id of image j. The counters below cover every target, whatever the mask says.
 *   Base      of image f2 (:72-82): aff[j] = AffLight::fromToVecExposure(f2.ab_exposure, host.ab_exposure, f2.aff_g2l(), host.aff_g2l()) in double on the host,
 *             from the frame states the context holds (what nalo_ba_get_frames reports): a = exp(SCALE_A (host.state[6] - f2.state[6])) * host.ab_exposure /
 *             f2.ab_exposure (both exposures 1 when either is 0), b = SCALE_B host.state[7] - a SCALE_B f2.state[7]. Per pixel colL = (float)(a * I + b) with the
 *             product and the sum in double, clamped <0 -> 0, >255 -> 255, the byte on all three channels. NaN fails both clamps: DEFINED byte 0.
 *   Residuals for every valid point of the host, in submission order (the active list of nalo_map_window_plot), and every residual slot of it that exists and
 *             whose state is not OOB: colour cT, energy mode (free_debug_param5 == 0): rT = (float)(20 * sqrt((double)(state_energy / 9))) - the quotient in
 *             float, ::sqrt and the product in double as the reference's overloads resolve -, clamped to [0, 255], Vec3b(0, 255 - rT, rT), each byte truncated;
 *             a NaN rT gives (0, 0, 0). State mode (anything else): IN (255, 0, 0), OUTLIER (0, 0, 255), anything else white. For each of the eight pattern
 *             pixels with Ku > 2 && Kv > 2 && Ku < w - 3 && Kv < h - 3 (float compares), pixel ((int)(Ku + 0.5f), (int)(Kv + 0.5f)) of the TARGET's image
 *             becomes cT (setPixel1).
 *   Square    setPixel9((int)(u + 0.5), (int)(v + 0.5), makeRainbow3B(idepth_scaled)) on the HOST's own image: the sums in double as `ph->u + 0.5` is,
 *             idepth_scaled = SCALE_IDEPTH x the current inverse depth, freeDebugParam3 = rainbow_scale (nalo_map_window_plot's Rainbow).
 *   Overlap   the last writer in point order wins, exactly so on every run: an integer maximum of (position in the host's list + 1) per pixel, then a pass that
 *             paints the winner or the base. One point has at most one residual per target, so the order inside a point never matters; squares and pattern
 *             pixels never share an image, because a residual's target is never its host (a slot in the host's own row is not drawn). No float atomic.
 *   Counters  n_points: valid points of the host; n_residuals: residuals drawn (existing, not OOB); n_pattern_pixels: pattern pixels that passed the guard.
 * DEFINED differences from the reference:
 *   1. The order inside the host's list is the library's (submission order); the reference's pointHessians is permuted by swap-with-back. It shows only where
 *      pixels of two points with different colours coincide.
 *   2. Projections are recomputed from the current state instead of being stored by the last linearize. They are the same values right after nalo_ba_optimize /
 *      nalo_ba_linearize, which is where the reference calls the function (up to FMA contraction inside the linearisation: an ulp, far below the half pixel
 *      that moves a painted pixel, except for a coordinate that lies on a rounding boundary).
 *   3. Pixels of a square outside the image are skipped; (int)(u + 0.5) of a value int cannot hold saturates, NaN gives 0; makeRainbow3B as in
 *      nalo_map_window_plot's difference 3.
 *   4. displayImageStitch's tiling and waitKey stay with the caller.
 * Refusals, each leaving the outputs and the context as they were. NALO_ERR_ARG: NULL ctx / args / bgr; host or a frame_mask bit at or above the window size;
 *   rainbow_scale or free_debug_param5 not finite. NALO_ERR_STATE: no window; the window's point arrays are unset (between nalo_ba_marginalize_frame and the
 *   carry); a selected frame's slot without a pyramid; a sharded window. NALO_ERR_HIP: a cross-rank exchange of this context failed earlier.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_residual_plot_args {
    int      host;                /* window index of the host frame */
    float    free_debug_param5;   /* == 0: energy colours, anything else: state colours (Residuals.cpp:283) */
    float    rainbow_scale;       /* freeDebugParam3, 1 in the reference */
    unsigned frame_mask;          /* bit i = the image of window frame i is returned; 0 = every frame */
    uint8_t* bgr;                 /* out: [n_frames][h][w][3], selected frames in window order, bytes of a pixel in Vec3b's order */
    int      n_frames;            /* out */
    int      frame_id[NALO_MAX_WINDOW];      /* out: of the painted frames */
    double   aff[NALO_MAX_WINDOW][2];        /* out: the affL each painted image was transferred with */
    int      n_points, n_residuals, n_pattern_pixels;   /* out */
} nalo_residual_plot_args;
int nalo_ba_get_pattern_projections(nalo_ctx* ctx, float* projected, float* state_energy);
int nalo_ba_residual_plot(nalo_ctx* ctx, nalo_residual_plot_args* args);

/* ------------------------------------------------------------------------------------------------
 * The 3-D panel of PangolinDSOViewer (IOWrapper/Pangolin/PangolinDSOViewer.cpp:186-236: per keyframe drawCam, refreshPC, drawPC(1); the dense clouds; the current
 * camera; drawConstraints :448-526; KeyFrameDisplay::drawCam / drawPC, KeyFrameDisplay.cpp:609-722) for a card without OpenGL or a display: one call, one wait, an
 * RGB image (and optionally its depth) up. Everything it draws is resident: the window's points, the immature set, the archive of removed points, the dense
 * archive, the graph's counts. GL's rasterisation is implementation defined, so this is a DEFINED rasteriser; tests/render_model.py is its literal model. The call
 * has no side effect on window, archives, immature set, tracker or graph.
 *
 *   Transforms  per listed frame f, M_f = (float)(viewFromWorld . camToWorld_f): the product on the host in double, entry (r, c) =
 *               (V[r][0] C[0][c] + V[r][1] C[1][c]) + V[r][2] C[2][c], then + V[r][3] for c = 3, then the cast. V_f = (float)viewFromWorld serves the world-space
 *               lines. Applying a transform to (x, y, z) is, in float with every operation rounded (no contraction), row r: ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3].
 *   Points      the records of a listed frame are exactly nalo_map_frame_cloud's for that frame (status 0 from the resident immature set when with_immature, 1 from
 *               the window, 2 and 3 from the archive), its filter (display_mode, scaledTH, absTH, minRelBS) and its colours, by the same device functions. Each
 *               survivor gives the 8 vertices of the no-jitter form (z = depth; the viewer's rand() jitter is not reproduced). With with_dense every dense-archive
 *               point of the frame with !(idepth < 0) gives one vertex, as nalo_map_dense_cloud's no-jitter form. A vertex goes through M_f to (xv, yv, zv) and is
 *               drawn iff zv > znear && zv < zfar and, with u = fx * (xv / zv) + cx and v = fy * (yv / zv) + cy in float, u >= 0 && u < vw && v >= 0 && v < vh
 *               (NaNs fall out through the comparisons). It lands on pixel ((int)floorf(u), (int)floorf(v)) with depth zv. Point size 1.
 *   Lines       one list of segments with float endpoints. drawCam's eight segments per listed frame when show_kf_cams (blue, sz = 0.1f, width 1) and for
 *               currentCamToWorld when show_current_cam (red, sz = 0.2f, width 2): apex (0, 0, 0) and the corners (sz * (0 - cx) / fx, sz * (0 - cy) / fy, sz) ..
 *               (sz * (w - 1 - cx) / fx, sz * (h - 1 - cy) / fy, sz) in float as written at :630-649, from the window's current calibration (value_scaledf) and
 *               the level-0 size, through M_f. The constraints, from nalo_map_graph_connections' list with the rules of :458-491: a connection with an end that
 *               is not in frames[] is skipped (the reference's `== 0`); nAct == 0 && nMarg > 0 draws green, width 1, when show_all_constraints; nAct > 0 draws
 *               blue, width 3, when show_active_constraints; the ends are the translations of camToWorld cast to float. show_trajectory: the strip through the
 *               listed frames' translations, red, width 3; show_full_trajectory: the strip through all_poses, green, width 3. These go through V_f.
 *               From view space on a segment is handled in double. It is dropped when a coordinate is not finite or both z <= znear. Otherwise an end with
 *               z < znear is replaced by A + t (B - A), t = (znear - za) / (zb - za), A and B the ends as given. The ends are projected, u = fx * (x / z) + cx;
 *               a segment with a projection that is not finite is dropped. n_segments counts the segments that remain. n = ceil(max(|ub - ua|, |vb - va|)).
 *               The parameter range [t0, t1] of the segment inside [-2, vw + 2] x [-2, vh + 2] comes from a Liang-Barsky clip (edges in the order left, right,
 *               top, bottom; p = -du, du, -dv, dv; q = ua + 2, (vw + 2) - ua, va + 2, (vh + 2) - va; r = q / p); an empty range gives no sample. n == 0: the one
 *               sample k = 0, t = 0. Else k = k0 .. k1 with k0 = ceil(t0 n), k1 = floor(t1 n), at most vw + vh + 10 of them (the first ones), so the work is
 *               bounded whatever the ends are. Sample k: t = k / n, (u, v) = (ua + t (ub - ua), va + t (vb - va)), depth = (float)(1 / ((1 - t) / za + t / zb));
 *               it is kept iff depth > znear && depth < zfar (n_line_samples counts these) and paints, for width L, the pixels (floor(u) + ox, floor(v) + oy),
 *               ox, oy in [-(L / 2), (L - 1) / 2], that lie inside the image (square caps, no anti-aliasing).
 *   Depth test  per pixel the candidate with the smallest depth wins (a positive float orders like its bit pattern); among equal depths the smallest
 *               (R << 16) | (G << 8) | B. One 64-bit integer minimum per candidate: no float atomic, no submission order, the same bytes on every run. A pixel
 *               without a candidate gets background, and +inf in depth.
 *   Counts      n_vertices: the vertices of the survivors of refreshPC's filter (8 per sparse survivor, 1 per dense one; without with_dense the sum of
 *               nalo_map_frame_cloud's n over the listed frames); n_drawn_points: those inside the frustum and the viewport; n_segments, n_line_samples: above.
 *   Refusals    nothing is enqueued; rgb, depth and every context state stay as they were (the four counts are zeroed). NALO_ERR_ARG: NULL ctx / args / rgb; vw or
 *               vh < 1, vw * vh > 2^26; a camera value or viewFromWorld entry that is not finite; znear <= 0 or zfar <= znear; n_frames < 0 or frames NULL with
 *               n_frames > 0 (all_poses alike); a frame_id listed twice, or one that is neither in the window nor in either archive; sparsity > 1.
 *               NALO_ERR_STATE: no window (its CalibHessian is the clouds' calibration); a listed window frame while the window's points are unset (between
 *               nalo_ba_marginalize_frame and the carry); a constraint flag with the graph off (and nalo_map_graph's own refusals); with_dense with the dense
 *               archive off; a sharded window; a context whose exchange failed. n_frames == 0 is legal: the background and the world-space lines.
 *   Cost        three kernels on the context's stream (points, lines, resolve) and ONE wait; with a constraint flag nalo_map_graph's launch and wait come first.
 *               The key plane cleans itself: it is filled only when it is allocated or grown.
 * nalo_view_look_at (host only): pangolin::ModelViewLookAt in double - z = (eye - target) / |eye - target|, x = up x z, y = z x x, x and y normalised, lengths as
 *   sqrt((a a + b b) + c c) - converted to x right, y down, z forward: rows x, -y, -z, translation row r = -((R[r][0] ex + R[r][1] ey) + R[r][2] ez). The viewer's
 *   start view is eye (0, -5, -10), target (0, 0, 0), up (0, -1, 0). NALO_ERR_ARG (nothing written) where pangolin throws: x or y of length 0, or not finite.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_view_frame { int frame_id; double camToWorld[12]; } nalo_view_frame;   /* a KeyFrameDisplay: id + the pose it was last set with */
typedef struct nalo_map_render_args {
    int vw, vh;                       /* output size */
    float fx, fy, cx, cy, znear, zfar;/* the panel's camera: the reference uses 400, 400, w/2, h/2, 0.1, 1000 (PangolinDSOViewer.cpp:95) */
    double viewFromWorld[12];         /* row-major 3x4, x right, y down, z forward */
    int n_frames; const nalo_view_frame* frames;      /* `keyframes`, in the viewer's order */
    int display_mode, with_immature, sparsity; float scaledTH, absTH, minRelBS;   /* as nalo_map_cloud_args */
    int with_dense;                   /* the second loop, :229-233 */
    int show_kf_cams, show_current_cam; double currentCamToWorld[12];
    int show_active_constraints, show_all_constraints, show_trajectory, show_full_trajectory;
    int n_all_poses; const float* all_poses;          /* allFramePoses [n][3] */
    uint8_t background[3];
    uint8_t* rgb;                     /* out, vh*vw*3, row 0 on top, R,G,B */
    float* depth;                     /* out, optional, vh*vw: the winner's view-space z, +inf where nothing was drawn */
    long long n_vertices, n_drawn_points, n_segments, n_line_samples;   /* out */
} nalo_map_render_args;
int nalo_map_render(nalo_ctx* ctx, nalo_map_render_args* args);
int nalo_view_look_at(const double eye[3], const double target[3], const double up[3], double viewFromWorld[12]);   /* host only */

/* ------------------------------------------------------------------------------------------------
 * The mesh in the 3-D panel. nalo_map_render_mesh(ctx, r, m) is DEFINED as nalo_map_render(ctx, r) with a third kind of candidate in the same depth test: the
 * triangles of up to three meshes that lie in device memory - the welded archive (nalo_tsdf_archive_view's arrays), the device mesh the last mesh call left
 * (nalo_tsdf_mesh_view, nalo_tsdf_mesh_color_view) and a caller's. Every candidate - point, line sample, triangle pixel - is entered into the key plane before
 * the resolve pass; the key plane, the resolve pass and the ONE host wait are nalo_map_render's. A DEFINED rasteriser: the same bytes on every run, equal bit for
 * bit to the literal model tests/render_mesh_model.py. nalo_map_render itself, its struct and its bytes are unchanged, and with no source selected the outputs of
 * nalo_map_render_mesh equal nalo_map_render's bit for bit. No side effect on volume, archive, device mesh, window or any other state of the context.
 *
 *   Sources     visited in the order archive, live mesh, user. The order is not observable except through the counts, which are sums. Mesh positions are world
 *               coordinates: vertex (x, y, z) goes through V_f = (float)viewFromWorld with the rounded `apply` of "Transforms" above, as the world-space lines do,
 *               to its view-space (xv, yv, zv).
 *   Classes     per triangle (i0, i1, i2) of a source with nv vertices the class is the FIRST rule that fires:
 *               1 bad index   some index is < 0 or >= nv (the user source only: the library's own meshes hold none).
 *               2 near        some view-space coordinate is not finite, or some zv fails zv > znear. A DELIBERATE difference from GL and from the lines above:
 *                             there is NO near-plane clipping; a triangle that reaches the near plane is not drawn. Mesh triangles are at most a voxel across.
 *               3 guard       per vertex u = fx * (xv / zv) + cx and v = fy * (yv / zv) + cy in float, as for points; the rule fires unless
 *                             -131072 < u && u < 131072 and the same for v (a NaN falls out through the comparisons). Then the vertex is snapped to 8 sub-pixel
 *                             bits, every operation rounded in float:  X = (int)floorf(u * 256.0f + 0.5f),  Y = (int)floorf(v * 256.0f + 0.5f).
 *               4 degenerate  A = (X1 - X0) * (Y2 - Y0) - (Y1 - Y0) * (X2 - X0) in 64-bit integers; A == 0 fires. If A < 0, vertices 1 and 2 are exchanged with
 *                             everything they carry (z, colour), so that A > 0 from here on.
 *               5 large       the box of the pixels (ix, iy) whose centres (256 ix + 128, 256 iy + 128) lie inside [minX, maxX] x [minY, maxY] is clipped to the
 *                             viewport; a box of more than max_box_pixels pixels (0 = 65536) fires. A call's work is bounded by n_triangles * max_box_pixels
 *                             whatever a caller submits.
 *               0 drawn       otherwise. An empty box draws nothing.
 *   Coverage    for the edges 0->1, 1->2, 2->0 (after the exchange) from A to B, with d = B - A and E(P) = dx * (Py - Ay) - dy * (Px - Ax) in 64-bit integers at
 *               the pixel centre P: the pixel is covered iff every edge has E > 0, or E == 0 and the edge is top-left, dy < 0 || (dy == 0 && dx > 0). A mesh
 *               whose edges run through pixel centres covers every pixel exactly once; two triangles that share an edge never both take a pixel. The weights
 *               are w0 = E12(P), w1 = E20(P), w2 = E01(P); they sum to A. With the guard and vw, vh <= 65536 every product stays below 2^52, so the conversions
 *               to double below are exact.
 *   Depth       in double, z_i the float zv of vertex i: t_i = (double)w_i / (double)z_i, q = (t0 + t1) + t2, depth = (float)((double)A / q). The pixel gets a
 *               candidate iff depth > znear && depth < zfar; n_tri_pixels counts these.
 *   Colour      colour_mode 0, per channel with c_i the vertex's byte: val = (((t0 * c0) + (t1 * c1)) + (t2 * c2)) / q, byte = min(255, (int)floor(val + 0.5)).
 *               Alpha is ignored. colour_mode 1, once per triangle, in double from the float view-space vertices in SUBMITTED order: e1 = P1 - P0, e2 = P2 - P0,
 *               n = e1 x e2 (nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z, nz = e1x e2y - e1y e2x: two rounded products and a rounded difference each),
 *               len = sqrt((nx nx + ny ny) + nz nz), s = len > 0 ? fabs(nz) / len : 0, g = (int)floor(64.0 + 191.0 * s), colour (g, g, g): a triangle seen
 *               edge-on is 64, one that faces the viewer 255.
 *   Key         (depth bits << 32) | R << 16 | G << 8 | B, one 64-bit integer minimum, as for points and lines: among equal depths the smaller colour word
 *               wins, whatever kind of candidate it belongs to.
 *   Arithmetic  the double divisions and the square root are the correctly rounded ones, no operation is contracted.
 *   Counts      n_triangles: the triangles of the selected sources; n_tri_bad_index .. n_tri_large: those of classes 1-5; n_tri_pixels above.
 *   Stream      a user source's arrays are read behind everything queued on its producer_stream at the time of the call (an event, on the device, as
 *               nalo_tsdf_integrate_depth); the call ends with its host wait, so the arrays are the caller's again when it returns.
 *   Refusals    nothing is queued; rgb, depth, the context, the device mesh and the archive stay as they were; all eleven counts are zeroed. Every refusal of
 *               nalo_map_render applies, with one exception: a window is required only when n_frames > 0, show_kf_cams or show_current_cam is set - a context
 *               that has only a volume can draw its mesh (and the world-space strips). NALO_ERR_ARG: NULL m; vw or vh > 65536; colour_mode outside 0..1;
 *               negative max_box_pixels; a user source with a negative count, a count > 2^31 - 1, or a NULL xyz / tri with a positive count. NALO_ERR_STATE:
 *               with_archive without an enabled archive; with_live_mesh before any mesh call; colour_mode 0 with a selected source that has no colours - an
 *               uncoloured archive, a live mesh left by the plain nalo_tsdf_mesh, a user rgba that is NULL with n_vertices > 0.
 *   Cost        one more kernel on the context's stream (all sources in one launch), between the lines and the resolve pass; still ONE wait.
 * nalo_view_triangle (host only, no context): rules 2-5 for one triangle given by its view-space vertices, through the function the kernel calls. Of cam it
 *   reads vw, vh, fx, fy, cx, cy, znear. cls: 0 drawn, or 2..5. X, Y: the snapped coordinates after the exchange (0 where rule 2 or 3 fired). box: the clipped
 *   box x0, x1, y0, y1, inclusive; (0, -1, 0, -1), so x1 < x0, when it is empty or rules 2-4 fired. NALO_ERR_ARG (nothing written): a NULL argument, vw or vh
 *   outside 1..65536, a negative max_box_pixels.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_render_mesh_src {            /* a caller's mesh in device memory */
    const float* xyz; const int* tri; const uint8_t* rgba;   /* [nv][3], [nt][3], [nv][4] or NULL */
    long long n_vertices, n_triangles;
    void* producer_stream;                       /* as nalo_tsdf_integrate_args; NULL = the null stream */
} nalo_render_mesh_src;
typedef struct nalo_map_render_mesh_args {
    int with_archive;                            /* the triangles of nalo_tsdf_archive_view */
    int with_live_mesh;                          /* the device mesh the last mesh call left (nalo_tsdf_mesh_view) */
    const nalo_render_mesh_src* user;            /* optional third source */
    int colour_mode;                             /* 0 vertex colours, 1 shaded grey */
    long long max_box_pixels;                    /* 0 = 65536 */
    long long n_triangles, n_tri_bad_index, n_tri_near, n_tri_guard, n_tri_degenerate, n_tri_large, n_tri_pixels;  /* out */
} nalo_map_render_mesh_args;
int nalo_map_render_mesh(nalo_ctx* ctx, nalo_map_render_args* r, nalo_map_render_mesh_args* m);
int nalo_view_triangle(const nalo_map_render_args* cam, const float view_xyz[3][3], long long max_box_pixels,
                       int* cls, int X[3], int Y[3], int box[4]);   /* host only, no context */

/* ------------------------------------------------------------------------------------------------
 * densemap=1: DenseMapping::updateMap (FullSystem/MapPoint.cpp:234-332, call site FullSystem.cpp:1488-1496) in one call, and FrameHessian::mapPoints as a
 * device archive beside the sparse one. The per-cluster route (nalo_dense_fit_planes, then nalo_dense_make_map per cluster) stays as it is.
 *
 * nalo_dense_update_map   for the window's frame host_frame: the clusters and planes nalo_dense_fit_planes returns for the same arguments (the same code path;
 *   clusters[] is filled as that call fills it), then per cluster, in record order, the loop of MapPoint.cpp:271-331 and makeMap:
 *     not fitted              the reference's `continue` (:280-281): runs[k] = {zero rect, n = 0, accept = 0, first = -1}
 *     mask_value == 0         rect = its box of the MASK scan (:300-310), nothing else (`if(pcolor==0) return;`, :355-357)
 *     otherwise               rect, then the pixel loop of :367-401 over the box with its exclusive upper bounds and the extent test of :403 (the order-dependent
 *                             maxy / maxz of SURVEY App. C.6 included): n = the points the loop kept, accept = the test (0 when n == 0: nothing to append;
 *                             nalo_dense_make_map reports the test on the untouched seeds there, which passes).
 *   rect is {INT_MAX, INT_MIN, INT_MAX, INT_MIN} when the value is nowhere in [2,w-2)x[2,h-2). The arithmetic is nalo_dense_make_map's (shared functions): the
 *   two routes are equal bit for bit.
 *   The kept points of every accepted cluster are appended to the dense archive under the frame's frame_id (nalo_frame_state): cluster order, raster order
 *   inside a cluster - the order of fh->mapPoints.insert(...). A rejected cluster appends nothing; a second call for the same frame appends a second set of runs
 *   (the reference does the same when a frame is third from last on two keyframes). runs[k].first = the position of the cluster's first point in the frame's
 *   dense list, -1 when it appended nothing. No point crosses the bus: the records, the runs and the two counts come up.
 *   Waits: two per call, none per cluster - one for the records and boxes (the host sizes the batched grid from them), one at the end; plus one, with a blocking
 *   copy of the chunk table, in a call for which the archive allocates a chunk (never in steady state).
 *   Reservation: room for every candidate of the scanned range (the pixels of [2,w-2)x[2,h-2) with i%3==0 || j%3==0; a pixel belongs to one cluster, so the count
 *   bounds the call) is reserved before anything is touched: a refusal for lack of memory leaves the archive as it was.
 *   Refusals (nothing appended, context usable): whatever nalo_dense_fit_planes refuses, with its codes (cap too small: NALO_ERR_ARG with *n_clusters set);
 *   NALO_ERR_STATE the dense archive is not enabled, the frame's slot has no mask; NALO_ERR_ARG camToWorld, runs or n_appended NULL.
 *
 * nalo_map_dense_enable(ctx, on, chunk_points)   the archive grows in chunks of chunk_points 16-byte points; 0 = 262144 (4 MiB: two to three keyframes of ~10^5
 *   points per allocation, and small enough that the unused tail of the last chunk does not matter). The size in force at the first allocation holds for the
 *   context. A chunk is allocated once and never moved; in steady state nothing is allocated. Independent of nalo_map_enable. Images wider or higher than 65535
 *   are refused (NALO_ERR_UNSUPPORTED: u, v are 16 bits). MEMORY: about 1.6 MB per keyframe at 10^5 points, released only by nalo_map_reset (which empties this
 *   archive too and keeps its chunks for reuse) and nalo_destroy. nalo_ba_snapshot / nalo_ba_restore do not include it.
 * nalo_map_dense_counts   the frame's points and appended cluster runs. NALO_ERR_ARG for a frame_id the dense archive has never seen (here and below).
 * nalo_map_dense_get      the frame's points in append order; cap < *n: NALO_ERR_ARG with *n set.
 * nalo_map_dense_world_points  SampleOutputWrapper's tsdf=1 loop over mapPoints (SampleOutputWrapper.h:152-176): one lane per point, in append order, through the
 *   function nalo_map_world_points and nalo_io_write_pcd_points share, with (float)u, (float)v and the window's float inverse calibration: equal bit for bit to
 *   nalo_map_world_points_host on the records of nalo_map_dense_get. cap < *n: NALO_ERR_ARG with *n set. One wait.
 * nalo_map_dense_cloud    KeyFrameDisplay::refreshPC() (IOWrapper/Pangolin/KeyFrameDisplay.cpp:212-271): idepth < 0 skips (NaN takes the branch the comparison
 *   gives it: it stays); depth = 1.0f / idepth; x = (u * fxi + cxi) * depth, y alike; z = depth * (1 + 2 * fxi * (r / (float)RAND_MAX - 0.5f)) with
 *   RAND_MAX = 2^31 - 1 and r = draws[j] for OUTPUT vertex j (rand() is drawn for survivors only: an ordered compaction); draws == NULL: z = depth. Colour is
 *   {bgr[2], bgr[1], bgr[0]}. {fxi, fyi, cxi, cyi}: the window's CalibHessian values, as nalo_map_frame_cloud takes them. cap (always) or n_draws (with draws)
 *   below the frame's record count: NALO_ERR_ARG with n_needed set. records = the frame's points, survivors = n. One wait.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_dense_run {             /* one per cluster record, same index as the nalo_plane_cluster beside it */
    int rect[4];                            /* minx, maxx, miny, maxy of the MASK scan; zeros for a cluster that was not fitted */
    int n;                                  /* points makeMap's loop kept (mpcache.size()) */
    int accept;                             /* the extent test of :403; 0 when n == 0 */
    long long first;                        /* position of the run's first point in the frame's dense list, -1 when nothing was appended */
} nalo_dense_run;
typedef struct nalo_dense_point { uint16_t u, v; float idepth; float color; uint8_t bgr[3]; uint8_t pad; } nalo_dense_point;   /* 16 bytes; MapPoint{u, v, idepth, color, bgr} */
typedef struct nalo_map_dense_cloud_args {
    int frame_id;
    int n_draws; const int* draws;          /* NULL: no jitter */
    int cap; float* xyz; uint8_t* rgb;      /* cap vertices: [cap][3] each */
    int n, n_needed;                        /* out: vertices written; the frame's records (what cap and n_draws must reach) */
    int records, survivors;                 /* out */
} nalo_map_dense_cloud_args;
int nalo_dense_update_map(nalo_ctx* ctx, int host_frame, const nalo_plane_fit_args* fit, const double camToWorld[12], int cap, nalo_plane_cluster* clusters,
                          nalo_dense_run* runs, int* n_clusters, int* n_appended);
int nalo_map_dense_enable(nalo_ctx* ctx, int on, int chunk_points);
int nalo_map_dense_counts(nalo_ctx* ctx, int frame_id, int* n_points, int* n_runs);
int nalo_map_dense_get(nalo_ctx* ctx, int frame_id, nalo_dense_point* out, int cap, int* n);
int nalo_map_dense_world_points(nalo_ctx* ctx, int frame_id, const double camToWorld[12], double* xyz /* n x 3 */, int cap, int* n);
int nalo_map_dense_cloud(nalo_ctx* ctx, nalo_map_dense_cloud_args* args);

/* ------------------------------------------------------------------------------------------------
 * tsdf=1: the dense map fused into a TSDF volume on the device. The reference constructs a cpu_tsdf::TSDFVolumeOctree (FullSystem.cpp:192-198), saves a point
 * file "for tsdf" (SampleOutputWrapper.h:150-176, nalo_map_dense_world_points here) and leaves the fusion to a third-party tool it neither vendors nor pins. This
 * section is a DEFINED operation instead: a projective integration of one depth image into a dense voxel volume that lives in the context. Colour is opt-in
 * ("Colour" below; the reference's switch is tsdf->setIntegrateColor, FullSystem.cpp:195). No octree; taking a fused plane back, or fusing at a corrected pose and scale: "The replacement" below; a volume that follows the camera: nalo_tsdf_shift; nalo_ba_snapshot / nalo_ba_restore do
 * not include the volume.
 *
 * nalo_tsdf_create   origin: world position of the CORNER of voxel (0,0,0); dims = {nx, ny, nz}. Storage: two contiguous F32 arrays [nz][ny][nx], x fastest;
 *                    tsdf starts at 1.0f, weight at 0.0f. NALO_ERR_ARG: a dimension outside [1, 2048], nx ny nz above 2^29, voxel_size / trunc / max_weight not
 *                    finite or <= 0, a non-finite origin. A failed allocation (NALO_ERR_HIP) leaves the context, and a volume it holds, as they were. A second
 *                    create replaces the volume (it waits for the main stream first).
 * nalo_tsdf_reset    the initial values again, the memory stays. nalo_tsdf_destroy frees the volume (no volume: NALO_OK); nalo_destroy frees it too.
 *                    nalo_map_reset does NOT touch the volume. Every other call of this section without a volume: NALO_ERR_STATE.
 *
 * nalo_tsdf_integrate_depth   everything in float, no FMA contraction, each operation rounded once:
 *     M = worldToCam: the 3x3 block of camToWorld transposed and -(R^T t), each row's three products summed left to right, in double; every entry then rounded to float.
 *     voxel (i, j, k):  px = origin[0] + ((float)i + 0.5f) * voxel_size, py and pz alike;  xc = ((M0 px + M1 py) + M2 pz) + M3, yc and zc alike (rows of M);
 *     uf = ((fx * (xc / zc)) + cx) + 0.5f, vf alike. Visible iff zc > 0 && uf >= 0 && uf < w && vf >= 0 && vf < h, compared in float BEFORE any conversion
 *     (a NaN fails); the pixel is ((int)uf, (int)vf). D = depth[pv][pu] is usable iff D >= min_depth && D <= max_depth. sdf = D - zc; skipped when sdf < -trunc.
 *     Otherwise, with t0 = tsdf, w0 = weight, d = fminf(1.0f, sdf / trunc):   tsdf = (t0 * w0 + d) / (w0 + 1.0f);   weight = fminf(w0 + 1.0f, max_weight).
 *   One lane owns a voxel for the whole call: no float atomic, the same bytes on every run. The kernel visits only the box of nalo_tsdf_frustum_box; a voxel
 *   the definition updates is always inside it (the box is conservative), so the result equals the definition evaluated on every voxel.
 *   depth: F32, one channel, w x h given by the plane - it need NOT be the context's size, K = {fx, fy, cx, cy} comes with the call for that size - any strides
 *   nalo_dev_plane_check accepts; no byte outside the described elements is read.
 *   Stream order as nalo_frame_ingest_device: the main stream waits on the device for what producer_stream has queued (skipped for the context's own stream), and
 *   an event is recorded behind the kernel, the last one that reads the plane; nalo_tsdf_release(ctx, stream) lets `stream` wait for it on the device (nothing to wait
 *   for: NALO_OK). With the volume allocated the call makes no host wait.
 *   NALO_ERR_ARG: a plane nalo_dev_plane_check refuses (host memory among them), a dtype other than F32, three channels, a non-finite entry of K or camToWorld,
 *   min_depth or max_depth not finite, min_depth > max_depth. A refused call queues nothing and leaves volume and context as they were.
 * nalo_tsdf_integrate_frame   DEFINED as nalo_tsdf_integrate_depth on the plane D[v][u] = 1.0f / idepth of the LAST record at (u, v) of the frame's dense list in
 *   append order (nalo_map_dense_get's order), 0 where there is none; the plane is context-owned scratch of the context's w x h. A second nalo_dense_update_map of
 *   the same frame appended a second set of runs: the last record is settled by an integer key (the record's position in the list), never by arrival order.
 *   NALO_ERR_ARG for a frame_id the dense archive has never seen; NALO_ERR_STATE without the dense archive (nalo_map_dense_enable) or on a sharded window.
 * nalo_tsdf_last     waits once. The last integration's visited box (lo inclusive, hi exclusive, voxel indices; all zero when the box was empty), the voxels
 *                    visited (the box's volume) and the voxels updated (an integer sum: a wave reduction, then one atomic per workgroup). NALO_ERR_STATE
 *                    before the first integration into this volume.
 * nalo_tsdf_get / nalo_tsdf_set   read-back / injection of the sub-block [lo, lo + size) as [size[2]][size[1]][size[0]] floats, x fastest; either array may be
 *                    NULL (not both). nalo_tsdf_set is to this volume what nalo_trk_set_depth is to the tracker. NALO_ERR_ARG for a block that is empty or leaves the
 *                    grid. Synchronous.
 * nalo_tsdf_view     host code only, launches nothing: the pointers of both arrays, the dimensions and the producing stream (nalo_stream), under "Lifetime of
 *                    a view" above: good until a non-zero nalo_tsdf_shift / nalo_tsdf_create / nalo_tsdf_destroy / nalo_destroy; the calls that rewrite what it names are nalo_tsdf_reset,
 *                    nalo_tsdf_set and the two integrations.
 * nalo_tsdf_surface_points   over the sub-box [lo, lo + size) (use_box == 0: the whole grid): for voxel v in ascending (k, j, i) and axis a = x, y, z, with n the
 *                    neighbour of v along +a INSIDE the sub-box, (v, a, n) is a crossing iff both weights are >= min_weight and (t0 < 0 && t1 >= 0) || (t0 >= 0 &&
 *                    t1 < 0) (a NaN fails both clauses); its point is centre(v) + e_a * (voxel_size * (t0 / (t0 - t1))), centre(v) the px, py, pz above.
 *                    Output in that order: a count pass, a scan, a write pass; no atomic append. n_needed is always set; cap < n_needed: NALO_ERR_ARG and nothing
 *                    is written. One wait. The call uses 1 B of context-owned scratch per sub-box voxel (the mesh's mask bytes: these are its axis vertices).
 * nalo_tsdf_frustum_box   host only, needs no context: the culling box. In double: the world box of the camera apex (camToWorld's t) and the four far corners, the
 *                    rays through (uf, vf) in {0, w} x {0, h}, i.e. x = ((uf - 0.5) - cx) / fx, y = ((vf - 0.5) - cy) / fy, at z = max_depth + trunc. Per axis
 *                    lo = floor((min - origin) / voxel_size - 0.5) - 1 and hi = ceil((max - origin) / voxel_size - 0.5) + 2, clipped to [0, dim]: the voxels whose
 *                    centres lie in the box, padded by one voxel on every side (hi exclusive). An empty box on any axis gives all zeros. NALO_ERR_ARG for a
 *                    descriptor nalo_tsdf_create refuses, w or h < 1, a non-finite K, pose or max_depth.
 *
 * The mesh. The reference includes cpu_tsdf/marching_cubes_tsdf_octree.h next to the octree volume (FullSystem.h:45-47): what its tsdf=1 mode is built towards is
 * a surface mesh, extracted by a tool it neither vendors nor pins. nalo_tsdf_mesh is a DEFINED, deterministic, indexed triangle list instead: marching tetrahedra
 * on the Kuhn split of every cell (no 256-case table, no ambiguous case; the face diagonals of neighbouring cells agree by translation, so the surface is closed
 * wherever the data is). Everything in float, no FMA contraction, each operation rounded once. Over the sub-box [lo, lo + size) (use_box == 0: the whole grid):
 *   Validity and sign: a voxel is VALID iff weight >= min_weight and its tsdf is not NaN; it is INSIDE iff tsdf < 0 (-0.0f and 0.0f are outside). centre(v) is
 *     the px, py, pz of the integration above.
 *   Edges and vertices: voxel v owns seven edges m = 1..7 from v to n = v + d_m, d_m = (m & 1, (m >> 1) & 1, (m >> 2) & 1): the axis edges m = 1, 2, 4, the face
 *     diagonals 3, 5, 6, the body diagonal 7. (v, m) carries a vertex iff n lies inside the sub-box, both ends are valid and exactly one end is inside. With
 *     s = t0 / (t0 - t1) and prod = voxel_size * s, each computed once, its position is centre(v) with prod added to every component a for which d_m[a] == 1.
 *     Vertices are numbered from 0 in ascending (k, j, i) of v, then ascending m. A vertex that no triangle names is legal (the rim of the valid band).
 *     The vertices with m in {1, 2, 4}, in order, are exactly nalo_tsdf_surface_points of the same sub-box and min_weight, bit for bit.
 *   Cells and tetrahedra: cell c has corners c + bits(b), b = dx + 2 dy + 4 dz = 0..7; it is LIVE iff all eight lie inside the sub-box and are valid. A live cell
 *     is cut into T0..T5 with corners (c0, c1, c2, c3) = (0,1,3,7), (0,1,5,7), (0,2,3,7), (0,2,6,7), (0,4,5,7), (0,4,6,7). Every tetrahedron edge joins corners
 *     p < q whose bits nest (p & q == p); its vertex is the one owned by voxel c + bits(p) with m = q ^ p.
 *   Triangles of a tetrahedron: mask has bit r set iff c_r is inside; X.Y is the vertex on edge XY. mask 0 or 15: none. One corner alone (one inside or one
 *     outside): with L that corner and O1, O2, O3 the others in ascending r, the triangle (L.O1, L.O2, L.O3). Two and two: insiders I1, I2 and outsiders O1, O2
 *     in ascending r give the quad q0 = I1.O1, q1 = I1.O2, q2 = I2.O2, q3 = I2.O1 and the triangles (q0, q1, q2), (q0, q2, q3).
 *   Winding: with every vertex at the midpoint of its edge in the unit cube, a triangle (A, B, C) is kept as written when ((B - A) x (C - A)) . (mean of the
 *     outside corners - mean of the inside corners) > 0, else its last two vertices are swapped (the product is never zero: an integer at doubled coordinates).
 *     The normal points from tsdf < 0 to tsdf >= 0, towards the camera that saw the surface.
 *   Order: ascending (k, j, i) of the cell, then T0..T5, then the order above.
 * nalo_tsdf_mesh     reads the volume only and always builds the mesh into context-owned device buffers; n_vertices / n_triangles are what the device mesh holds.
 *                    A host array that is given (non-NULL) is filled when its cap suffices. A classify pass (5 B of scratch per sub-box voxel), two scans, a
 *                    vertex and a triangle pass; no atomic append, the same bytes on every run; one host wait when nothing is downloaded and the buffers suffice
 *                    (they grow to what a call finds plus a quarter, and the two write passes run again). NALO_ERR_ARG, with nothing written to either host
 *                    array: a negative cap, a cap > 0 with a NULL array, a NaN min_weight, a sub-box that is empty or leaves the grid or holds more than 2^28
 *                    voxels (seven vertices a voxel must fit an int index) - such a call queues nothing and leaves volume, context and the previous device mesh as
 *                    they were, with both counts 0 - and a cap below the count of an array that is given: that is known only behind the scans, so the device
 *                    mesh IS built and both counts are set. NALO_ERR_STATE without a volume. A failed allocation (NALO_ERR_HIP) leaves the previous mesh whole.
 * nalo_tsdf_mesh_view   host code only, launches nothing: the device mesh ([n_vertices][3] float, [n_triangles][3] int) and its producing stream, under "Lifetime
 *                    of a view": good until the next nalo_tsdf_mesh, nalo_tsdf_create, nalo_tsdf_destroy or nalo_destroy. NALO_ERR_STATE before the first mesh.
 * nalo_tsdf_mesh_table  host only, needs no context: the table the kernels use, built from the rules above at compile time. For tetrahedron t and mask the six
 *                    entries are the vertices of up to two triangles in output order, each coded 8 p + (q ^ p), -1 as padding; 120 triangles in all.
 *
 * Colour. Opt-in: a context that never calls nalo_tsdf_color_enable queues what it queued before and produces the same bits. Everything in float, no FMA
 * contraction, each operation rounded once; no float atomic, the same bytes on every run.
 * nalo_tsdf_color_enable   three contiguous F32 arrays [3][nz][ny][nx], the planes in B, G, R order (as the slots store colour), each laid out as tsdf; they start
 *                    at 0.0f. NALO_ERR_STATE without a volume; already enabled: NALO_OK and nothing changes; a failed allocation (NALO_ERR_HIP) leaves volume
 *                    and context as they were. Enable BEFORE the first integration if the colour is to be the average of every observation: enabling later is
 *                    legal, and the running average then starts from 0 under the weight that is already there (the first colours are pulled towards black).
 * nalo_tsdf_color_disable  frees the planes (it waits for the main stream first); not enabled: NALO_OK. nalo_tsdf_reset sets them to 0.0f; nalo_tsdf_create
 *                    replaces the volume WITHOUT colour; nalo_tsdf_destroy and nalo_destroy free them.
 * nalo_tsdf_integrate_depth_color   nalo_tsdf_integrate_depth, and at every voxel its definition updates, with (pu, pv) that voxel's pixel, w0 the weight BEFORE
 *                    this update and (b, g, r) the colour bytes at the pixel, for each plane X with byte x:   X = (X0 * w0 + (float)x) / (w0 + 1.0f).
 *                    A voxel the definition does not update keeps its three words bit for bit. colour: U8, three channels, exactly the depth plane's w x h, any
 *                    strides nalo_dev_plane_check accepts (HWC, CHW, pitched, x-strided); colour_is_rgb: channel 0 is R. NALO_ERR_ARG otherwise, also for a
 *                    NULL colour; NALO_ERR_STATE without colour enabled; the refusals of nalo_tsdf_integrate_depth are unchanged and a refused call queues
 *                    nothing. Stream order and nalo_tsdf_release as there: producer_stream produces both planes, and the recorded event lies behind the one
 *                    kernel that reads either. The colour of a lane's four voxels is loaded and stored only where tsdf and weight are stored.
 *                    nalo_tsdf_integrate_depth on a coloured volume stays legal: it updates tsdf and weight and leaves the colour untouched, so the average
 *                    counts that observation as one more of the colour the voxel already holds: its weight grows, its colour does not move.
 *                    nalo_tsdf_integrate_frame on a coloured volume integrates colour too: the colour at (u, v) is the bgr of the same LAST record that
 *                    supplies idepth, (0, 0, 0) where there is none (this shows when min_depth <= 0 makes D = 0 usable), settled by the same integer key.
 * nalo_tsdf_color_get / nalo_tsdf_color_set   the sub-block [lo, lo + size) as [3][size[2]][size[1]][size[0]] floats, planes B, G, R, bit for bit (NaN payloads
 *                    pass). Refusals as nalo_tsdf_get / nalo_tsdf_set, and NALO_ERR_STATE without colour. Synchronous.
 * nalo_tsdf_color_view   host code only, launches nothing: the pointer of the [3][nz][ny][nx] block, the dimensions and the producing stream, under "Lifetime of
 *                    a view": good until a non-zero nalo_tsdf_shift / nalo_tsdf_color_disable / nalo_tsdf_create / nalo_tsdf_destroy / nalo_destroy. NALO_ERR_STATE without colour.
 * nalo_tsdf_mesh_color   everything nalo_tsdf_mesh does - the same definition, order, counts, growth protocol and refusals - and one colour per vertex, in vertex
 *                    order, into a context-owned device buffer [n_vertices][4] of bytes that grows with xyz. For the vertex on edge (v, m) with far end n and the
 *                    s = t0 / (t0 - t1) of its position, per plane:   cX = X(v) + s * (X(n) - X(v));   byte = (uint8)(int)(fminf(fmaxf(cX, 0.0f), 255.0f) + 0.5f).
 *                    A NaN gives 0 through fmaxf (a NaN s from an infinite corner among them). The four bytes are R, G, B, 255: one aligned store per vertex,
 *                    written by the vertex pass. NALO_ERR_STATE without colour. NALO_ERR_ARG, with nothing written to ANY host array: a NULL argument, a
 *                    negative cap, cap > 0 with a NULL rgba, and an rgba that is given with cap below n_vertices (known behind the scans: the device mesh is
 *                    built and the counts are set, as for xyz).
 * nalo_tsdf_mesh_color_view   host code only, launches nothing: the device colours of the last mesh. NALO_ERR_STATE unless the LAST mesh call was
 *                    nalo_tsdf_mesh_color: a plain nalo_tsdf_mesh afterwards invalidates it. nalo_tsdf_mesh_view keeps working after either.
 *
 * The ray-cast. What the fused model looks like from a pose: a depth, a normal and a colour image of the volume's zero crossing, without a mesh and without a GL
 * context. The reference never reads its octree, so nalo_tsdf_raycast is a DEFINED operation: a march at a fixed step, trilinear over cells whose eight corners
 * are all valid, the first front face. Everything in float, no FMA contraction, each operation rounded once; no float atomic, the same bytes on every run.
 *   Ray: for pixel (u, v) of the w x h view with K = {fx, fy, cx, cy} (any size, not the context's):  rx = ((float)u - cx) / fx,  ry = ((float)v - cy) / fy - the
 *     inverse of the integration's (int)(fx * (xc / zc) + cx + 0.5f) at the pixel centre. With R and t the entries of camToWorld, each rounded to float:
 *     d_a = (R[a][0] * rx + R[a][1] * ry) + R[a][2],  o_a = t_a  (a = x, y, z). The ray is parametrised by camera-z: its point at z is p_a = o_a + d_a * z.
 *   Samples: z_n = min_depth + (float)n * step. N is the number of n in 0..4096 with z_n <= max_depth, evaluated in float with that expression (they form a
 *     prefix: z_n does not decrease with n). nalo_tsdf_raycast_steps computes N and refuses (NALO_ERR_ARG) when z_4096 <= max_depth, so 1 <= N <= 4096.
 *     The grid coordinate of a point is q_a = ((p_a - origin_a) / voxel_size) - 0.5f: voxel centres are the integers.
 *   Field S(q): i_a = floorf(q_a), f_a = q_a - i_a. The sample is VALID iff for every axis i_a >= 0.0f && i_a <= (float)(dim_a - 2), compared in float BEFORE
 *     any conversion (a NaN or an infinity fails; a grid with a dimension of 1 has no cell), and the eight corners (ix + dx, iy + dy, iz + dz), dx, dy, dz in
 *     {0, 1}, are all valid in the mesh's sense: weight >= min_weight and tsdf not NaN. With t_zyx the tsdf of corner (dx, dy, dz) = (x, y, z) - the digits of t
 *     read z, y, x, so t001 is the corner one step along +x - and a_yz the value interpolated along x on the edge with those y and z:
 *       a00 = t000 + fx * (t001 - t000),  a10 = t010 + fx * (t011 - t010),  a01 = t100 + fx * (t101 - t100),  a11 = t110 + fx * (t111 - t110)   (fx = f_x here),
 *       b0 = a00 + fy * (a10 - a00),  b1 = a01 + fy * (a11 - a01),  S = b0 + fz * (b1 - b0).
 *     A NaN S (inf - inf among infinite corners) makes the sample INVALID.
 *   March: the smallest n in [1, N) whose samples n - 1 and n are both VALID and differ in (S < 0) ends the ray. S_{n-1} >= 0 && S_n < 0 is a HIT (-0.0f is
 *     outside, as in the mesh); the other order is a BACK face and the pixel is a miss. An invalid sample breaks the pairs on both its sides: nothing is
 *     interpolated across it. No such n, or N < 2: a miss.
 *   Hit: s = S_{n-1} / (S_{n-1} - S_n),  depth = z_{n-1} + step * s;  q* is the grid coordinate of the ray's point at z = depth.
 *   Normal (with_normals): G_a = S(q* + e_a) - S(q* - e_a), the shifted coordinate q*_a + 1.0f and q*_a - 1.0f in float. All six samples must be VALID, else the
 *     normal is (0, 0, 0) and the pixel stays a hit. len = sqrt((Gx * Gx + Gy * Gy) + Gz * Gz), correctly rounded; if len > 0 and finite the normal is G_a / len,
 *     else zeros. World axes (the grid is axis-aligned); it points from tsdf < 0 to tsdf >= 0, towards the camera that saw the surface: the mesh's orientation.
 *   Colour (with_colour): per plane the trilinear expression above at q* on the colour plane; only the index test applies, the weights are not consulted.
 *     byte = (uint8)(int)(fminf(fmaxf(c, 0.0f), 255.0f) + 0.5f), the mesh colour's conversion (a NaN gives 0); the bytes are R, G, B, 255. Where the index
 *     test fails at q* (a NaN depth): 0, 0, 0, 255.
 *   Miss: depth 0.0f, normal zeros, rgba 0, 0, 0, 0. nalo_tsdf_integrate_depth ignores a depth of 0 for min_depth > 0: the plane can be integrated as it stands.
 *   The kernel: one lane per pixel, a wave an 8 x 8 tile, a workgroup 16 x 16. A lane visits only a conservative interval of n: the slab test of its ray against
 *     the cells' region, widened and clipped to [0, N). Samples outside the region fail the index test and an invalid sample never forms a pair, so the result
 *     equals the definition evaluated at every n. n_hit, n_back (rays a back face ended) and n_normal (non-zero normals) are integer sums: wave reductions,
 *     then one atomic per workgroup.
 * nalo_tsdf_raycast  reads the volume only. The images live in context-owned device buffers that grow when a larger view is asked for, are never shrunk and are
 *                    freed with the volume. A host array that is given is filled through pinned staging, and only on success; NULL leaves that image on the
 *                    device. One host wait per call, for the counts and whatever is downloaded. A context that never ray-casts queues what it queued before.
 *                    NALO_ERR_STATE: no volume; with_colour without colour enabled. NALO_ERR_ARG: NULL args; w or h < 1 or w * h > 2^26; a non-finite entry
 *                    of K or camToWorld; fx or fy equal to 0; min_depth, max_depth or step not finite, min_depth < 0, min_depth > max_depth, step <= 0, more
 *                    than 4096 steps; a NaN min_weight; a host normal or rgba given without its with_ flag. A refused call queues nothing, leaves volume,
 *                    context, the previous device images and every host array as they were, and zeroes the counts. A failed allocation (NALO_ERR_HIP)
 *                    leaves the previous images whole.
 * nalo_tsdf_raycast_view   host code only, launches nothing: the images of the last ray-cast as nalo_dev_plane descriptors (depth: F32, one channel, what
 *                    nalo_tsdf_integrate_depth takes as it is; normal: F32, three channels interleaved; rgba: U8, the channels R, G, B at stride_x 4 - the
 *                    alpha byte lies between pixels - so a colour plane with colour_is_rgb = 1) and the producing stream, under "Lifetime of a view": good
 *                    until the next nalo_tsdf_raycast, nalo_tsdf_create, nalo_tsdf_destroy or nalo_destroy. An image the last call was not asked for has a
 *                    NULL ptr. NALO_ERR_STATE before the first ray-cast.
 * nalo_tsdf_raycast_steps  host only, needs no context: N of the definition. NALO_ERR_ARG as nalo_tsdf_raycast refuses the three values, and for a NULL n_steps.
 *
 * A volume that follows the camera. The volume keeps the origin it was created with, origin0, and an integer base[3], zero at nalo_tsdf_create. The origin
 * every other call of this section uses is origin[a] = origin0[a] + (float)base[a] * voxel_size, in float, the product rounded, then the sum, no FMA: recomputed
 * from origin0 at every shift and never accumulated, so a base that returns to 0 returns origin0 bit for bit.
 * nalo_tsdf_shift    with s = shift and n = dims: after the call voxel (i, j, k) holds, in tsdf, weight and (with colour enabled) the three colour planes, the
 *                    words voxel (i + s[0], j + s[1], k + s[2]) held before it, copied as 32-bit words: NaN payloads, -0.0f and denormals pass unchanged.
 *                    Where that voxel lies outside the grid, the voxel takes the initial values: tsdf 1.0f, weight 0.0f, colour 0.0f. base[a] += s[a]: a
 *                    positive s[a] moves the box towards +a in the world, the slab of s[a] voxels at the low end leaves and a slab of initial values enters
 *                    at the high end. The pass is out of place (a parallel move in place would overwrite words another workgroup still has to read): it
 *                    writes a second set of arrays and swaps the two sets. The spare tsdf and weight arrays are allocated at the first non-zero shift, the
 *                    spare colour block at the first non-zero shift of a coloured volume; they are kept, and freed with the volume or the colour: A VOLUME THAT
 *                    HAS BEEN SHIFTED HOLDS TWICE ITS MEMORY. With the spares in place a shift allocates nothing, makes no host wait and enqueues on the main
 *                    stream only. A failed allocation (NALO_ERR_HIP) leaves everything as it was. A shift of (0, 0, 0) is NALO_OK and queues, swaps and
 *                    allocates nothing. A context that never shifts queues exactly what it queued before.
 *                    Behind a non-zero shift: nalo_tsdf_last is NALO_ERR_STATE until the next integration (its box was in the old indices); the device mesh
 *                    and the ray-cast images stay valid (they are in world coordinates); the event nalo_tsdf_release waits for is untouched. nalo_tsdf_reset
 *                    resets the values and keeps base; nalo_tsdf_create starts from base = 0; nalo_tsdf_color_enable works as before; nalo_tsdf_color_disable
 *                    frees both colour blocks. Lifetime of a view: nalo_tsdf_view and nalo_tsdf_color_view are good only until the next non-zero
 *                    nalo_tsdf_shift, because the pointers swap.
 *                    NALO_ERR_STATE without a volume; NALO_ERR_ARG for a NULL shift, for any |base[a] + s[a]| > 2^24 (the sum taken in 64 bits; at the bound
 *                    the conversion to float is still exact) and for a resulting origin that is not finite. A refused call queues nothing and leaves volume,
 *                    colour, geometry, views and nalo_tsdf_last as they were.
 *                    The kernel is driven from the destination: as in the integration a lane owns four voxels consecutive in memory and 16-byte aligned by
 *                    linear index and issues one 16-byte store per array; its loads are 16 bytes where the four sources lie in one row at a 16-byte aligned
 *                    index (for nx a multiple of four: s[0] % 4 == 0), else four words. It reads 4 B and writes 4 B per voxel and array: 16 B per voxel, 40 B
 *                    with colour.
 * nalo_tsdf_geometry host only, launches nothing: desc with the CURRENT origin - the descriptor nalo_tsdf_frustum_box wants after a shift, and what a twin
 *                    volume is created from - origin0 and base. NALO_ERR_STATE without a volume.
 * nalo_tsdf_shift_for   host only, needs no context: the shift that puts the voxel containing `centre` at index dims[a] / 2, with a dead band. In double:
 *                    q = floor((centre[a] - origin[a]) / voxel_size); d = q - (double)(dims[a] / 2); shift[a] = |d| > margin[a] ? (int)d : 0. NALO_ERR_ARG for
 *                    a descriptor nalo_tsdf_create refuses, a non-finite centre, a negative margin, |d| > 2^24, a NULL pointer; shift is then not written.
 * nalo_tsdf_shift_boxes host only, needs no context: the sub-boxes of the volume as it is BEFORE nalo_tsdf_shift(shift) that a caller meshes (or reads surface
 *                    points or a block from) so that no cell is lost. Per axis, with n voxels and shift s, the kept voxels are [s, n) for s > 0 and [0, n + s)
 *                    for s < 0; a cell survives iff all eight of its corners are kept. The leaving voxel range includes the seam voxel: [0, min(s + 1, n)) for
 *                    s > 0, [max(n + s - 1, 0), n) for s < 0. |s| >= n on any axis: everything leaves, the one box is the whole grid and kept_lo / kept_size
 *                    are zeros. Otherwise up to three boxes, in this order: X = leaving x by all y by all z; Y = kept x by leaving y by all z; Z = kept x by
 *                    kept y by leaving z; an axis with s = 0 contributes none. The cells of the boxes are pairwise disjoint and their union is exactly the
 *                    cells that do not survive (nalo_tsdf_mesh cuts cells at a sub-box's faces). Unused entries of lo / size are zero. NALO_ERR_ARG for a
 *                    NULL pointer or a dimension outside [1, 2048].
 *
 * The mesh archive. The meshes of the boxes that leave a following volume, kept on the device as ONE indexed triangle list and welded by vertex identity, not by
 * position: the seam voxels stay in the volume and keep integrating, and the origin is recomputed at every shift, so the later copy of a seam vertex lies
 * somewhere else in its last bits or more. The archive lives in the context next to the volume and outlives it: nalo_tsdf_create, nalo_tsdf_destroy and
 * nalo_tsdf_reset leave its contents alone (a drive may replace its volume); nalo_destroy frees it.
 *   Identity: the vertex nalo_tsdf_mesh places on edge (v, m) of sub-box [lo, lo + size) has the KEY (gx, gy, gz, m), g = base + lo + (i, j, k) of v with the
 *     base nalo_tsdf_geometry reports at the time of the call: four ints, one 16-byte word. |base| <= 2^24 and a dimension <= 2048: nothing overflows. Two
 *     vertices are the same vertex iff their keys are equal. Within one mesh all keys are distinct (an edge carries at most one vertex); duplicates arise
 *     only between a piece and what was archived before it.
 *   Append of a piece (the device mesh a mesh call left): its vertices are visited in the piece's order. A vertex whose key the archive holds is dropped and
 *     its index maps to the archived one: the FIRST occurrence's position and colour win. Every other vertex is added at the end, in order, its xyz, rgba and
 *     key copied as words (a NaN position passes). Then all the piece's triangles are added at the end, in order, with mapped indices. Triangles are never
 *     deduplicated: the same box archived twice adds no vertex and every triangle a second time.
 *   Lattice: the archive belongs to one lattice. Its first successful append records the volume's origin0 and voxel_size as words (nalo_tsdf_archive_reset
 *     forgets them); the same lattice re-created is accepted.
 * nalo_tsdf_archive_enable   allocates the archive (4096 vertices, 8192 triangles, 8192 table slots) and empties it. It is COLOURED iff there is a volume and its
 *                    colour is enabled at that moment. Already enabled: NALO_OK, nothing changes. A failed allocation (NALO_ERR_HIP) leaves the context as it
 *                    was. A context that never enables the archive queues exactly what it queued before.
 * nalo_tsdf_archive_disable  frees it (it waits for the main stream first); not enabled: NALO_OK.
 * nalo_tsdf_archive_reset    empties it and keeps its buffers and its colour state; queues one fill of the table, no wait.
 * nalo_tsdf_archive_mesh     DEFINED as nalo_tsdf_mesh(ctx, m) - nalo_tsdf_mesh_color with no host colours when the archive is coloured - followed by the append
 *                    of the device mesh. The host arrays and caps in m are honoured as nalo_tsdf_mesh honours them; the device mesh and nalo_tsdf_mesh_view
 *                    (and nalo_tsdf_mesh_color_view) behind the call are exactly what the mesh call alone leaves. out (may be NULL): the vertices added, the
 *                    vertices welded and the triangles added by this call, and what nalo_tsdf_archive_stats reports.
 *                    The passes, all on the main stream: a key pass directly behind the mesh (it reads the mesh passes' scratch, which
 *                    nalo_tsdf_surface_points would overwrite); a read-only lookup, one lane per piece vertex, through an open-addressed table of 32-bit
 *                    slots (an archived index or empty; keys are compared through the archive's key array, one 16-byte load); a scan of the "new" flags; a
 *                    pass that writes the new vertices and inserts them with one 32-bit atomicCAS on an empty slot each (all inserted keys are distinct and
 *                    absent); a triangle pass. Which slot a key lands in is not observable; everything observable is fixed by the definition: the same
 *                    bytes on every run, no float atomic. Before launching, the host makes room for the worst case, every piece vertex new: buffers grow to
 *                    what is needed plus a quarter (contents copied on the device), the table to the power of two that keeps its load at or below one half,
 *                    rebuilt from the key array in one pass. Every probe loop is bounded by the slot count; a lane that exhausts it raises a device flag,
 *                    the call returns NALO_ERR_HIP and the table is rebuilt from the vertices the archive held: nothing spins.
 *                    Host waits: the mesh call's own (one, two when its buffers grow or a host array is filled) and ONE for the append, for the count of new
 *                    vertices and the flag. An empty piece appends without a wait.
 *                    NALO_ERR_STATE: the archive is not enabled, or there is no volume - nothing is queued. Every refusal of nalo_tsdf_mesh applies unchanged,
 *                    and a cap below the count of a host array that is given (the device mesh IS built) appends nothing. NALO_ERR_STATE, with the plain
 *                    nalo_tsdf_mesh of the box built as a mesh call would: a volume whose colour state differs from the archive's, or whose origin0 or
 *                    voxel_size differ from the recorded ones. NALO_ERR_ARG, behind the mesh: an archive that would pass 2^31 - 1 vertices or triangles with
 *                    every piece vertex counted as new. A refused or failed call, a failed growth (NALO_ERR_HIP) included, leaves the archive as it was,
 *                    bit for bit.
 * nalo_tsdf_archive_stats    host only, launches nothing: the last nalo_tsdf_archive_mesh's three counts (zeros behind enable and reset), the totals, the
 *                    capacities, the table's slots, the colour state and the lattice (have_lattice 0: none recorded yet).
 * nalo_tsdf_archive_get      copies to the host: xyz [n_vertices][3], tri [n_triangles][3], rgba [n_vertices][4], key [n_vertices][4], each optional (NULL) and
 *                    each with its own cap, under the cap / count protocol of nalo_tsdf_mesh: n_vertices / n_triangles are always set; NALO_ERR_ARG with
 *                    nothing written to ANY array for a negative cap, a cap > 0 with a NULL array, or a cap below the count of an array that is given.
 *                    NALO_ERR_STATE for an rgba given to an uncoloured archive. One wait when anything is copied.
 * nalo_tsdf_archive_view     host only, launches nothing: the device arrays (rgba NULL in an uncoloured archive), the counts and the producing stream, under
 *                    "Lifetime of a view": good until the next nalo_tsdf_archive_mesh that grows a buffer, or until nalo_tsdf_archive_reset,
 *                    nalo_tsdf_archive_disable or nalo_destroy. A later append that does not grow only adds behind the counts the view holds.
 * nalo_tsdf_archive_get, _view and _stats are NALO_ERR_STATE before nalo_tsdf_archive_enable.
 * nalo_tsdf_follow   the loop that keeps a volume around the camera, DEFINED as exactly these calls, in order, with nothing new underneath:
 *                    nalo_tsdf_geometry; nalo_tsdf_shift_for(desc, centre, margin); if the shift is non-zero, nalo_tsdf_shift_boxes and
 *                    nalo_tsdf_archive_mesh(box, min_weight, no host arrays) on each box in order; nalo_tsdf_shift. The first call that fails ends it with that
 *                    call's code (a refusal of nalo_tsdf_shift_for or nalo_tsdf_shift_boxes: NALO_ERR_ARG). shift_out (may be NULL) takes the shift; stats
 *                    (may be NULL) the number of boxes, the sums of the three per-call counts and the archive's totals. NALO_ERR_STATE with the archive
 *                    disabled or without a volume, before anything else.
 *
 * The alignment. Whether a depth plane fits the model it is about to be fused into: a direct alignment of the plane against the signed-distance field, the
 * step every dense fusion pipeline has in front of its integration (the reference fuses with the pose it is given). DEFINED here; it reads volume and plane and
 * changes neither. The estimate is (R, t, s): camToWorld as nalo_tsdf_integrate_depth takes it (12 doubles, rigid) and a scale s > 0, 1 unless the monocular
 * window's gauge is in doubt; dof = 6 keeps s fixed, dof = 7 estimates it.
 * nalo_tsdf_align_eval   one evaluation at one estimate, in ONE kernel launch. Per pixel everything in float, no FMA contraction, each operation rounded once:
 *     Visited: pixel (u, v) of the plane iff u % step == 0 && v % step == 0. The plane: F32, one channel, its own w x h and K, any strides nalo_dev_plane_check accepts.
 *     D is usable iff D >= min_depth && D <= max_depth (a NaN fails). rx, ry as in the ray-cast; pc = (rx * D, ry * D, D).
 *     M = [s R | t], 3 x 4, each entry formed in double (s * R[a][j]; t[a]) and rounded to float; pw_a = ((M_a0 pcx + M_a1 pcy) + M_a2 pcz) + M_a3;
 *     q_a = ((pw_a - origin_a) / voxel_size) - 0.5f, the ray-cast's grid coordinate.
 *     r = S(q), the ray-cast's field with its validity rule and min_weight (one device function serves both kernels). G_a = S(q + e_a) - S(q - e_a) as for the
 *     ray-cast's normal, all six samples VALID; g_a = G_a * (0.5f / voxel_size), the quotient computed once.
 *     State, the first rule that fires: 1 D not usable; 2 S(q) invalid; 3 a gradient sample invalid; 0 used.
 *     J = (g, pw x g, g . (pw - tf)), tf = M_a3: each entry of the cross product two rounded products and a rounded difference, (pw_y g_z - pw_z g_y,
 *     pw_z g_x - pw_x g_z, pw_x g_y - pw_y g_x); the dot summed left to right; J_6 is 0.0f for dof = 6. The tangent is translation, then rotation, then log s.
 *     hw = fabsf(r) <= huber ? 1.0f : huber / fabsf(r);  Jw_i = hw * J_i.
 *   Sums over the used pixels, in double: H_ij = sum (double)Jw_i (double)J_j for i <= j; b_i = sum (double)Jw_i (double)r; rr = sum (double)r (double)r -
 *     every term an exact product of two floats - and E = sum rho, rho = (double)r (double)r for fabsf(r) <= huber, else huber * (2.0 * |r| - huber) in double.
 *     nalo_tsdf_align_sums holds the 37: H's upper triangle row-major (H[0][0..6], H[1][1..6], ...), b, E, rr; and count[state], four integers.
 *   No float or double atomic: lanes reduce inside the wave, waves through LDS, each workgroup writes one partial record, and the workgroup that draws the last
 *     (integer) ticket adds the records in workgroup order: the same bytes on every run of the same launch configuration (plane size and step).
 *   records (optional, DEVICE memory, records_cap floats >= h w 10): [h][w][10] = r, hw, J0..J6, (float)state, written at visited pixels only; every field but
 *     the state is 0.0f unless the state is 0. Without it the kernel stores nothing per pixel.
 *   Stream order as nalo_tsdf_integrate_depth (producer_stream, the event nalo_tsdf_release waits for). The sums come up through host-mapped memory: one host wait.
 * nalo_tsdf_align_step   host only, needs no context: one Levenberg-Marquardt step in fp64. Hl = H with its diagonal scaled by 1 + lambda; inc = solve(Hl, -b)
 *     over the leading dof x dof block by Cholesky (inc[6] = 0 for dof = 6); (R, t) <- exp(inc[0..5]) . (R, t), s <- s * exp(inc[6]). NALO_ERR_ARG, with
 *     nothing written: a NULL pointer, dof outside {6, 7}, a lambda that is negative or not finite, an Hl or b that is not finite or an Hl that is not positive
 *     definite, an estimate or an update that is not finite.
 * nalo_tsdf_align_depth  the Levenberg-Marquardt loop, driven by the host: one launch per evaluation, its 37 doubles and four counts read from host-mapped
 *     memory behind one wait, the 7 x 7 system solved on the host (nalo_tsdf_align_step). With n = count[0]:
 *       evaluate est_in; fewer than max(min_used, 1) used pixels: NALO_TSDF_ALIGN_TOO_FEW. lambda = lambda0 (0: the default 0.01). Then up to max_iterations times:
 *       (inc, cand) = step(H, b, lambda) of the current estimate (refused: NALO_TSDF_ALIGN_SOLVE_FAILED, the loop ends); evaluate cand; it is accepted iff
 *       n_new >= max(min_used, 1) && E_new / n_new < E / n - then it becomes the current estimate and lambda *= 0.5, else lambda *= 4; then, if
 *       sqrt(sum inc_i^2) <= eps: NALO_TSDF_ALIGN_CONVERGED. All iterations used: NALO_TSDF_ALIGN_ITERATION_LIMIT.
 *     result: the current estimate (est_in itself when no step was accepted), status, iterations (steps taken), evaluations, E and n of the first evaluation and
 *     of the current estimate, the current estimate's sums, and a trace the caller caps: one entry per evaluation, in order - estimate, the lambda its step was
 *     solved with (lambda0 for the first), E, the counts, accepted (1 for the first). n_trace = min(evaluations, trace_cap).
 * nalo_tsdf_align_frame  to nalo_tsdf_align_depth what nalo_tsdf_integrate_frame is to nalo_tsdf_integrate_depth: the same context-owned plane of the frame's
 *     dense list (last-record rule, one code path), args->K for the context's w x h; args->depth and producer_stream are not looked at. The same refusals.
 * Refusals: nothing is queued; volume, context, plane and outputs stay as they were; the counts (count[], iterations, evaluations, n_first, n_last, n_trace)
 *     are zeroed. NALO_ERR_STATE: no volume. NALO_ERR_ARG: a NULL pointer; a plane nalo_tsdf_integrate_depth would refuse; step < 1; dof outside {6, 7}; a
 *     non-finite pose, K, s or threshold (min_depth, max_depth, huber); s <= 0; huber <= 0; min_depth > max_depth; a NaN min_weight; records given with
 *     records_cap < h w 10; and for the loop max_iterations outside 1..64, a lambda0 or eps that is negative or not finite, a negative trace_cap, trace_cap > 0
 *     with a NULL trace.
 *
 * The replacement. A keyframe is fused with the pose and depth it has when it is made; the window then moves its pose (nalo_ba_optimize), the scale fix rescales
 * it (nalo_ba_plane_scale_fix), and nalo_tsdf_align_depth with dof = 7 returns an estimate (R, t, s) the plain integration cannot take. This is the DEFINED
 * removal of one plane's contribution and its fusion again at another estimate, without nalo_tsdf_reset and a second fusion of every frame.
 * A side (nalo_tsdf_side) is a depth plane, optionally a colour plane (ptr NULL: none), K for that size, an estimate est = (camToWorld, s) and a depth range.
 *     With Rt = R^T and s = est.s, M in double: M_aj = Rt[a][j] / s, M_a3 = -(((Rt_a0 t0 + Rt_a1 t1) + Rt_a2 t2)) / s; every entry then rounded to float
 *     (nalo_tsdf_est_world_to_cam). For s == 1 this is nalo_tsdf_integrate_depth's M bit for bit: a quotient by 1.0 is exact.
 *     The per-voxel predicate is nalo_tsdf_integrate_depth's, word for word, up to sdf (one device function serves both kernels). Then sdf = (D - zc) * (float)s;
 *     the voxel is skipped when sdf < -trunc; d = fminf(1.0f, sdf / trunc). For s == 1 the product is exact: an add at s == 1 IS nalo_tsdf_integrate_depth
 *     (nalo_tsdf_integrate_depth_color with a colour plane), bit for bit, nalo_tsdf_last included.
 *   Add, at a voxel the side's predicate accepts: as the integration. tsdf = (t0 * w0 + d) / (w0 + 1.0f); weight = fminf(w0 + 1.0f, max_weight); with a colour plane
 *     X = (X0 * w0 + (float)x) / (w0 + 1.0f) for the three planes.
 *   Remove, at a voxel the side's predicate accepts, with w1 = w0 - 1.0f: if !(w1 > 0.0f) - w0 <= 1, a NaN weight, a voxel never seen - tsdf = 1.0f, weight = 0.0f
 *     and, on a side with a colour plane, the three colour words 0.0f: the initial values ("reset"). Else tsdf = (t0 * w0 - d) / w1; weight = w1; colour
 *     X = (X0 * w0 - (float)x) / w1.
 *     What this is: the exact algebraic inverse of the add while the voxel's weight never reached max_weight; in floats an inverse up to rounding (three
 *     roundings: |error| <= 3 * 2^-24 * (|t0| w0 + |d|) / w1 to first order), and exact again when the last contribution goes (the reset). What it is not: on
 *     a voxel whose weight sat at max_weight the running mean has forgotten how many planes it holds, and the removal is a defined approximation. A caller who
 *     wants faithful removal gives max_weight room. Nor is it tied to the voxels the add touched: it is the side's predicate evaluated on the grid AS IT IS
 *     NOW. Behind a nalo_tsdf_shift the origin is origin0 + (float)base * voxel_size, rounded anew, so a voxel's centre can differ in its last bit from the one
 *     the frame was fused with, and at the rim of the frustum or of the truncation band the predicate can come out the other way: a voxel removed that was
 *     not added, or one left with its contribution. The operation stays defined (it is what the model computes on the shifted geometry); it is exact bookkeeping
 *     only between shifts.
 *   Replace: remove on side `remove`, then add on side `add`, per voxel, in that order - DEFINED as the two operations one after the other, computed in one
 *     launch over the hull of the two sides' culling boxes, every voxel loaded and stored at most once. Either side may be NULL: remove only is the de-integration,
 *     add only the integration at an estimate. use_box: the REMOVE side applies only to voxels of [lo, lo + size); the add side always sees the whole grid. A
 *     side with a colour plane moves colour and needs a coloured volume; a side without one leaves the colour words alone, as nalo_tsdf_integrate_depth does.
 *     No float atomic, one lane owns a voxel: the same bytes on every run.
 * nalo_tsdf_replace_depth   stream order as nalo_tsdf_integrate_depth: the main stream waits on the device for producer_stream, an event is recorded behind the
 *     kernel, nalo_tsdf_release applies; with the volume allocated the call makes no host wait. Afterwards nalo_tsdf_last reports the hull box, visited = its voxel
 *     count and updated = the voxels written. Refusals queue nothing and leave volume, colour and nalo_tsdf_last as they were: NALO_ERR_ARG for both sides NULL,
 *     anything nalo_tsdf_integrate_depth[_color] refuses about a plane, K, range or pose, an s that is not finite or <= 0, a box that is empty or leaves the grid;
 *     NALO_ERR_STATE for a colour plane on an uncoloured volume (and without a volume).
 * nalo_tsdf_replace_last    waits once: the hull box, visited, and the voxels removed, reset (removed and back at the initial values), added and written (either).
 *     Integer sums: a wave reduction, then one atomic instruction per workgroup. NALO_ERR_STATE when the last operation on the volume was not a replacement.
 * The fusion log: so that a fused frame can be replaced with its frame_id and the new estimate alone. The plane of a fused frame is rebuilt from the dense
 *     archive (nalo_tsdf_integrate_frame's plane), so nothing per frame is kept on the device; an entry (nalo_tsdf_log_entry) is host memory: frame_id, n_records
 *     (the length of the frame's dense list that was fused), the estimate, K and range it was fused with, whether that fusion moved colour, and the RESIDENT BOX [lo, lo + size): the voxels that
 *     have held this frame's contribution without a break since it was fused. The log belongs to the context and is OFF by default; while it is off nothing in
 *     the library behaves differently. nalo_tsdf_log_enable(ctx, on) and nalo_tsdf_log_get(ctx, out, cap, n) are host only and launch nothing (n: the entries
 *     there are; min(n, cap) are copied, in the order the frames were first fused; out may be NULL with cap 0). With the log on:
 *       nalo_tsdf_integrate_frame of a frame without an entry adds one (s = 1, box = the whole grid), the volume's bytes exactly as without the log; of a
 *       frame that has an entry it returns NALO_ERR_STATE (use the replacement) and does nothing.
 *       A non-zero nalo_tsdf_shift, the one inside nalo_tsdf_follow too, maps every entry's box through nalo_tsdf_box_shift and drops the entries whose box is
 *       empty: the voxels a shift brings in are fresh, and a later removal must not touch what other frames fused into them.
 *       nalo_tsdf_reset, nalo_tsdf_create, nalo_tsdf_destroy and nalo_tsdf_log_enable(ctx, 0) clear the log. nalo_tsdf_set, nalo_tsdf_color_set,
 *       nalo_tsdf_integrate_depth[_color], nalo_tsdf_replace_depth and nalo_ba_snapshot / nalo_ba_restore do not touch it: what a caller writes into the volume
 *       by those is the caller's to keep track of.
 * nalo_tsdf_replace_frame   DEFINED as nalo_tsdf_replace_depth with
 *       remove = the entry's estimate, K and range on the last-record plane of the FIRST n_records records of the frame's dense list, restricted to the entry's
 *                box; absent when the frame has no entry;
 *       add    = est_new (NULL: absent), K and range of this call on the last-record plane of the WHOLE list as it is now;
 *     colour from the records: on the add side iff the volume holds colour now, on the remove side iff the frame's fusion moved colour (the entry's `coloured`: the
 *     volume held colour when the frame was last fused; nalo_tsdf_color_disable clears it in every entry) - a frame fused before nalo_tsdf_color_enable is taken
 *     out of tsdf and weight only, its colour words, which never held it, are left alone. The one context-owned plane serves both sides when the list has not grown since the frame was
 *     fused, a second context-owned plane is built when it has. With est_new the entry becomes {est_new, the current length, K, range, the whole grid} (a frame
 *     without an entry gets it); with NULL the entry is dropped. nalo_tsdf_last / nalo_tsdf_replace_last as after nalo_tsdf_replace_depth. Enqueues only.
 *     NALO_ERR_STATE: no volume, the log off, no dense archive, a sharded window, a list shorter than n_records (the dense archive was reset). NALO_ERR_ARG: a
 *     frame_id the dense archive has never seen, NULL with no entry, a K, estimate or range nalo_tsdf_replace_depth refuses. A refusal queues nothing and leaves
 *     volume, colour, log and nalo_tsdf_last as they were.
 *
 * The window replacement. nalo_ba_optimize moves every keyframe of the window at once and nalo_ba_plane_scale_fix rescales all of them; looping the single
 * replacement sweeps nearly the same voxels once per frame. An ordered list of n pairs, 1 <= n <= 16 (the largest window the library accepts), each a
 * nalo_tsdf_replace_args: a remove side or NULL, an add side or NULL, its own use_box / lo / size, its own producer_stream.
 *   DEFINED: the result is the volume after nalo_tsdf_replace_depth(pair[0]), nalo_tsdf_replace_depth(pair[1]), ... nalo_tsdf_replace_depth(pair[n-1]) in that
 *     order, bit for bit in tsdf, weight and the colour words. A replacement's arithmetic at a voxel reads only that voxel's own tsdf, weight and colour words,
 *     so the chain is computed per voxel in registers: ONE launch over the hull of all sides' culling boxes (each side's box computed exactly as for the single
 *     call, the remove sides cut by their pair's box), every voxel loaded at most once and stored at most once; rows of the hull in no side's box are left before
 *     any voxel is loaded. The order is part of the definition: pair k's removal sees what pair k - 1's add left - a weight that sat at max_weight, a voxel one
 *     pair reset and a later one adds into. The colour words go through the chain side by side. No float atomic, one lane owns a voxel: the same bytes on every
 *     run. n = 1 IS nalo_tsdf_replace_depth, nalo_tsdf_last and nalo_tsdf_replace_last included.
 * nalo_tsdf_replace_depth_n   stream order as nalo_tsdf_replace_depth: the main stream waits on the device for every distinct producer_stream of the list, one
 *     event is recorded behind the kernel, nalo_tsdf_release applies; with the volume allocated the call makes no host wait (the sides travel through one of four
 *     pinned staging slots, each guarded by an event: only a fifth call queued behind four that have not started waits, for the first one's copy). Every pair is
 *     checked before anything is queued. Refusals queue nothing and leave volume, colour, log and nalo_tsdf_last as they were: NALO_ERR_ARG for n outside
 *     1..16, a NULL list, a pair with both sides NULL; for a pair nalo_tsdf_replace_depth would refuse, that call's code, with "pair k" in the message.
 *     Afterwards nalo_tsdf_last reports the hull, visited = its voxel count, updated = written_total: the voxels where ANY pair fired, each counted once.
 *     nalo_tsdf_replace_last reports the hull, written = written_total, and removed / reset / added summed over the pairs.
 * nalo_tsdf_replace_last_n    waits once: `total` (may be NULL) as nalo_tsdf_replace_last, and per pair removed, reset, added and written (the voxels where
 *     that pair fired at all): min(n, cap) rows are copied, *n is the number there are. Exact integers: wave ballots and population counts, summed per workgroup
 *     in LDS, one atomic instruction per counter per workgroup. NALO_ERR_STATE when the last operation on the volume was not a window replacement.
 * nalo_tsdf_replace_frames    DEFINED as nalo_tsdf_replace_frame(frame_id[k], has_est[k] ? &est_new[k] : NULL, K, min_depth, max_depth) for k = 0 .. n - 1 in
 *     order: the volume and the log afterwards are those of that loop, bit for bit, and nalo_tsdf_log_get's order (first fusion) with them. The work is the
 *     plane builds, one after the other on the context's stream into a pool of planes the volume owns (one per frame, two when its list has grown; it grows on
 *     demand and goes with the volume), and the ONE launch above; each entry's resident box cuts its pair's remove side. All or nothing: every refusal of
 *     nalo_tsdf_replace_frame, for any k, refuses the whole call ("frame k" in the message), and a frame_id that appears twice is NALO_ERR_ARG (the loop would
 *     allow it; one transaction on the log does not need to). A refused call leaves log, volume, colour and nalo_tsdf_last unchanged; an accepted one updates
 *     the log for all pairs. skip_unchanged != 0: a frame that has an entry, whose est_new, K and range equal the entry's bit for bit and whose dense list is as
 *     long as n_records, is no pair; its entry stays as it is and it is counted in n_skipped. A call whose frames are all skipped launches nothing, returns
 *     NALO_OK and leaves nalo_tsdf_last as it was. nalo_tsdf_replace_frame, nalo_tsdf_integrate_frame and nalo_tsdf_align_frame keep their planes.
 * nalo_tsdf_replace_frames_plan   host only, no context: the list's own checks and skip_unchanged's predicate on a log given as an array. list_len[k]: the
 *     length of frame k's dense list now (NULL: nothing is skipped). skip[k] = 1 for a skipped frame, written for every k < n on NALO_OK. NALO_ERR_ARG: NULL
 *     args or skip, n outside 1..16, a NULL frame_id list, a frame_id twice, and - for a frame that has an estimate - a pose that is not finite, an s that is
 *     not finite or <= 0, a K that is not finite, a range that is not finite or has min_depth > max_depth.
 * nalo_tsdf_est_world_to_cam   host only, no context: the M above. NALO_ERR_ARG for a non-finite pose or an s that is not finite or <= 0.
 * nalo_tsdf_frustum_box_est    host only, no context: nalo_tsdf_frustum_box with z = max_depth + trunc / s in double and each far corner at
 *     (((c0 X + c1 Y) + c2 z) * s) + c3. For s == 1 it is nalo_tsdf_frustum_box's box exactly (one function computes both). It is conservative for every voxel
 *     either operation touches: such a voxel has 0 < zc <= max_depth + trunc / s in the estimate's camera, which maps to the world by p -> s R p + t.
 * nalo_tsdf_box_shift   host only, no context: the box [lo, lo + size) of a volume translated by -shift - where its voxels lie after nalo_tsdf_shift(shift) - and
 *     clipped to the grid, in place; all zeros when nothing of it is left (or a size was < 1). 64-bit arithmetic on any int. NALO_ERR_ARG: a dimension outside [1, 2048].
 * ------------------------------------------------------------------------------------------------ */
typedef struct nalo_tsdf_desc { float origin[3]; float voxel_size; int dims[3]; float trunc; float max_weight; } nalo_tsdf_desc;
typedef struct nalo_tsdf_integrate_args {
    nalo_dev_plane depth;                   /* F32, one channel, w x h of its own */
    float K[4];                             /* fx, fy, cx, cy for that size */
    double camToWorld[12];
    float min_depth, max_depth;
    void* producer_stream;                  /* hipStream_t whose queued work produces the plane; NULL = the null stream */
} nalo_tsdf_integrate_args;
typedef struct nalo_tsdf_stats { int lo[3], hi[3]; long long visited, updated; } nalo_tsdf_stats;
typedef struct nalo_tsdf_volume_view { float* tsdf; float* weight; int dims[3]; void* stream; } nalo_tsdf_volume_view;
typedef struct nalo_tsdf_surface_args {
    int use_box; int lo[3], size[3];        /* use_box == 0: the whole grid */
    float min_weight;
    long long cap; float* xyz;              /* host, [cap][3] */
    long long n, n_needed;                  /* out: points written; crossings found */
} nalo_tsdf_surface_args;
int nalo_tsdf_create(nalo_ctx* ctx, const nalo_tsdf_desc* desc);
int nalo_tsdf_reset(nalo_ctx* ctx);
int nalo_tsdf_destroy(nalo_ctx* ctx);
int nalo_tsdf_integrate_depth(nalo_ctx* ctx, const nalo_tsdf_integrate_args* args);
int nalo_tsdf_release(nalo_ctx* ctx, void* stream);
int nalo_tsdf_integrate_frame(nalo_ctx* ctx, int frame_id, const double camToWorld[12], const float K[4], float min_depth, float max_depth);
int nalo_tsdf_last(nalo_ctx* ctx, nalo_tsdf_stats* stats);
int nalo_tsdf_get(nalo_ctx* ctx, const int lo[3], const int size[3], float* tsdf, float* weight);
int nalo_tsdf_set(nalo_ctx* ctx, const int lo[3], const int size[3], const float* tsdf, const float* weight);
int nalo_tsdf_view(nalo_ctx* ctx, nalo_tsdf_volume_view* out);
int nalo_tsdf_surface_points(nalo_ctx* ctx, nalo_tsdf_surface_args* args);
int nalo_tsdf_frustum_box(const nalo_tsdf_desc* desc, int w, int h, const float K[4], const double camToWorld[12], float max_depth, int lo[3], int hi[3]);   /* host only */
typedef struct nalo_tsdf_mesh_args {
    int use_box; int lo[3], size[3];        /* as nalo_tsdf_surface_args */
    float min_weight;
    long long cap_vertices, cap_triangles;
    float* xyz; int* tri;                   /* host, [cap][3] each; NULL: leave the mesh on the device */
    long long n_vertices, n_triangles;      /* out: what the device mesh holds */
} nalo_tsdf_mesh_args;
typedef struct nalo_tsdf_mesh_dev { float* xyz; int* tri; long long n_vertices, n_triangles; void* stream; } nalo_tsdf_mesh_dev;
int nalo_tsdf_mesh(nalo_ctx* ctx, nalo_tsdf_mesh_args* args);
int nalo_tsdf_mesh_view(nalo_ctx* ctx, nalo_tsdf_mesh_dev* out);     /* host only, launches nothing */
int nalo_tsdf_mesh_table(signed char out[6][16][6]);                 /* host only, no context */
typedef struct nalo_tsdf_color_volume_view { float* bgr; int dims[3]; void* stream; } nalo_tsdf_color_volume_view;   /* bgr: [3][nz][ny][nx] */
typedef struct nalo_tsdf_mesh_color_args { long long cap; uint8_t* rgba; } nalo_tsdf_mesh_color_args;               /* host, [cap][4]; NULL: leave the colours on the device */
typedef struct nalo_tsdf_mesh_color_dev { uint8_t* rgba; long long n_vertices; void* stream; } nalo_tsdf_mesh_color_dev;
int nalo_tsdf_color_enable(nalo_ctx* ctx);
int nalo_tsdf_color_disable(nalo_ctx* ctx);
int nalo_tsdf_integrate_depth_color(nalo_ctx* ctx, const nalo_tsdf_integrate_args* args, const nalo_dev_plane* colour, int colour_is_rgb);
int nalo_tsdf_color_get(nalo_ctx* ctx, const int lo[3], const int size[3], float* bgr);
int nalo_tsdf_color_set(nalo_ctx* ctx, const int lo[3], const int size[3], const float* bgr);
int nalo_tsdf_color_view(nalo_ctx* ctx, nalo_tsdf_color_volume_view* out);   /* host only, launches nothing */
int nalo_tsdf_mesh_color(nalo_ctx* ctx, nalo_tsdf_mesh_args* args, nalo_tsdf_mesh_color_args* colour);
int nalo_tsdf_mesh_color_view(nalo_ctx* ctx, nalo_tsdf_mesh_color_dev* out); /* host only, launches nothing */
typedef struct nalo_tsdf_raycast_args {
    int w, h; float K[4];                   /* fx, fy, cx, cy of the view: any size, not the context's */
    double camToWorld[12];
    float min_depth, max_depth, step;       /* camera-z of the first sample, the last allowed one, the spacing */
    float min_weight;
    int with_normals, with_colour;
    float* depth; float* normal; uint8_t* rgba;   /* host, optional: [h][w], [h][w][3], [h][w][4]; NULL = leave on the device */
    long long n_hit, n_back, n_normal;      /* out */
    int n_steps;                            /* out: N */
} nalo_tsdf_raycast_args;
typedef struct nalo_tsdf_raycast_dev { nalo_dev_plane depth, normal, rgba; int w, h; void* stream; } nalo_tsdf_raycast_dev;
int nalo_tsdf_raycast(nalo_ctx* ctx, nalo_tsdf_raycast_args* args);
int nalo_tsdf_raycast_view(nalo_ctx* ctx, nalo_tsdf_raycast_dev* out);       /* host only, launches nothing */
int nalo_tsdf_raycast_steps(float min_depth, float max_depth, float step, int* n_steps);   /* host only, no context */
/* the two structs share their call's name, so they are named by their tags: `struct nalo_tsdf_geometry g;` (a typedef would collide with the function in C) */
struct nalo_tsdf_geometry { nalo_tsdf_desc desc; float origin0[3]; int base[3]; };                 /* desc.origin: the current origin */
struct nalo_tsdf_shift_boxes { int n_boxes; int lo[3][3], size[3][3]; int kept_lo[3], kept_size[3]; };   /* lo[b], size[b]: box b < n_boxes, voxel indices */
int nalo_tsdf_shift(nalo_ctx* ctx, const int shift[3]);
int nalo_tsdf_geometry(nalo_ctx* ctx, struct nalo_tsdf_geometry* out);       /* host only, launches nothing */
int nalo_tsdf_shift_for(const nalo_tsdf_desc* now, const double centre[3], const int margin[3], int shift[3]);   /* host only, no context */
int nalo_tsdf_shift_boxes(const int dims[3], const int shift[3], struct nalo_tsdf_shift_boxes* out);            /* host only, no context */
struct nalo_tsdf_archive_stats {                                             /* named by its tag, as nalo_tsdf_geometry */
    long long added_vertices, welded_vertices, added_triangles;             /* the last nalo_tsdf_archive_mesh */
    long long n_vertices, n_triangles;                                      /* the archive */
    long long cap_vertices, cap_triangles, table_slots;
    int coloured, have_lattice; float origin0[3], voxel_size;
};
typedef struct nalo_tsdf_archive_get_args {
    long long cap_vertices, cap_triangles, cap_rgba, cap_key;               /* rows each array has room for */
    float* xyz; int* tri; uint8_t* rgba; int* key;                          /* host, [cap][3], [cap][3], [cap][4], [cap][4]; NULL: not asked for */
    long long n_vertices, n_triangles;                                      /* out */
} nalo_tsdf_archive_get_args;
typedef struct nalo_tsdf_archive_dev { float* xyz; int* tri; uint8_t* rgba; int* key; long long n_vertices, n_triangles; void* stream; } nalo_tsdf_archive_dev;
typedef struct nalo_tsdf_follow_stats { int n_boxes; long long added_vertices, welded_vertices, added_triangles, n_vertices, n_triangles; } nalo_tsdf_follow_stats;
int nalo_tsdf_archive_enable(nalo_ctx* ctx);
int nalo_tsdf_archive_disable(nalo_ctx* ctx);
int nalo_tsdf_archive_reset(nalo_ctx* ctx);
int nalo_tsdf_archive_mesh(nalo_ctx* ctx, nalo_tsdf_mesh_args* m, struct nalo_tsdf_archive_stats* out);
int nalo_tsdf_archive_stats(nalo_ctx* ctx, struct nalo_tsdf_archive_stats* out);   /* host only, launches nothing */
int nalo_tsdf_archive_get(nalo_ctx* ctx, nalo_tsdf_archive_get_args* args);
int nalo_tsdf_archive_view(nalo_ctx* ctx, nalo_tsdf_archive_dev* out);             /* host only, launches nothing */
int nalo_tsdf_follow(nalo_ctx* ctx, const double centre[3], const int margin[3], float min_weight, int shift_out[3], nalo_tsdf_follow_stats* stats);
typedef struct nalo_tsdf_align_est { double camToWorld[12]; double s; } nalo_tsdf_align_est;
typedef struct nalo_tsdf_align_args {
    nalo_dev_plane depth;                   /* F32, one channel, w x h of its own (nalo_tsdf_align_frame: not looked at) */
    float K[4];                             /* fx, fy, cx, cy for that size */
    float min_depth, max_depth, min_weight, huber;
    int step, dof;                          /* every step-th pixel both ways; 6 or 7 */
    void* producer_stream;                  /* as nalo_tsdf_integrate_args */
    float* records; long long records_cap;  /* DEVICE, optional: [h][w][10]; the floats there is room for */
    int max_iterations, min_used;           /* the loop only: 1..64; the fewest used pixels an estimate may have */
    double lambda0, eps;                    /* the loop only: 0 = 0.01; the norm of the increment that ends it */
} nalo_tsdf_align_args;
typedef struct nalo_tsdf_align_sums { double H[28], b[7], E, rr; long long count[4]; } nalo_tsdf_align_sums;   /* count[state]; count[0] = n */
typedef struct nalo_tsdf_align_trace { nalo_tsdf_align_est est; double lambda, E; long long count[4]; int accepted; } nalo_tsdf_align_trace;
enum { NALO_TSDF_ALIGN_CONVERGED = 0, NALO_TSDF_ALIGN_ITERATION_LIMIT = 1, NALO_TSDF_ALIGN_TOO_FEW = 2, NALO_TSDF_ALIGN_SOLVE_FAILED = 3 };
typedef struct nalo_tsdf_align_result {
    nalo_tsdf_align_est est;
    int status, iterations, evaluations;
    double E_first, E_last; long long n_first, n_last;
    nalo_tsdf_align_sums last;              /* the sums at est */
    nalo_tsdf_align_trace* trace; int trace_cap;   /* in: host, optional */
    int n_trace;
} nalo_tsdf_align_result;
int nalo_tsdf_align_eval(nalo_ctx* ctx, const nalo_tsdf_align_args* args, const nalo_tsdf_align_est* est, nalo_tsdf_align_sums* out);
int nalo_tsdf_align_depth(nalo_ctx* ctx, const nalo_tsdf_align_args* args, const nalo_tsdf_align_est* est_in, nalo_tsdf_align_result* result);
int nalo_tsdf_align_frame(nalo_ctx* ctx, int frame_id, const nalo_tsdf_align_args* args, const nalo_tsdf_align_est* est_in, nalo_tsdf_align_result* result);
int nalo_tsdf_align_step(const double H[28], const double b[7], double lambda, int dof, const nalo_tsdf_align_est* est, double inc[7], nalo_tsdf_align_est* est_out);   /* host only, no context */
typedef struct nalo_tsdf_side {
    nalo_dev_plane depth;                   /* F32, one channel, w x h of its own */
    nalo_dev_plane colour;                  /* ptr NULL: none; else U8, three channels, the depth plane's size */
    int colour_is_rgb;                      /* channel 0 is R (else B) */
    float K[4];                             /* fx, fy, cx, cy for that size */
    nalo_tsdf_align_est est;                /* camToWorld and the scale s > 0 */
    float min_depth, max_depth;
} nalo_tsdf_side;
typedef struct nalo_tsdf_replace_args {
    const nalo_tsdf_side* remove;           /* NULL: add only */
    const nalo_tsdf_side* add;              /* NULL: remove only */
    int use_box; int lo[3], size[3];        /* use_box != 0: the remove side applies to these voxels only */
    void* producer_stream;                  /* as nalo_tsdf_integrate_args, for the planes of both sides */
} nalo_tsdf_replace_args;
typedef struct nalo_tsdf_replace_stats { int lo[3], hi[3]; long long visited, removed, reset, added, written; } nalo_tsdf_replace_stats;
int nalo_tsdf_replace_depth(nalo_ctx* ctx, const nalo_tsdf_replace_args* args);
int nalo_tsdf_replace_last(nalo_ctx* ctx, nalo_tsdf_replace_stats* stats);
typedef struct nalo_tsdf_log_entry {
    int frame_id, n_records;                /* n_records: the length of the frame's dense list that was fused */
    nalo_tsdf_align_est est; float K[4]; float min_depth, max_depth;   /* what it was fused with */
    int lo[3], size[3];                     /* the resident box */
    int coloured;                           /* the fusion moved colour: a removal takes the frame out of the colour words too */
} nalo_tsdf_log_entry;
int nalo_tsdf_log_enable(nalo_ctx* ctx, int on);                                       /* host only, launches nothing */
int nalo_tsdf_log_get(nalo_ctx* ctx, nalo_tsdf_log_entry* out, int cap, int* n);       /* host only, launches nothing */
int nalo_tsdf_replace_frame(nalo_ctx* ctx, int frame_id, const nalo_tsdf_align_est* est_new /* NULL: remove only */, const float K[4], float min_depth, float max_depth);
typedef struct nalo_tsdf_replace_pair_stats { long long removed, reset, added, written; } nalo_tsdf_replace_pair_stats;
int nalo_tsdf_replace_depth_n(nalo_ctx* ctx, const nalo_tsdf_replace_args* pairs, int n);       /* 1 <= n <= 16 */
int nalo_tsdf_replace_last_n(nalo_ctx* ctx, nalo_tsdf_replace_stats* total /* may be NULL */, nalo_tsdf_replace_pair_stats* per_pair, int cap, int* n);
typedef struct nalo_tsdf_replace_frames_args {
    int n; const int* frame_id;             /* 1 <= n <= 16, no frame_id twice */
    const nalo_tsdf_align_est* est_new;     /* [n]; NULL: remove only, for every frame */
    const unsigned char* has_est;           /* optional [n]: 0 = this frame is removed only; NULL = all have one */
    float K[4]; float min_depth, max_depth;
    int skip_unchanged;
    int n_skipped;                          /* out */
} nalo_tsdf_replace_frames_args;
int nalo_tsdf_replace_frames(nalo_ctx* ctx, nalo_tsdf_replace_frames_args* args);
int nalo_tsdf_replace_frames_plan(const nalo_tsdf_replace_frames_args* args, const nalo_tsdf_log_entry* log, int n_log, const int* list_len, unsigned char* skip);   /* host only, no context */
int nalo_tsdf_est_world_to_cam(const nalo_tsdf_align_est* est, float M[12]);   /* host only, no context */
int nalo_tsdf_frustum_box_est(const nalo_tsdf_desc* desc, int w, int h, const float K[4], const nalo_tsdf_align_est* est, float max_depth, int lo[3], int hi[3]);   /* host only, no context */
int nalo_tsdf_box_shift(const int dims[3], const int shift[3], int lo[3], int size[3]);   /* host only, no context */

/* ------------------------------------------------------------------------------------------------
 * Profiling: per-kernel HIP-event timing on the ctx stream. Names: "trk_eval", "ba_linearize",
 * "ba_sc", "ba_reduce", "ba_resub", "pyramid", "trk_lm", "imm_trace", "imm_optimize", "pixsel", "dist_bfs", "dense_bbox", "dense_map", "dense_extent", "dense_boxes", "dense_update_map", "map_dense_world_points", "map_dense_cloud", "ingest", "tsdf_integrate", "tsdf_replace", "tsdf_replace_n", "tsdf_surface", "tsdf_mesh", "tsdf_raycast", "tsdf_align", "tsdf_shift", "tsdf_archive" (the key pass and the append of nalo_tsdf_archive_mesh, not its mesh), "map_render_tris" (the triangle pass of nalo_map_render_mesh). Enable, run, then query (sync inside).
 * nalo_profile_select(ctx, name) restricts the brackets to ONE scope (NULL = all): a recorded event pair costs ~10 us of pipeline bubbles on a
 * latency-bound window, so a timed run brackets only the kernel it reports ("ba_linearize" carries its timestamps in the dispatch itself).
 * ------------------------------------------------------------------------------------------------ */
int nalo_profile_enable(nalo_ctx* ctx, int on);
int nalo_profile_select(nalo_ctx* ctx, const char* kernel);
int nalo_profile_reset(nalo_ctx* ctx);
/* bracket only one launch in `every` of the selected scopes (default 1 = all). The event pairs cost a few microseconds of pipeline each: on the KITTI-sized
 * window 8 bracketed launches per keyframe are 4-6 % of a step; a sampled average (every = 3: co-prime with the 8 launches of a keyframe) measures the same kernel
 * with a third of the perturbation. nalo_profile_get reports the bracketed launches only. */
int nalo_profile_sample(nalo_ctx* ctx, int every);
int nalo_profile_get(nalo_ctx* ctx, const char* kernel, double* total_ms, int* launches);
/* every bracketed launch of a scope since the last nalo_profile_reset, in launch order (milliseconds; at most cap values are copied, *n = how many exist):
 * the spread and the position inside a keyframe that the mean of nalo_profile_get hides */
int nalo_profile_samples(nalo_ctx* ctx, const char* kernel, float* ms, int cap, int* n);

/* Calibration of the roofline's denominator on THIS device ("fraction of the box's measured device-copy / triad bandwidth from a calibration
 * kernel in the same run"; no reference counterpart). Runs `iters` timed passes (after one untimed) of a streaming kernel over `bytes`-sized buffers on the
 * context's stream, timed with HIP events: copy_GBs = 2 * bytes / t (b[i] = a[i], 16 B per lane, grid-stride), triad_GBs = 3 * bytes / t (c[i] = a[i] + s * b[i]).
 * bytes is rounded down to a multiple of 16; >= 1 MiB. Either output may be NULL. */
int nalo_hbm_calibrate(nalo_ctx* ctx, size_t bytes, int iters, double* copy_GBs, double* triad_GBs);

#ifdef __cplusplus
}
#endif
#endif
