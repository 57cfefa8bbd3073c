// Internal state of a nalo_ctx: HBM-resident frame pyramids, tracker point clouds, BA window arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include <chrono>

#include "../../include/nalo_gpu.h"
#include "host_math.h"
#include "ref_constants.h"
#include "tsdf_device.h"
#include "map_render_tri.h"

namespace nalo {

// The owners below wrap the HIP allocation calls and nothing else: each frees what it holds in its destructor and is move-only, so a struct
// that holds one releases it without a list anywhere. Kernel-argument structs take raw views (.p / .dev).
template <typename T>
struct DevBuf {                  // device buffer, grows on demand (contents are not kept), freed with its holder
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// A painter's per-pixel key plane: a DevBuf whose every byte is FillByte while no call is in flight. The scatter passes move keys with integer atomics and the
// resolve pass puts back what it found moved (plot_take_keys, plot_device.h), so a call pays for a fill only when the plane is new or has grown, or when the
// call before it failed between begin() and settled(). What lives beside the plane and is kept idle the same way (a painter's counters) follows `refilled`.
template <typename T, int FillByte>
struct KeyPlane : private DevBuf<T> {
    using DevBuf<T>::p;
    // room for `words` keys; the fill, when one is due, covers the whole capacity and is queued on s in front of the caller's scatter
    hipError_t begin(size_t words, hipStream_t s, bool* refilled = nullptr) {
        const bool refill = words > this->cap || !idle;
        if (refilled) *refilled = refill;
        idle = false;
        hipError_t e = this->reserve(words);
        if (e == hipSuccess && refill) e = hipMemsetAsync(p, FillByte, this->cap * sizeof(T), s);
        return e;
    }
    void settled() { idle = true; }                                             // the resolve pass that restores every key has been queued
private:
    bool idle = false;
};

// pixels per workgroup of a resolve pass (256 lanes x 4 pixels): key planes and the images resolved from them are sized in whole workgroups
constexpr int kResolvePix = 1024;
inline size_t resolve_padded_pixels(size_t pixels) { return (pixels + kResolvePix - 1) / kResolvePix * kResolvePix; }

template <typename T>
struct HostBuf {                 // pinned host block with DevBuf's grow rule; cap is the allocation, in elements
    T* p = nullptr;
    T* dev = nullptr;            // the device alias of a hipHostMallocMapped block, fetched once per allocation
    size_t cap = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    HostBuf(HostBuf&& o) noexcept : p(o.p), dev(o.dev), cap(o.cap) { o.p = o.dev = nullptr; o.cap = 0; }
    HostBuf& operator=(HostBuf&& o) noexcept { std::swap(p, o.p); std::swap(dev, o.dev); std::swap(cap, o.cap); return *this; }
    ~HostBuf() { release(); }
    hipError_t reserve(size_t n, unsigned flags = 0) {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), flags);
        if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer((void**)&dev, p, 0);
        if (e == hipSuccess) cap = n; else release();
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = dev = nullptr; cap = 0; }   // hipHostFree waits for copies in flight
};

struct Event {                   // one hipEvent_t, created on first use with the flags its site asks for; passes as the raw handle
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = 0) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

struct Stream {                  // one non-blocking hipStream_t; passes as the raw handle. A nalo_ctx is never copied or moved, so neither is this
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

struct FrameSlot {
    DevBuf<float> I[NALO_MAX_LEVELS];        // planar irradiance per level
    DevBuf<float4> dI[NALO_MAX_LEVELS];      // {I, dx, dy, 0} per level: one 16-B load per bilinear tap
    DevBuf<float> absg[NALO_MAX_LEVELS];     // absSquaredGrad
    DevBuf<float> mask;                      // level 0 (densemap only)
    DevBuf<uint8_t> bgr;
    bool valid = false;
    Event ev_up;                             // nalo_frame_upload_async: the slot's H2D copies (copy stream) have completed; nalo_frame_ingest_device: its last kernel that reads a caller's plane has
    DevBuf<uint8_t> raw;                     // nalo_frame_upload_raw_async: this slot's sensor frame as uploaded (several frames may be in flight)
    DevBuf<float> dI0t; bool tiled_valid = false;    // level 0 again as 12-byte texels in 5x2 tiles of 128 bytes (ba_linearize's gathers), made on demand (frame_tile_level0)
};

struct ProfEntry { double ms = 0; int n = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; std::vector<float> samples; };   // samples: every bracketed launch, in launch order (nalo_profile_samples)

// precalc record per (host,target), 32 floats: KRKi(9) Kt(3) R0(9) t0(3) aff(2) b0 thmax dp(8)... see kernels_ba.hip
struct BAWindow;
struct PixSel;
struct Initializer;
struct MapArchive;
struct DenseArchive;
struct TsdfVolume;
struct TsdfArchive;

}  // namespace nalo

struct nalo_ctx {
    int device = 0;
    int w = 0, h = 0, levels = 0;
    int wl[NALO_MAX_LEVELS], hl[NALO_MAX_LEVELS];
    float fx[NALO_MAX_LEVELS], fy[NALO_MAX_LEVELS], cx[NALO_MAX_LEVELS], cy[NALO_MAX_LEVELS];   // tracker pyramid intrinsics
    float K0[4];
    // Members are destroyed in reverse order of declaration: the streams stand before every buffer and event of the context, so they outlive all of them
    // (nalo_destroy has drained them, and deleted ba / pixsel / init, before the context goes).
    nalo::Stream stream, side, copy;         // copy: H2D frame uploads of nalo_frame_upload_async (overlap the kernels of `stream`), created on first use
    nalo::Event ev_main;                     // main-stream marker the copy stream waits on before it overwrites a slot that has been used
    nalo::Event ev_prod;                     // nalo_frame_ingest_device, nalo_trk_ref_import: recorded on the caller's producer stream, the main stream waits for it
    nalo::DevBuf<float> gamma_dev;           // 256-entry gamma table of the asynchronous upload path
    float gamma_last[256]; bool gamma_have = false;   // what gamma_dev holds: the table is re-sent only when the caller's differs (and then behind every kernel that may read it)
    // raw-frame ingest (nalo_undist_set / nalo_frame_upload_raw): photometric + geometric undistortion tables, raw staging
    int und_wOrg = 0, und_hOrg = 0, und_photometric = 0, und_GDepth = 0; bool und_set = false, und_remap = false, und_vig = false;
    nalo::DevBuf<float> und_G, und_vinv, und_rxy; nalo::DevBuf<uint8_t> und_raw, und_mask, und_bgr;   // und_rxy: the remap table interleaved {x, y} (one 8-byte load per pixel in the ingest pass)
    std::string err;
    std::vector<nalo::FrameSlot> slots;

    // ---- tracker
    int slot_ref = -1;
    nalo::DevBuf<float> trk_idepth[NALO_MAX_LEVELS], trk_wsum[NALO_MAX_LEVELS], trk_wbak[NALO_MAX_LEVELS];
    nalo::DevBuf<float> pc_u[NALO_MAX_LEVELS], pc_v[NALO_MAX_LEVELS], pc_id[NALO_MAX_LEVELS], pc_col[NALO_MAX_LEVELS];
    int pc_n[NALO_MAX_LEVELS] = {};
    nalo::Event ev_imp;                      // nalo_trk_ref_import: recorded behind the copy kernel, i.e. the caller's arrays have been read (nalo_trk_ref_release)
    nalo::DevBuf<float> trk_partial;         // [blocks][64]
    nalo::DevBuf<unsigned> trk_ticket;       // trk_eval_kernel's arrival counter (zero between launches)
    nalo::DevBuf<float> ref_res; int ref_res_n = -1;   // nalo_trk_ref_upload: {Ku, Kv, new_idepth, HdiF} of the tracking reference, resident (n = -1: none)
    nalo::DevBuf<double> trk_out;            // 64 doubles
    nalo::HostBuf<double> trk_out_host;      // pinned, host-mapped: results + sequence flag
    unsigned long long trk_seq = 0;
    nalo::DevBuf<unsigned long long> lm_partial;   // persistent LM kernel: [2][blocks][64] block partials {fp32, tag}
    unsigned long long lm_launches = 0;
    nalo::HostBuf<double> lm_tries_host;     // nalo_trk_track_tries, host-mapped: summary (32, seq at [31]) | NALO_TRK_MAX_TRIES records | the list of tries
    int lm_evals_lvl[5] = {};                // LM evaluations per pyramid level of the last nalo_trk_track (nalo_trk_last_evals)
    int trk_cfg[9] = {};                     // launch of the last nalo_trk_track (nalo_trk_get_launch_config)
    int trk_rank = 0, trk_world = 1; nalo_allreduce_fn trk_hook = nullptr; void* trk_hook_user = nullptr; bool trk_hook_stream_ordered = false;   // nalo_trk_set_shard
    nalo::DevBuf<double> trk_shard_sums;     // a sharded evaluation's 52 sums on the device, summed over the ranks in place by the hook
    bool lm_host_only = false;                 // latched when a trk_lm launch lost a workgroup (CUs taken by another context): the host-driven LM loop from then on
    nalo::DevBuf<int> scan_tmp;              // compaction counts
    nalo::DevBuf<unsigned long long> dense_lb;   // nalo_dense_make_map scratch: row table | chunk aggregates | last[2] | ticket
    // nalo_dense_update_map (kernels_dense.hip): the per-cluster tables, the chunk aggregates and counts, the call's point scratch (one record per candidate of the
    // scanned range, sized once) and the pinned block the boxes and results come up and the batch table goes down through
    nalo::DevBuf<uint4> dn_tab, dn_blk, dn_pts; nalo::HostBuf<int> dn_host;
    nalo::DevBuf<int> trk_cnt;               // hits per level-0 pixel of the reference scatter (ordered redo of pixels with >= 3 hits)
    nalo::DevBuf<unsigned long long> trk_seed_ticket;   // nalo_trk_set_ref_from_depth: {arrived workgroups << 32 | passing pixels} of the seed kernel (zero between launches)
    nalo::DevBuf<float> upload_tmp;
    nalo::HostBuf<float> pinned_f;           // nalo_trk_set_ref's staging (upload4)
    // nalo_trk_depth_image (kernels_depth_image.hip), sized on first use: the select's histograms, state and results; the painted image; the pinned block it comes up through
    nalo::DevBuf<unsigned> di_scr; nalo::DevBuf<uint8_t> di_bgr; nalo::HostBuf<uint8_t> di_host;
    nalo::HostBuf<float> imm_host; nalo::DevBuf<float> imm_dev;   // immature-point staging (pinned / device), grown together (imm_stage)
    nalo::DevBuf<float> imm_res; int imm_res_n = 0, imm_res_maxhost = -1;         // device-resident immature points (nalo_imm_resident_*)
    nalo::DevBuf<float> imm_type; bool imm_type_set = false; float imm_type_max = 0;   // their my_type (nalo_imm_resident_set_type; a new set invalidates it)
    nalo::DevBuf<int> imm_act; int imm_act_stats[4] = {};                         // nalo_imm_resident_activate's scratch; the last call's counts (nalo_imm_activate_last)
    // what nalo_ba_carry_window(insert_activated) needs of the resident set and of the last activation that was asked for its optimisation outputs
    std::vector<float> imm_uv_h; std::vector<int> imm_host_h;                     // host copy of the set's u | v and host_idx (12 bytes per point, nalo_imm_resident_set)
    // nalo_imm_resident_carry: the buffers the set is gathered into (they change places with imm_res / imm_type), its scratch, and the last call's map and counts
    nalo::DevBuf<float> imm_res2, imm_type2; nalo::DevBuf<int> imm_carry_scr;
    std::vector<int> imm_carry_map; int imm_carry_stats[4 + NALO_MAX_WINDOW] = {}; bool imm_carry_have = false;
    nalo::DevBuf<int> act_pend;                                                  // the pending result on the device, out of the shared staging: sel (n) | idepth_out (n) | res_in (n x W bytes)
    std::vector<int> act_sel_h, act_result_h;                                    // its sel / result as they went to the caller
    int act_pend_n = -1, act_pend_W = 0; unsigned act_pend_epoch = 0;            // n = -1: none pending; the window's frames (BAWindow::frames_epoch) when it was made

    // ---- mask clusters and their planes (kernels_plane.hip): the call's device scratch (the member lists of the last call stay in it), rocPRIM's sort storage,
    // the pinned block the draws go down and the records come up through; plane_last_n = -1: no completed call
    nalo::DevBuf<unsigned> plane_w; nalo::DevBuf<unsigned char> plane_sort; nalo::HostBuf<int> plane_host; int plane_last_n = -1, plane_last_members = 0;
    nalo::DevBuf<unsigned> ground_bits;      // nalo_trk_fit_ground's w x h bitmap of ground pixels: zeroed when allocated, and left all zero by every call

    // ---- BA (opaque; defined in host_ba.hip)
    nalo::BAWindow* ba = nullptr;
    nalo::PixSel* pixsel = nullptr;          // pixel selector state (kernels_pixsel.hip)
    void* rccl = nullptr;                    // RCCL communicators of the sharded BA (host_rccl.hip)
    bool xchg_failed = false;                // a cross-rank sum failed (host_rccl.hip): the ranks' systems may differ, every later BA call of this context fails
    nalo::Initializer* init = nullptr;       // two-frame initialiser state (host_init.hip)
    nalo::MapArchive* map = nullptr;         // the archive of removed points and the clouds made from it (host_map.hip); NULL until nalo_map_enable
    nalo::DenseArchive* dmap = nullptr;      // the dense map: FrameHessian::mapPoints on the device (host_map.hip); NULL until nalo_map_dense_enable
    nalo::TsdfVolume* tsdf = nullptr;        // the TSDF volume and its scratch (host_tsdf.hip); NULL until nalo_tsdf_create
    nalo::TsdfArchive* tsdf_archive = nullptr;   // the welded mesh archive (nalo_tsdf_archive_*, host_tsdf.hip); NULL until nalo_tsdf_archive_enable. It outlives volumes
    // the fusion log (nalo_tsdf_log_*, host_tsdf.hip): what nalo_tsdf_replace_frame removes by, in the order the frames were first fused. Host memory only; the
    // switch outlives volumes, the entries do not. Off, no call looks at it
    bool tsdf_log_on = false;
    std::vector<nalo_tsdf_log_entry> tsdf_log;
    // the keyframe graph (nalo_map_graph_*, host_map.hip): EnergyFunctional::connectivityMap's keys, (host frame_id << 32) + target frame_id, with the count [1] of
    // marginalised residuals; the count [0] of live residuals is taken from the resident slots when the graph is read
    bool graph_on = false;
    std::map<uint64_t, int> graph_marg;
    nalo_settings set = {1, nalo::kAffineOptModeA, nalo::kAffineOptModeB, 1};   // util/settings.cpp:71,128-129,74

    // ---- host wall-clock accounting (NALO_HOST_TIMING=1, read by nalo_create, prints it at nalo_destroy)
    bool host_timing = false;
    std::map<std::string, std::pair<double, long>> host_t;

    // ---- nalo_test_inject: the matching event that takes a count to zero fails once (0 = disarmed)
    int inject_lm_lost_block = 0, inject_gated_solve = 0;

    // ---- profiling
    bool prof_on = false;
    std::string prof_only;                   // empty = every scope; else only the scope of that name is bracketed
    int prof_every = 1; unsigned prof_tick = 0;   // nalo_profile_sample: bracket one launch in prof_every (the brackets perturb a latency-bound pipeline)
    std::vector<hipEvent_t> prof_pool;       // idle events (raw handles: they move between this pool and ProfEntry::pending; nalo_destroy destroys both)
    std::map<std::string, nalo::ProfEntry> prof;
};

namespace nalo {

inline int fail(nalo_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; return code; }
#define NALO_HIP(ctx, expr)                                                                          \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess)                                                                       \
            return nalo::fail(ctx, NALO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// Wait for a kernel to publish `seq` into host-mapped memory (system-scope release on the device side). Spinning on the
// flag costs a few microseconds; hipStreamSynchronize costs tens. Every 2^20 spins the stream is queried for a fault and the wall clock is
// checked: after timeout_s (10 s; a launch that legitimately runs several of today's passes its multiple) without the flag the call fails with NALO_ERR_HIP (a faulted kernel or a collective
// that never completes must not stall the caller for minutes).
inline bool poll_flag(nalo_ctx* c, volatile double* flag, double seq, double timeout_s = 10.0) {
    std::chrono::steady_clock::time_point t0;
    bool timing = false;
    for (unsigned long long spins = 0;; ++spins) {
        if (*flag == seq) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return true; }
        if ((spins & 0xFFFFF) == 0xFFFFF) {
            const hipError_t e = hipStreamQuery(c->stream);
            if (e != hipSuccess && e != hipErrorNotReady) { c->err = std::string("kernel failed: ") + hipGetErrorString(e); return false; }
            const auto now = std::chrono::steady_clock::now();
            if (!timing) { t0 = now; timing = true; }
            else if (std::chrono::duration<double>(now - t0).count() > timeout_s) { c->err = "timeout waiting for the device"; return false; }
        }
        __builtin_ia32_pause();
    }
}

struct HostTimer {                // wall-clock scope, accumulated per name; a no-op unless the context was created under NALO_HOST_TIMING (two clock reads, a std::string
    nalo_ctx* c; const char* name; std::chrono::steady_clock::time_point t0;      // and a map lookup per scope, ~50 scopes per keyframe, are not free on a 1.3 ms step)
    HostTimer(nalo_ctx* ctx, const char* n) : c(ctx), name(n) { if (c->host_timing) t0 = std::chrono::steady_clock::now(); }
    ~HostTimer() { if (!c->host_timing) return; auto& e = c->host_t[name]; e.first += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); e.second++; }
};

struct ProfScope {               // HIP-event bracket on the ctx stream (only when profiling is enabled, and selected: nalo_profile_select)
    // external = true: the events are not recorded here but handed to hipExtLaunchKernelGGL, which timestamps the dispatch itself: no barrier
    // packets around the kernel (an event pair recorded on the stream costs ~10 us of bubbles per bracket on a latency-bound pipeline)
    nalo_ctx* c; const char* name; hipEvent_t a = nullptr, b = nullptr; bool external;
    ProfScope(nalo_ctx* ctx, const char* n, bool ext = false) : c(ctx), name(n), external(ext) {
        if (c->prof_on && (c->prof_only.empty() || c->prof_only == n) && (c->prof_every <= 1 || (c->prof_tick++ % (unsigned)c->prof_every) == 0)) {
            // events come from a pool (filled by nalo_profile_enable, refilled as brackets are drained): no hipEventCreate on the measured path
            for (hipEvent_t* e : {&a, &b}) { if (c->prof_pool.empty()) (void)hipEventCreate(e); else { *e = c->prof_pool.back(); c->prof_pool.pop_back(); } }
            if (!external) (void)hipEventRecord(a, c->stream);
        }
    }
    ~ProfScope() {
        if (a) { if (!external) (void)hipEventRecord(b, c->stream); c->prof[name].pending.emplace_back(a, b); }
    }
};

// kernels_imm.hip
int imm_create_launch(nalo_ctx* c, const float4* dI, int n, const int* u, const int* v, float* color, float* weights, float* gradH, float* energyTH);
int imm_trace_launch(nalo_ctx* c, const float4* dI, int n, const float* base, const int* host_idx, const float* KRKi, const float* Kt, const float* aff,
                     float* idmin, float* idmax, int* status, float* quality, float* lastUV, float* lastInterval);
int imm_optimize_resident_launch(nalo_ctx* c, const float4* const* dI, int W, const float K[4], const float* Rt, const float* aff, int n, const int* sel, const float* res, size_t N,
                                 int minObs, int* result, float* idepth_out, uint8_t* res_in, const int* n_dev = nullptr);
int imm_optimize_launch(nalo_ctx* c, const float4* const* dI, int W, const float K[4], const float* Rt, const float* aff, int n, const int* host, const float* base,
                        int minObs, int* result, float* idepth_out, uint8_t* res_in);
int dist_make_launch(nalo_ctx* c, const float4* pt_geo, const uint8_t* pt_flags, const int* blk_host, int Ppad, int frame, const float* KRKi, const float* Kt, uint8_t* seed, float* out);
// the selection loop of activatePointsMT over the resident set (nalo_imm_resident_activate)
constexpr unsigned kActIdxBits = 27, kActIdxMask = (1u << kActIdxBits) - 1, kActIdxMaxN = kActIdxMask;   // key = host << 27 | index: NALO_MAX_WINDOW = 16 hosts
constexpr int kActFirstRounds = 12, kActMaxRounds = 768;                    // rounds enqueued before the host looks: 12, then 48, 192, 768, 768, ...
struct ActParams {
    int n, W, frame, w1, h1, cw, ch;
    float minActDist;
    const float *res, *type, *KRKi, *Kt, *D0; const int* flagged;               // res: the resident block (N = n entries per array); flagged[W]
    int* fate; uint4* rec; uint2* items;                                        // rec[i] = {U | V << 16, key, need, cell} (need = kActNoRec: no survivor); items: {pixel, key} by cell
    int *cell_off, *cell_fill, *stats;                                          // cell_off[cw*ch + 1]: counts, then offsets; stats: survivors, accepted, rejected by an earlier point, rounds
};
int act_launch(nalo_ctx* c, const ActParams& P, bool first, int rounds, int* ctr, int* cnt, int* sel);
int pixsel_hists_launch(nalo_ctx* c, const float* absg0, float* ths, float* thsSmoothed);
int scan_ints_launch(nalo_ctx* c, int* a, int m);                              // exclusive scan of a[0..m) in place on c->stream, the total into a[m] (one workgroup)
// kernels_imm_carry.hip: the resident set across a keyframe (nalo_imm_resident_carry). Every pointer is device memory.
struct ImmCarryParams {
    int n, nb, m, mb, H;                                                        // old points and append-list entries with their 256-thread workgroups; OLD hosts
    int w, h, append_host, rank_live;                                           // append_host: NEW numbering, -1 none; rank_live: name an appended point by its rank among the list's live entries
    const int* host_map;                                                        // [H] old host -> new host, -1: the frame left
    const float *res, *type; float *res2, *type2;                               // the set and my_type (type NULL: none given), and the second buffer they are gathered into
    const uint8_t* code;                                                        // per old point 0 stays, 1 deleted, 2 deleted if its status is IPS_OOB; NULL: all stay
    const int* list; const float4* dI;                                          // append list (idx | status << 28) and level 0 of the new frame
    int *cnt, *src, *mover, *arank, *out;                                       // cnt: 2 H nb + 2 mb + nb + 1; src: n + m; mover: n; arank: m; out: 4 + NALO_MAX_WINDOW
};
int imm_carry_launch(nalo_ctx* c, const ImmCarryParams& P);
// host_init.hip: level 0 of the initialiser for nalo_ba_window_from_initializer, the device made the current side first (the host mirror is uploaded when it is
// the newer one; the initialiser's state does not change). u / v never change after setFirst: the host's copies serve the layout. NALO_ERR_STATE without setFirst.
struct InitLevel0 { int n, slot_first; const float *u_host, *v_host, *u, *v, *iR; double thisToNext[12]; };
int init_level0(nalo_ctx* c, const char* who, InitLevel0* out);
// kernels_init_window.hip: the ordered sum of iR and the constructor's verdict per level-0 point; then the kept points gathered into a two-frame window's arrays
struct InitWindowDev;                                                           // ba_device.h, beside CarryDev
int init_window_scan_launch(nalo_ctx* c, const float4* dI, const float* u, const float* v, const float* iR, int n, uint8_t* ok, float* sum);
int init_window_gather_launch(nalo_ctx* c, const InitWindowDev& A, int nblocks);
// kernels_pixsel.hip: the last map's compact list when it was made on `slot` (false otherwise): on the device with its holes (status 0), on the host without
bool pixsel_last_list(nalo_ctx* c, int slot, const int** dev, int* n_dev, const int** host_live, int* n_live);
// host_ba.hip: nalo_trk_set_ref_from_window's inputs gathered from the window on c->stream ({Ku | Kv | new_idepth | HdiF}, *n each, holes included)
int ba_trk_ref_inputs(nalo_ctx* c, int* slot, int* n, const float** dev);
// host_ba.hip: nalo_dense_fit_planes' window half. The device slots of host_frame's points in submission order (*kmap, *seg entries: a segment of the map
// nalo_trk_set_ref_from_window keeps), how many of them are valid (the host's mirror of the flags), the arrays the gather reads and the frame's slot
int ba_plane_inputs(nalo_ctx* c, int host_frame, int* slot, const int** kmap, int* seg, int* n_valid, const float4** geo, const uint8_t** flags);
// host_ba.hip: nalo_trk_fit_ground's window half (the marking of CoarseTracker.cpp:669-693). Entry k of kmap is the k-th point in (host, submission) order
struct GroundWindowView { int P, W; const int* kmap; const uint8_t* st_last; const float4* cpt_last; const uint32_t* pt_last; };
int ba_ground_inputs(nalo_ctx* c, GroundWindowView* V, const int** k2p);      // k2p[k]: submission index of entry k, built with the map
// ---- the map (host_map.hip, kernels_map.hip): removed points archived on the device, and the clouds the reference publishes per keyframe
// nalo_ba_marginalize_flagged's append: the window's arrays as the kernels read them. Entry k of kmap is the k-th point in (host, submission) order.
struct MapAppendDev {
    int P, nb;                                                                  // entries of kmap and their 256-lane workgroups
    const int *kmap, *blk_host;
    const uint8_t *flags, *ngood, *dec;                                         // dec / H: ba_flag_points_kernel's outputs per slot
    const float4 *geo, *col0, *col1, *acc;
    const float *prior, *relbs, *H;                                             // relbs: the buffer of the last pass that recorded relBS, taken BEFORE the marginalisation pass swaps it
    int frame_id[NALO_MAX_WINDOW];
    int *cnt, *hs, *hs_next;                                                    // cnt [nb + 1]: removed points per workgroup, scanned; hs [NALO_MAX_WINDOW][2]: per host {marginalised, out}
    nalo_map_record* const* chunks; long long base, cap; int chunk;             // record at archive position q lives at chunks[q / chunk][q % chunk]; cap: positions that exist
};
int map_append_rank_launch(nalo_ctx* c, const MapAppendDev& A);                 // counts + their scan
int map_append_write_launch(nalo_ctx* c, const MapAppendDev& A, bool patch);    // the records; patch: the two words marginalizePointsF's addPoint rewrites on a marginalised point
// a cloud's records: a virtual list of segments. kind 0: the resident immature set (every point; the frame's are picked by host_idx), 1: a segment of kmap (valid points),
// 2 / 3: an archive run, of which the pass takes the records of that status, 4 (nalo_map_render only): a piece of the dense archive. frame: the listed frame the
// segment belongs to (nalo_map_render's row of its transform table; 0 elsewhere). A kind-0 segment serves every frame at once: imm_frame[host_idx] is the
// point's frame (-1: the host is not listed)
struct MapSeg { const void* p; int start, n, kind, frame; };
struct MapSrcDev {
    const MapSeg* segs; int nseg, total, nb;
    const float* imm; int immN, imm_frame[NALO_MAX_WINDOW];
    const uint8_t* flags; const float4 *geo, *col0, *col1, *acc; const float *prior, *relbs;
    int* cnt;                                                                   // [nb + 1] survivors per workgroup, scanned
};
struct MapWorldDev { MapSrcDev S; float ci[4]; double m[12]; double* xyz; int cap; };                                           // cap: points xyz holds
struct MapCloudDev { MapSrcDev S; int mode; float scaledTH, absTH, minRelBS, ci[4]; const int* draws; float* xyz; uint8_t* rgb; int* stats; int cap; };   // stats: records [4] | survivors [4], zero before; cap: records the outputs hold
int map_world_launch(nalo_ctx* c, const MapWorldDev& D);
int map_cloud_launch(nalo_ctx* c, const MapCloudDev& D);
// host_map.hip: what nalo_ba_marginalize_flagged calls around its marginalisation. begin: room for `ub` more records (a refusal touches nothing), the ranks and the
// records, A.chunks / base / cap / chunk / cnt / hs filled in here; patch: behind the marginalisation's accumulation; fetch: the per-host counts on their way up, before
// the call's one wait; commit: the host index, after it
bool map_on(const nalo_ctx* c);
int map_append_begin(nalo_ctx* c, MapAppendDev& A, int W, int ub);
int map_append_patch(nalo_ctx* c);
int map_append_fetch(nalo_ctx* c);
void map_append_commit(nalo_ctx* c);
void map_destroy(nalo_ctx* c);
// ---- the keyframe graph (host_map.hip). add_frames: the pairs EnergyFunctional::insertFrame creates, for every ordered pair of ids without an entry; add_marg:
// marginalizePointsF's [1]++ from the per-(host row, target row) residual counts of a marginalisation pass (misc[2 (h + t W)], id_of_row: frame_id per device row)
inline bool graph_on(const nalo_ctx* c) { return c->graph_on; }
void graph_add_frames(nalo_ctx* c, int W, const int* ids);
void graph_add_marg(nalo_ctx* c, int W, const int* id_of_row, const double* misc);
// host_ba.hip: the window as the graph reads it. ids: frame_id of the frames nalo_ba_get_frames returns now; act[i * NALO_MAX_WINDOW + j]: the slots with RS_EXISTS of
// valid points hosted by frame i in the row of frame j (one launch, one 1 KB copy, one wait). sharded / W only when count is false.
struct GraphWindowView { int W; int ids[NALO_MAX_WINDOW]; bool sharded; int act[NALO_MAX_WINDOW * NALO_MAX_WINDOW]; };
int ba_graph_view(nalo_ctx* c, bool count, GraphWindowView* V);
// host_ba.hip: the window as nalo_map_frame_cloud reads it. widx = -1: frame_id is not in the window; pts_ok: the point arrays stand (kmap: the frame's seg entries, n_valid of them valid). ci: {fxi, fyi, cxi, cyi} of the CalibHessian (value_scaledi)
struct MapWindowView { int widx, n_valid, seg; bool pts_ok; const int* kmap; const uint8_t* flags; const float4 *geo, *col0, *col1, *acc; const float *prior, *relbs; float ci[4], cf[4]; bool sharded; };   // cf: {fx, fy, cx, cy} (value_scaledf)
int ba_map_view(nalo_ctx* c, int frame_id, MapWindowView* V);
// ---- the 3-D panel (nalo_map_render; host_map.hip, kernels_map_render.hip). The host half of kernels_map_render.hip is the call's arithmetic: that file is built
// without FMA contraction, so the products below are the ones include/nalo_gpu.h defines, operation by operation.
struct MrLine { double ua, va, ub, vb, za, zb, n, k0; int count, width; unsigned col; int pad; };   // a clipped, projected segment: samples k0 .. k0 + count - 1 of n
// MrCam { vw, vh, fx, fy, cx, cy, znear, zfar }: map_render_tri.h, with the triangle set-up that host and device share
struct MapRenderDev {
    MapSrcDev S; const float* M;                                                // M: [n_frames][12], row MapSeg::frame
    int mode; float scaledTH, absTH, minRelBS, ci[4]; MrCam cam;
    const MrLine* lines; int n_lines;
    unsigned long long* key; size_t padded;                                     // one word per pixel, rounded up (resolve_padded_pixels); all-ones between calls
    unsigned long long *cnt, *cnt_next;                                         // kMrCounters words: n_vertices, n_drawn_points, n_line_samples, 0, then the triangles' six (MrTrisDev); the idle buffer zeroed for the next call
    uint8_t* rgb; float* depth; unsigned background;                            // rgb: 3 bytes per key word; depth: 4
};
void map_render_transform(const double view[12], const double camToWorld[12], float M[12]);          // (float)(view . camToWorld)
void map_render_apply(const float M[12], const float p[3], float out[3]);                              // ((M0 x + M1 y) + M2 z) + M3 per row, in float
// one segment in view space (float endpoints) through the drop rules, the near clip, the projection and the viewport clip; false: dropped (no segment counted)
bool map_render_line(const MrCam& cam, const float a[3], const float b[3], unsigned col, int width, MrLine* out);
void map_render_frustum(const float cf[4], int w, int h, float sz, float pts[5][3]);                  // drawCam's apex and four corners (:630-649), camera space
// the triangles of nalo_map_render_mesh (kernels_map_render_mesh.hip): up to three sources behind one another in ONE launch; workgroup b serves source s when
// blk0[s] <= b < blk0[s + 1]. rgba: 4 bytes per vertex, read bytewise (a caller's array needs no alignment), NULL in colour_mode 1. cnt: the call's counter
// block; words 4..9 are n_tri_bad_index, n_tri_near, n_tri_guard, n_tri_degenerate, n_tri_large, n_tri_pixels
constexpr int kMrCounters = 12;
struct MrTriSrc { const float* xyz; const int* tri; const uint8_t* rgba; int nv, nt; };
struct MrTrisDev {
    MrTriSrc src[3]; unsigned blk0[4]; int n_src;
    float V[12]; MrCam cam; int colour_mode; long long max_box;
    unsigned long long *key, *cnt;
};
int map_render_tris_launch(nalo_ctx* c, const MrTrisDev& T);
int map_render_launch(nalo_ctx* c, const MapRenderDev& D, MrTrisDev* T = nullptr);   // points, lines, (T: triangles, its cam / key / cnt filled in here,) resolve on c->stream
// ---- the window panel (nalo_map_window_plot; host_map.hip, kernels_window_plot.hip): FullSystem::debugPlot from resident data
// host_ba.hip: the whole window as the painter reads it. Per window frame: frame_id, slot, its seg entries of the (host, submission) map and how many are valid
struct PlotWindowView {
    int W; bool pts_ok, sharded;
    int frame_id[NALO_MAX_WINDOW], slot[NALO_MAX_WINDOW], seg[NALO_MAX_WINDOW], n_valid[NALO_MAX_WINDOW]; const int* kmap[NALO_MAX_WINDOW];
    const uint8_t* flags; const float4* geo;
};
int ba_plot_view(nalo_ctx* c, PlotWindowView* V);
// the frames a panel paints: those frame_mask names (0: all), in window order. out_of: window frame -> painted frame or -1; per painted frame its window frame and
// level-0 irradiance. who: the caller's name in the refusal of a frame whose slot has no pyramid
int ba_plot_frames(nalo_ctx* c, const char* who, const PlotWindowView& V, unsigned frame_mask, int out_of[NALO_MAX_WINDOW], int frame_of[NALO_MAX_WINDOW],
                   const float* I[NALO_MAX_WINDOW], int* n_frames);
// the sources: a virtual list of segments, a frame's in the reference's painting order (its kmap segment, its archive runs once for status 2 and once for status 3), so
// that a source's position in its frame's sublist IS its priority. kind as MapSeg's; kind 0 is the whole resident set once (fstart 0, the frame from host_idx).
// widx: the window frame; fstart: where the frame's sublist starts
struct PlotSeg { const void* p; int start, n, kind, widx, fstart, pad; };
constexpr int kPlotResWords = 8;                                                // n_values, min_new, max_new, min_used, max_used, the rewritten pair, 0
struct WindowPlotDev {
    const PlotSeg* segs; int nseg, total;
    int mode, w, h, n_frames; float rainbow_scale, quality_scale;
    const float* imm; int immN;
    const uint8_t* flags; const float4* geo;
    int out_of[NALO_MAX_WINDOW];                                                // window frame -> painted frame, -1: masked out
    int fstart[NALO_MAX_WINDOW]; const float* I[NALO_MAX_WINDOW];               // per PAINTED frame: its sublist's start, its level-0 irradiance
    unsigned *key, *col; uint8_t* bgr;                                          // key: n_frames w h words rounded up (resolve_padded_pixels), zero between calls; col: total words; bgr: 3 bytes per key word
    unsigned* res; int *cnt, *cnt_next;                                         // res [kPlotResWords]; cnt [NALO_MAX_WINDOW][4] rings per painted frame and class, the idle buffer zeroed for the next call
    float io_min, io_max; int have_io;
};
int window_plot_launch(nalo_ctx* c, const WindowPlotDev& D);                   // [select, mode 7] scatter, resolve on c->stream
// ---- the initialiser's depth panel (nalo_init_depth_image; host_init.hip, kernels_init_plot.hip): CoarseInitializer::debugPlot from the resident Pnt arrays
struct InitPlotDev {
    int n, w, h; float rainbow_scale;
    const float *u, *v, *iR; const uint8_t* good; const float4* dI;             // the level's points and the first frame's texels of that level (x: the irradiance)
    unsigned *key, *col, *res; uint8_t* bgr;                                    // key: w h words rounded up (resolve_padded_pixels), zero between calls; col: n words;
};                                                                              // res: {n_good, sid, fac, 0}; bgr: 3 bytes per key word
int init_plot_launch(nalo_ctx* c, const InitPlotDev& D);                       // sum, scatter, resolve on c->stream
// ---- the residual panel (nalo_ba_residual_plot) and the read-back of projectedTo / state_energy (nalo_ba_get_pattern_projections); host_ba.hip,
// kernels_residual_plot.hip. Rows are the window's residual rows = its frames while the point arrays stand.
struct ResidualPlotDev {
    int W, Ppad, w, h;                                                          // residual rows, slots per row, image size
    const float* pre; const int* blk_host;                                      // the precalc records the last linearisation read ([W * W][kPreStride], host * W + target)
    const uint8_t *flags, *state; const float4* geo; const float2* energy;
    float *proj, *en_out;                                                       // the read-back: [W][Ppad][8][2] and [W][Ppad], either may be NULL
    // the painter: the host's points in painting order (entry k of kmap -> device slot), seg of them
    const int* kmap; int seg, host_row, energy_mode, n_frames; float rainbow_scale;
    int out_of[NALO_MAX_WINDOW];                                                // residual row -> painted image, -1: masked out
    const float* I[NALO_MAX_WINDOW]; double aff[NALO_MAX_WINDOW][2];            // per PAINTED image: its level-0 irradiance and the affL it is transferred with
    unsigned *key, *col; uint8_t* bgr; int* cnt;                                // key: n_frames w h words rounded up (resolve_padded_pixels), zero between calls; col: n_frames x seg words; bgr: 3 bytes
};                                                                              // per key word; cnt: {points, residuals, pattern pixels}, zero before
int residual_projections_launch(nalo_ctx* c, const ResidualPlotDev& D);        // rp_get_kernel on c->stream
int residual_plot_launch(nalo_ctx* c, const ResidualPlotDev& D);               // scatter, resolve on c->stream
// ---- the dense map (nalo_dense_update_map, nalo_map_dense_*)
constexpr int kDenseMaxClusters = 2048;      // = the most clusters a fit returns (kernels_plane.hip)
// host_map.hip: the dense archive as the copy pass writes it (the point at position q lives at chunks[q / chunk][q % chunk]; cap: positions that exist)
struct DenseArchiveView { nalo_dense_point* const* chunks; long long base, cap; int chunk; };
bool map_dense_on(const nalo_ctx* c);
int map_dense_reserve(nalo_ctx* c, long long ub, DenseArchiveView* V);          // room for ub more points; a refusal leaves the archive as it was
long long map_dense_frame_points(nalo_ctx* c, int frame_id);                   // the frame's points so far (0: none, or never seen)
void map_dense_commit(nalo_ctx* c, int frame_id, int n_points, int n_runs);     // after the call's last wait: the host index (the frame counts as seen from here on)
void map_dense_destroy(nalo_ctx* c);
// kernels_map.hip: the two products of a frame's dense points. segs: the frame's archive pieces in append order (MapSeg::p: nalo_dense_point, kind unused)
struct MapDenseDev { const MapSeg* segs; int nseg, total, nb; int* cnt; float ci[4]; double m[12]; const int* draws; double* wxyz; float* xyz; uint8_t* rgb; };
int map_dense_world_launch(nalo_ctx* c, const MapDenseDev& D);
int map_dense_cloud_launch(nalo_ctx* c, const MapDenseDev& D);                  // cnt[nb]: the survivors in all, behind the scan
// kernels_dense.hip: nalo_dense_update_map's device half. boxes_enqueue runs behind the fit's kernels and before its wait (rec / n_clusters_dev: the fit's records and
// their count on the device): every cluster's mask box in one pass, on its way up with the records. finish: the batched makeMap of every fitted cluster with a
// colour, the accept tests and the copy of the accepted runs into the archive; the call's second wait; runs[C] filled in
long long dense_candidates_bound(int w, int h);                                // pixels of [2,w-2)x[2,h-2) with i%3==0 || j%3==0: the most points one call can append
int dense_boxes_enqueue(nalo_ctx* c, const float* mask, const nalo_plane_cluster* rec, const int* n_clusters_dev, int cap_clusters);
int dense_update_finish(nalo_ctx* c, int slot, const nalo_plane_cluster* clusters, int C, const double camToWorld[12], const DenseArchiveView& V, long long frame_points,
                        nalo_dense_run* runs, int* n_appended, int* n_runs);
// host_map.hip: the frame's dense list as segments in append order (MapSeg::p: nalo_dense_point on the device; the list itself is host memory of the caller's:
// nothing is queued or staged). NALO_ERR_STATE without the dense archive or on a sharded window, NALO_ERR_ARG for a frame_id the archive has never seen; a frame
// without points gives total = 0
int map_dense_segments(nalo_ctx* c, const char* who, int frame_id, std::vector<MapSeg>* segs, int* total);
// ---- the TSDF volume (nalo_tsdf_*; host_tsdf.hip, host_tsdf.cpp, kernels_tsdf*.hip). The kernel files are built without FMA contraction: their arithmetic is the
// definition in include/nalo_gpu.h, operation by operation. Every kernel-argument struct below embeds the grid (tsdf_device.h: TsdfGridDev), which
// host_tsdf.hip fills in one place.
struct TsdfIntegrateDev {
    TsdfGridDev g;                                                              // g.col != NULL selects the coloured instantiation; tsdf, weight and col are written
    int lo[3], hi[3];                                                           // the culling box, hi exclusive, not empty
    float trunc, max_weight, M[12], fx, fy, cx, cy, min_depth, max_depth;
    const char* depth; long long sy, sx; int w, h;                              // the plane by byte strides
    unsigned long long* updated;                                                // zero before
    // colour: the pixel's bytes lie at colour + pv csy + pu csx + csc[plane] (csc already holds the B, G, R order of the caller's channels)
    const unsigned char* colour; long long csy, csx, csc[3];
};
int tsdf_integrate_launch(nalo_ctx* c, const TsdfIntegrateDev& D);
// nalo_tsdf_replace_depth (kernels_tsdf_replace.hip, built without FMA contraction): remove on one side, then add on the other, per voxel, in one launch over the
// hull of the two sides' boxes. A side is a camera at an estimate and its planes; the predicate reads it as it reads TsdfIntegrateDev (tsdf_voxel_device.h).
struct TsdfSideDev {
    int on, coloured;                                                           // on: the side exists and its box is not empty; coloured: it moves the colour words
    int lo[3], hi[3];                                                           // the voxels the side may touch, hi exclusive: its culling box (remove: cut by the caller's box)
    float M[12], fx, fy, cx, cy, min_depth, max_depth, s;                      // M: nalo_tsdf_est_world_to_cam; s: (float)est.s
    const char* depth; long long sy, sx; int w, h;                              // the plane by byte strides
    const unsigned char* colour; long long csy, csx, csc[3];                    // as TsdfIntegrateDev's
};
struct TsdfReplaceDev {
    TsdfGridDev g;                                                              // g.col != NULL selects the coloured instantiation (a side is coloured); tsdf, weight and col are written
    int lo[3], hi[3];                                                           // the hull of the sides that are on, hi exclusive, not empty
    float trunc, max_weight;
    TsdfSideDev rem, add;
    unsigned long long* counts;                                                 // [4], zero before: written, removed, reset, added
};
int tsdf_replace_launch(nalo_ctx* c, const TsdfReplaceDev& D);
// nalo_tsdf_replace_depth_n (kernels_tsdf_replace_n.hip, built without FMA contraction): the chain of n pairs per voxel in one launch over the hull of every
// side's box. 2 n sides do not fit the kernel arguments: they lie in a device table, pair k's remove side at [2k] and its add side at [2k + 1] (on = 0: absent).
constexpr int kTsdfReplaceMaxPairs = 16;                                        // the largest window the library accepts
struct TsdfReplaceNDev {
    TsdfGridDev g;                                                              // g.col != NULL selects the coloured instantiation (some side is coloured); tsdf, weight and col are written
    int lo[3], hi[3];                                                           // the hull of the sides that are on, hi exclusive, not empty
    float trunc, max_weight;
    int n;                                                                      // pairs, 1 .. kTsdfReplaceMaxPairs
    const TsdfSideDev* sides;                                                   // [2 n], device memory, read only
    unsigned long long* counts;                                                 // [4 n + 1], zero before: per pair removed, reset, added, written; then written_total
};
int tsdf_replace_n_launch(nalo_ctx* c, const TsdfReplaceNDev& D);
int tsdf_fill_launch(nalo_ctx* c, float* tsdf, float* weight, size_t n);       // 1.0f / 0.0f
// one array's sub-block [lo, lo + size) to (to_volume = 0) or from (1) a contiguous block, x fastest
int tsdf_block_launch(nalo_ctx* c, float* vol, float* block, const int dims[3], const int lo[3], const int size[3], int to_volume);
// nalo_tsdf_shift: dst voxel (i, j, k) = src voxel (i + s[0], j + s[1], k + s[2]) as 32-bit words, the initial values where that lies outside the grid. Out of
// place: src is read only, every word of dst is written, the two never alias. src_col != NULL selects the coloured instantiation; the other touches neither
// colour pointer
struct TsdfShiftDev {
    const unsigned *src_tsdf, *src_weight, *src_col;                            // col: [3][n], the planes n words apart
    unsigned *dst_tsdf, *dst_weight, *dst_col;
    int nx, ny, nz, s[3];                                                       // |s[a]| <= dims[a]: the host clamps, beyond it nothing is kept either way
    long long n;                                                                // nx ny nz <= 2^29
};
int tsdf_shift_launch(nalo_ctx* c, const TsdfShiftDev& D);
// nalo_tsdf_mesh and nalo_tsdf_surface_points (kernels_tsdf_mesh.hip): an ordered compaction over the sub-box, kTsdfVoxPerBlock voxels to a workgroup. The
// surface points are the mesh's vertices on the axis edges: they run the classify and the vertex pass restricted to those, and no triangle pass.
constexpr int kTsdfVoxPerBlock = 1024;                                          // 256 lanes x 4 consecutive voxels of the sub-box
struct TsdfMeshDev {
    int lo[3], size[3], total, nb;                                              // total: voxels of the sub-box (<= 2^28; the surface points: 2^29); nb: its workgroups
    TsdfGridDev g;                                                              // read only; g.col != NULL: nalo_tsdf_mesh_color. Behind the box: the triangle pass keeps its instruction order so
    float min_weight;
    unsigned char* vmask; int* vbase;                                           // [total + 3] each (a lane stores its four at once): a voxel's edges that carry a vertex (bit m - 1), the index of its first vertex
    int *cntv, *cntt;                                                           // [nb + 1] each: vertices / triangles per workgroup, scanned; [nb] the sums (cntt read as unsigned)
    float* xyz; int* tri; long long capv, capt;                                 // written only when both sums fit
    unsigned* rgba;                                                             // nalo_tsdf_mesh_color: [capv] vertex colours R | G << 8 | B << 16 | 255 << 24
};
// axis_only (the surface points): vbase, cntt, tri, capt and rgba are not looked at
int tsdf_mesh_classify_launch(nalo_ctx* c, const TsdfMeshDev& D, bool axis_only);   // classify and the scans on c->stream
int tsdf_mesh_write_launch(nalo_ctx* c, const TsdfMeshDev& D, bool axis_only);      // the vertex pass, and the mesh's triangle pass
// nalo_tsdf_integrate_frame's plane: D[v][u] = 1.0f / idepth of the record with the highest position at (u, v), 0 without one. key: w h words, zero between calls.
// colour != NULL (a coloured volume): w h words, that record's B | G << 8 | R << 16, 0 without one - a U8 plane of three channels with stride_x 4, stride_c 1
// segs is HOST memory: the segments travel as kernel arguments, kTsdfSegsPerLaunch to a launch, so the call stages nothing that a later call could overwrite
constexpr int kTsdfSegsPerLaunch = 32;
int tsdf_frame_plane_launch(nalo_ctx* c, const MapSeg* segs, int nseg, unsigned long long* key, float* plane, unsigned* colour, int w, int h);
// nalo_tsdf_raycast (kernels_tsdf_raycast.hip, built without FMA contraction): one lane per pixel, an 8 x 8 tile to a wave. It reads the volume only.
struct TsdfRaycastDev {
    TsdfGridDev g;                                                              // read only; g.col != NULL: with_colour
    float min_weight;
    float R[9], t[3], fx, fy, cx, cy; int w, h;                                 // camToWorld rounded to float; the view
    float min_depth, step; int N;                                               // z_n = min_depth + (float)n * step, n < N
    float* depth; float* normal; unsigned* rgba;                                // [h][w], [h][w][3] (with_normals), [h][w] words R | G << 8 | B << 16 | A << 24 (with_colour)
    unsigned long long* cnt;                                                    // n_hit, n_back, n_normal: zero before
};
int tsdf_raycast_launch(nalo_ctx* c, const TsdfRaycastDev& D);
// nalo_tsdf_align_eval (kernels_tsdf_align.hip, built without FMA contraction): one lane per visited pixel, an 8 x 8 tile of them to a wave. It reads volume and
// plane and writes only what is named here. The sums: H's upper triangle row-major (28), b (7), E, sum r r.
constexpr int kTsdfAlignSums = 37, kTsdfAlignStride = 40;                       // a workgroup's partial record: 37 doubles and two words of counts, padded to 320 B
struct TsdfAlignDev {
    TsdfGridDev g;                                                              // read only
    float min_weight;
    float M[12], fx, fy, cx, cy;                                                // [s R | t] rounded to float, rows of four; K of the plane
    float min_depth, max_depth, huber; int step, dof;
    const char* depth; long long sy, sx; int w, h;                              // the plane by byte strides
    int vw, vh;                                                                 // visited pixels per row and column: ceil(w / step), ceil(h / step)
    float* records;                                                             // NULL, or [h][w][10]: written at visited pixels only
    double* partial;                                                            // [workgroups][kTsdfAlignStride]: the 37 sums, then the four counts in two words
    unsigned* ticket;                                                           // zero between launches
    double* out;                                                                // host-mapped: 37 doubles, then the four counts as 64-bit integers
};
int tsdf_align_launch(nalo_ctx* c, const TsdfAlignDev& D);
long long tsdf_align_blocks(int vw, int vh);                                    // the workgroups tsdf_align_launch starts
void tsdf_destroy(nalo_ctx* c);
// nalo_tsdf_archive_* (kernels_tsdf_archive.hip): the welded mesh archive. Integers and words only: nothing here depends on the contraction policy. A vertex's key is
// (gx, gy, gz, m) as one int4; the table is open-addressed with linear probing, 32-bit slots that hold an archived vertex index or kTsdfArchiveEmpty, a power of
// two of them, and the host keeps its load at or below one half BEFORE a launch (every piece vertex counted as new). Every probe loop is bounded by the slot count;
// a lane that exhausts it raises *err and stops.
constexpr int kTsdfArchiveEmpty = -1;
struct TsdfArchiveDev {
    // the piece: the device mesh behind nalo_tsdf_mesh and the scratch its passes left (vmask, vbase), the sub-box and the volume's base at the time of the call
    const unsigned char* vmask; const int* vbase; int lo[3], size[3], base[3], total;
    const float* p_xyz; const unsigned* p_rgba; const int* p_tri; int p_nv, p_nt;   // p_rgba NULL: an uncoloured archive
    int4* p_key; int* p_map;                                                    // [p_nv] each: the piece's keys; the archived index of every piece vertex (-1 behind the lookup: new)
    int* cnt; int nb;                                                           // [nb + 1]: new vertices per workgroup of 256 piece vertices, scanned; [nb] their sum
    // the archive
    float* xyz; unsigned* rgba; int4* key; int* tri; int nv, nt;                // nv, nt: what it holds before this append; the buffers have room for nv + p_nv and nt + p_nt
    int* table; unsigned mask;                                                  // slots - 1
    int* err;                                                                   // raised to 1 by a lane whose probe ran through every slot
};
int tsdf_archive_keys_launch(nalo_ctx* c, const TsdfArchiveDev& D);             // the piece's keys from vmask / vbase
int tsdf_archive_append_launch(nalo_ctx* c, const TsdfArchiveDev& D);           // lookup, scan, insert, triangles
int tsdf_archive_rebuild_launch(nalo_ctx* c, const int4* key, int nv, int* table, unsigned mask, int* err);   // an all-empty table filled from the key array in one pass
void tsdf_archive_destroy(nalo_ctx* c);
// host_ba.hip: frame_id (nalo_frame_state) of window frame host_frame, which ba_plane_inputs has validated
int ba_frame_id(nalo_ctx* c, int host_frame);
// host_ba.hip
void ba_destroy(nalo_ctx* c);
// host_rccl.hip
void rccl_release(nalo_ctx* c);
// host_init.hip
void init_destroy(nalo_ctx* c);
// kernels_pixsel.hip
void pixsel_destroy(nalo_ctx* c);
void pixsel_invalidate_hists(nalo_ctx* c, int slot);
void pixsel_invalidate_map(nalo_ctx* c, int slot);     // the slot's mask changed under an unchanged image: the last map (nalo_pixsel_make_maps_lidar reads the mask) goes, the gradient histograms stay
// staging for the immature-point entry points: pinned host block + device block of `floats` 4-byte words (grown on demand)
int imm_stage(nalo_ctx* c, size_t words);
int imm_put_launch(nalo_ctx* c, float* dst, const float* src, int n);
// kernels_init.hip: one calcResAndGS pass over one level. Every per-point array is a device pointer; idepth (the current inverse depths) may be NULL, then calcEC's
// three sums (slots 91..93) stay zero. sums: 96 doubles, on the device or (mapped) in host-mapped memory the caller polls.
struct InitParams {
    const float4 *colorRef, *colorNew; int wl, hl, n;
    float fx, fy, cx, cy, RKi[9], t[3], r2new0, r2new1, alphaOpt, couplingWeight;
    const float *u, *v, *idepth, *idepth_new, *iR, *energy, *outlierTH; const uint8_t* isGood;
    uint8_t* isGood_new; float *energy_new, *maxstep, *lastHessian_new, *Jb;
};
struct InitInc { float v[8]; };
int init_calc_launch(nalo_ctx* c, InitParams& P, int lvl, double* sums, int mapped = 0, double seq = 0);   // mapped: sums is host-mapped, [95] receives seq last
int init_do_step_launch(nalo_ctx* c, int n, const uint8_t* isGood, const float* Jb, const float* maxstep, const float* idepth, float lambda, const float inc[8], float* idepth_new);
int init_apply_step_launch(nalo_ctx* c, int n, uint8_t* isGood, const uint8_t* isGood_new, float* idepth, float* idepth_new, const float* iR, float* energy, const float* energy_new,
                           float* lastHessian, const float* lastHessian_new);
// the dependency-ordered sweeps (optReg: mode 0, the top level's resetPoints: mode 1) and the per-point parts of resetPoints / propagateDown / propagateUp
constexpr int kSweepNT = 128;                          // lanes of the sweep workgroup = the most points a schedule step may hold. trackFrame at 1224x368, same box:
                                                       // 64 lanes (no second wave at the barrier, 37 % more steps) 8.1 ms, 128: 7.4 ms, 256: 8.0 ms
constexpr size_t kSweepLdsBytes = 158 * 1024;          // of the 160 KB per workgroup
int init_sweep_launch(nalo_ctx* c, int mode, int n, int nsteps, const int* off, const int* rec, float* iR, uint8_t* isGood, float* idepth, float* idepth_new, float regWeight, float* scratch);
int init_reset_launch(nalo_ctx* c, int n, float* energy, float* idepth_new, const float* idepth);
int init_fill_launch(nalo_ctx* c, int n, float* iR, float* idepth_new, float* lastHessian);
int init_propagate_down_launch(nalo_ctx* c, int n, const int* parent, const uint8_t* pGood, const float* pLastHessian, const float* pIR, uint8_t* isGood, float* iR, float* idepth,
                               float* idepth_new, float* lastHessian);
int init_propagate_up_launch(nalo_ctx* c, int nT, const int* child_off, const int* child_idx, const uint8_t* cGood, const float* cIR, const float* cLastHessian, uint8_t* isGood,
                             float* iR, float* idepth);
// host_init.hip: the host arithmetic either side of that pass (pose / affine / alpha terms in, Accumulator9 sums -> H, b, Hsc, bsc, E out), shared by the staged
// entry point (nalo_init_calc_res_and_gs) and the resident trackFrame
struct InitPose { float alphaEnergy; };
void init_pose_setup(const nalo_ctx* c, int lvl, int n, const nalo::SE3& T, const double aff[2], float alphaW, float alphaK, float couplingWeight, InitParams& P, InitPose& X);
void init_sums_to_system(const double* sums, const nalo::SE3& T, int n, const InitParams& P, const InitPose& X, double* H, double* b, double* Hsc, double* bsc, double E3[3]);
// kernels_pyramid.hip
constexpr int NALO_LM_LOST_BLOCK = 1000;     // trk_lm_launch only (never crosses the C ABI): the persistent kernel's workgroups were not co-resident
int pyramid_build(nalo_ctx* c, nalo::FrameSlot& s, const float* gammaB_dev);
int frame_tile_level0(nalo_ctx* c, nalo::FrameSlot& s);
void hbm_stream_launch(hipStream_t st, const float4* a, const float4* b, float4* d, size_t n, int triad);
int ingest_launch(nalo_ctx* c, hipStream_t st, const void* raw, int bpp, int wOrg, int hOrg, const float* G, const float* vinv, const float2* remapXY, int photometric,
                  float factor, const uint8_t* mask_org, const uint8_t* bgr_org, float* out_I, float* out_mask, uint8_t* out_bgr);
// kernels_ingest_dev.hip: the same from planes on the device, every descriptor already validated (host_api.hip: dev_plane_validate). img: NALO_DT_U8 / _U16 sensor
// frame (und_wOrg x und_hOrg) or NALO_DT_F32 rectified irradiance (w x h, copied word for word; G .. factor unused). attach: mask and / or colour resized into the
// slot's planes (out_mask w*h floats, out_bgr 3*w*h bytes B,G,R); either descriptor may be null
int ingest_dev_launch(nalo_ctx* c, hipStream_t st, const nalo_dev_plane& img, const float* G, const float* vinv, const float2* remapXY, int photometric, float factor, float* out_I);
int attach_launch(nalo_ctx* c, hipStream_t st, const nalo_dev_plane* mask, const nalo_dev_plane* colour, int colour_is_rgb, float* out_mask, uint8_t* out_bgr);
// kernels_trk_lm.hip: workgroups of trk_lm_kernel for a largest level of maxn points; the whole pyramid descent of nalo_trk_track in one persistent launch
int trk_lm_blocks(int maxn);
// nalo_trk_track_tries in one persistent launch (trk_lm_tries_kernel): summary[32] and run x kLmRecDoubles records, see kernels_trk_lm.hip
constexpr int kLmRecDoubles = 32;            // per try: ok taken abort_lvl have_repeated n_evals | lastRes(5) flow(3) T(12) aff(2) | evals per level(5)
int trk_lm_tries_launch(nalo_ctx* c, int slot_new, const double* tries, int n_tries, const double aff_init[2], const double ref_aff[2], const float exposures[2],
                        int coarsest, double thr, double summary[32], double* records);
int trk_lm_launch(nalo_ctx* c, int slot_new, const double T0[12], const double aff0[2], const double ref_aff[2], const float exposures[2], int coarsest, int stop_lvl, const double* minRes, double out24[32]);
// kernels_depth_image.hip: debugPlotIDepthMap on c->stream. scr: kDepthImageScratchWords words (zeroed here; the results are its last 8: n_positive, min_new, max_new,
// min_used, max_used, the rewritten minmax pair), bgr: 3 w h bytes. Nothing is painted when the map holds no positive value (n_positive = 0).
constexpr int kDepthImageScratchWords = 2048 + 2 * 2048 + 2 * 512 + 16 + 8;
int depth_image_launch(nalo_ctx* c, const float* idepth, const float* I, float io_min, float io_max, int have_io, unsigned* scr, uint8_t* bgr);
// kernels_tracker.hip
int trk_build_ref(nalo_ctx* c, int n, const float* dKu, const float* dKv, const float* dId, const float* dHdi);
// the same reference from a depth plane (nalo_trk_set_ref_from_depth, already checked): one seed kernel in place of the scatter and the sum pyramid
int trk_build_ref_from_depth(nalo_ctx* c, const nalo_dev_plane& d, float min_depth, float max_depth, float hdi, int step, float min_grad, int* n_seeded);
int trk_append_plane_launch(nalo_ctx* c, const float* mask, const float4* dIref, const float dir[3], float dis, float refColor, int x0, int nx, int y0, int ny, int n0, int* n_dev);
// the append loop of CoarseTracker.cpp:582-666 over the records nalo_trk_fit_planes has just written on the device (hdr: kernels_plane.hip's header words)
int trk_append_clusters_launch(nalo_ctx* c, const float* mask, const float4* dIref, nalo_plane_cluster* rec, int* hdr, int cap_clusters);
int trk_eval_launch(nalo_ctx* c, int slot_new, int lvl, const float RKi[9], const float t[3], const float Ki[9],
                    float affa, float affb, float b0, float cutoff, float maxEnergy, double out64[64]);

}  // namespace nalo
