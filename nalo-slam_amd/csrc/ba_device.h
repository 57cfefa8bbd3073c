// Device-side layout of the BA window (shared by kernels_ba.hip and host_ba.hip).
//
// Points are sorted by host frame; every host segment is padded to a multiple of kBlk so that one 256-thread
// block only holds points of one host (blk_host[b]). One residual slot per (target t, point d): arrays are
// [W][Ppad], t-major, so a wave reads consecutive points of one target: coalesced.
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>
#include <cstdint>

namespace nalo {

constexpr int kBlk = 256;            // points per linearize block
constexpr int kTopVals = 93;         // 91 AccumulatorApprox entries + residual count + energy
constexpr int kTopStride = 96;       // floats per (block, target) partial
constexpr int kPreStride = 40;       // floats per (host,target) precalc record
constexpr int kThSmallSlots = 16384; // Ppad up to this: frameEnergyTH by ba_th_small_kernel (one workgroup); beyond: the radix select of ba_th_fill_kernel
constexpr int kPreDirectSlots = 32768;   // Ppad up to this: ba_linearize reads the precalc records from mapped host memory; beyond: ba_pull_kernel copies them
constexpr int kThDblAB = 1024, kThDblC = 256;   // setNewFrameEnergyTH: the three radix histograms (2048 + 2048 + 512 bins) as doubles, two bins per double = the cross-rank payloads of a sharded window

// residual slot state byte
enum : uint8_t { RS_STATE_MASK = 3, RS_EXISTS = 4, RS_ACTIVE = 8, RS_LINEARIZED = 16 };
// point flags
enum : uint8_t { PT_VALID = 1, PT_MARG = 2, PT_HAS_PRIOR = 4, PT_DROP = 8 };   // PT_MARG / PT_DROP: the resident decisions of ba_flag_points_kernel (MARGINALIZE / both DROP classes)
// decision of flagPointsForRemoval per point (nalo_ba_flag_points)
enum : uint8_t { DEC_KEEP = 0, DEC_DROP_NORES = 1, DEC_DROP = 2, DEC_MARGINALIZE = 3 };

// precalc record (FrameFramePrecalc, reference src/FullSystem/HessianBlocks.h:80-107 + adHTdeltaF):
//  [0..8] PRE_KRKiTll  [9..11] PRE_KtTll  [12..20] PRE_RTll_0  [21..23] PRE_tTll_0  [24,25] PRE_aff_mode  [26] PRE_b0_mode
//  [27..34] adHTdeltaF[h + t*W]  (EnergyFunctional.cpp:175-181)
struct BADev {
    int W, P, Ppad, nblocks, w, h;
    const float* calib;                         // [10] {fxl, fyl, cxl, cyl, fxli, fyli (CalibHessian::value_scaledf / value_scaledi), cDeltaF[4] (EnergyFunctional)}
    const float4* img[16];                      // level-0 {I,dx,dy,0} of every window frame (row major)
    const float* img_t[16];                     // the same texels, 12 bytes each, in 5x2 tiles of 128 bytes (frame_tile_level0): what ba_linearize gathers from
    int wt;                                     // tiles per tile row = ceil(w / 5)
    int lin_sub;                                // ba_linearize workgroups (= fp64 partials) per point block: 1 = 256 threads, 4 = one wave each (small windows)
    const float* pre;                           // [W*W][kPreStride], index h*W + t
    float* frameTH;                             // [W] frameEnergyTH (device resident, updated by the quantile kernel)
    const int* blk_host;                        // [nblocks]
    const int* blk_order;                       // [8][xcd_len]: point blocks an XCD walks (spatial eighth of every host), -1 = none
    int xcd_len;
    // points
    float4* pt_geo;                             // {u, v, idepth, idepth_zero}
    const float4 *pt_col0, *pt_col1, *pt_w0, *pt_w1;
    float* pt_prior;                            // EFPoint::priorF
    uint8_t* pt_flags;
    float4* pt_acc;                             // {Hdd_accAF, bd_accAF, HdiF, bdSumF}
    float4* pt_hcd;                             // Hcd_accAF
    uint8_t* pt_ngood;
    // point history (nalo_ba_set_point_history), NULL without one: PointHessian::numGoodResiduals and lastResiduals[2] packed in one word,
    // byte 0 / 1 = window index of lastResiduals[0 / 1].first (int8, -1 = null), byte 2 / 3 = lastResiduals[0 / 1].second
    int* pt_numgood; uint32_t* pt_last;
    float* pt_step;
    float* pt_backup;
    const unsigned* gate_p; unsigned* gate_err; unsigned gate_p_want;   // ba_linearize_kernel: NULL, or the gate of its precalc records (GateBlock::p_seq)
    const float* adF;                           // float adjoints [adHostF (W*W*64) | adTargetF (W*W*64)], index (h + t*W)*64 + i*8 + j (ba_resub_kernel, XMODE 2)
    float* pt_relbs;                            // max relBS over this pass' active residuals (fix mode): the pass' atomicMax target, all zero when the pass starts
    float* pt_relbs_next;                       // the buffer of the NEXT fix pass: zeroed by this pass' idle (target == host) workgroups - no fill launch on the path
    // residual slots [W][Ppad]
    uint8_t* rs_state;
    float2* rs_energy;                          // {state_energy, state_NewEnergy}
    float4 *rs_jp0, *rs_jp1;                    // EFResidual::JpJdF
    float4* rs_pp0; float2* rs_pp1;             // per-slot share of the point sums: {bd, Hdd, Hcd0, Hcd1}, {Hcd2, Hcd3}
    float4* rs_cpt;                             // {Ku, Kv, new_idepth, relBS} (centerProjectedTo), written when fix/marg
    float* en_new;                              // [Ppad] state_NewEnergyWithOutlier of residuals targeting frame W-1 (-1 = none)
    double *th_bufAB, *th_bufC;                 // radix-select histograms of setNewFrameEnergyTH, two bins per double: A | B (1024 doubles each), C (256, behind the stitched systems)
    unsigned* th_state;                         // {count, k below bin A, bin A, empty, k below bin B, bin B}
    // partials
    double* top_partial;                        // [nblocks*lin_sub][W][kTopStride]: one partial per ba_linearize workgroup and target (fp64: one rounding less before the cancelling H_A - H_sc)
    double* sc_partial;                         // [sc_groups * sc_split][T(T+1)/2 upper tiles][256] (MFMA register order)
    int sc_split;                               // 1 or 4 workgroups per point block in ba_sc_kernel (4 for small windows)
    const int* host_blk;                        // [W+1] point-block range of every host
    const int* sc_grp;                          // [W+1] ba_sc workgroup-group range of every host (groups of sc_bpw blocks)
    int sc_bpw, sc_groups;                      // blocks per group (1 when sc_split > 1), total groups
    // settings (nalo_set_settings): setting_affineOptModeA / B < 0 zero JabF[0] / JabF[1] (Residuals.cpp:241-242)
    int fix_a, fix_b;
    int reset_oob;                              // 1: the pass starts from resetOOB'ed residuals (the first linearisation of optimize(), FullSystemOptimize.cpp:412-429): state = IN, energies 0
    int no_th;                                  // 1: this pass does not feed setNewFrameEnergyTH (the re-run that applies an accepted step, setting_forceAceptStep = false)
    double* noapply_E;                          // [nblocks*lin_sub][W] energy partials of a linearisation that is NOT applied (FIX = 2)
};

// {xc (4) | xAd [W*W][8]} of resubstituteFPt for windows of up to 8 frames, passed by value as kernel arguments (ba_resub_kernel)
constexpr int kXadArgFrames = 8;     // windows up to this many frames pass {xc, xAd} to the back-substitution as kernel arguments (XadArg); larger ones pass x
                                     // and every workgroup builds its host's rows of xAd (ba_resub_kernel, XMODE 2)
struct XadArg { float v[4 + kXadArgFrames * kXadArgFrames * 8]; };

// Gate of a kernel that is enqueued BEFORE its inputs exist (round 4, small single-GPU windows): the host still solves the system while the back-substitution and
// the next linearisation already sit in the stream; each spins (one lane per workgroup, bounded) on a word of host-mapped memory until the host has written the
// inputs - the step {xc, xAd}, the precalc records - and then the sequence number. What it saves per Gauss-Newton iteration is the launch latency of the two
// kernels on the critical path (the device starts ~1.5 us after the host's store instead of 5-6 us after its launch call). 0xFFFFFFFF = cancelled: the kernel returns
// without touching anything (the host's error paths), as it does when the bound expires (and then raises err).
// (the payload starts on its own 128-byte line: a gated kernel's first look at a flag is a cached scalar load made BEFORE the host writes the payload, and a device
// cache line that held both would hand the payload's loads the bytes of the iteration before)
struct GateBlock { unsigned x_seq, p_seq, err, pad[29]; float x[4 + NALO_MAX_WINDOW * NALO_MAX_WINDOW * 8]; };
static_assert(offsetof(GateBlock, x) == 128, "flags and payload of the gate block on separate cache lines");
constexpr unsigned kGateCancel = 0xFFFFFFFFu;
struct GateArg { const unsigned* flag; unsigned* err; const float* x; unsigned want; };
__device__ __forceinline__ bool gate_wait(const unsigned* flag, unsigned want, unsigned* err) {      // one lane; true = the inputs are there
    // RELAXED system-scope loads (always served by the host's memory) + a compiler barrier: an ACQUIRE at system scope invalidates the L2 on every poll, and the
    // kernel behind the gate then finds its points, residuals and texels gone (measured: 46 -> 96 us per iteration). Nothing the gate orders lives in a device
    // cache: the inputs are in host-mapped memory, read after the loop in program order (the hardware does not issue loads past an unresolved branch).
    // First a SCALAR load - the path the precalc records themselves take (scalar cache + L2, shared by the workgroups): a gate that is already open (the
    // linearisation's usually is: the host wrote its records while the back-substitution ran) then costs what one more record word costs. 256 workgroups asking
    // the host for one word with cache-bypassing loads are served one after the other, ~75 ns each (measured: 15 -> 34 us per gated linearisation; a volatile load is
    // the same sc0 sc1 access). The value is unique per launch: a cached copy can only be an older, closed one, and falls through to the polling loop.
    {
        unsigned v0;
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v0) : "s"(flag) : "memory");
        if (v0 == want) { __atomic_signal_fence(__ATOMIC_ACQUIRE); return true; }
    }
    for (unsigned spins = 0; spins < (1u << 21); ++spins) {
        const unsigned v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (v == want) { __atomic_signal_fence(__ATOMIC_ACQUIRE); return true; }
        if (v == kGateCancel) return false;
        __builtin_amdgcn_s_sleep(2);
    }
    if (err) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return false;
}

// What may ride along with ba_reduce_kernel: the newest frame's energy threshold of a small window (one more workgroup: ba_th_small's body) and, on a misc-only
// fetch, the publication of the tail {misc, step sums, TH, 1.0} + sequence number into host-mapped memory by the last workgroup to finish
struct RedExtra {
    const float* th_en; int th_n; float* th_out;             // th_en != NULL: one more workgroup computes setNewFrameEnergyTH from en_new[0..th_n)
    double* pub; double seq; unsigned* ticket; const float* th_src;   // pub != NULL: mapped tail block; th_src = frameTH of the newest frame
};

// Stitch operands (kernels_ba.hip ba_stitch_kernel)
struct StitchDev {
    const double* AD;                           // [adHost (W*W*64) | adTarget (W*W*64)], index (h + t*W)*64 + i*8 + k
    const double *M_top, *M_sc;                 // acc13 [W*W][169], G [W][NPL*NPL]
    double* H;                                  // the stitched block (StitchLayout)
    unsigned* ticket;
    int W, n1, NPL;
};

// The stitched block of a window of W frames (n1 = 8W + 5), in doubles. The reduce and stitch kernels fill it on the device (BAWindow::stitched) and publish it
// into a mapped host mirror (BAWindow::stitched_host):
//   [H~_A (n1^2) | H~_sc (n1^2) | misc: {count, energy} per (host, target) (2 W^2) | step sums (3) | {TH sum, ranks} (2)] = npub doubles.
// In the mirror the sequence number the host polls follows them (flag, written last); the mirror's tail is padded to 16 doubles. On the device level C's
// histogram of the threshold's radix select (kThDblC doubles) starts at the next multiple of 16 doubles: a sharded window sums it with the systems in one all-reduce.
struct StitchLayout {
    size_t top, sc, misc, step, th, flag, npub, lo, dev_size, host_size;
    constexpr StitchLayout(int n1, int W)
        : top(0), sc((size_t)n1 * n1), misc(2 * sc), step(misc + 2 * (size_t)W * W), th(step + 3), flag(th + 2), npub(flag),
          lo((npub + 15) & ~(size_t)15), dev_size(lo + kThDblC), host_size(step + 16) {}
};
// ba_reduce_kernel (kernels_ba.hip) publishes the tail from misc on with its own count, ntail = 2 W^2 + 5, and puts {TH, 1.0} at ntail - 2
static_assert(StitchLayout(21, 2).npub - StitchLayout(21, 2).misc == 2 * 2 * 2 + 5 && StitchLayout(21, 2).th - StitchLayout(21, 2).misc == 2 * 2 * 2 + 5 - 2,
              "StitchLayout and ba_reduce_kernel's tail disagree");

// ---- A window issued on the device (nalo_ba_carry_window, nalo_ba_window_from_initializer). What a fresh slot holds is defined HERE, once: IssuePoint's
// defaults are the padding slot, issue_store_point / issue_store_row write a slot's point arrays and rows with every zero beside them. nalo_ba_set_points
// (host_ba.hip), which fills from host arrays, takes the padding from the same struct.
// PointHessian::lastResiduals[2] in one word (BADev::pt_last): byte 0 / 1 = window index of [0 / 1].first (int8, -1 = null), byte 2 / 3 = [0 / 1].second
__host__ __device__ constexpr uint32_t pack_last(int t0, int t1, uint32_t s0, uint32_t s1) {
    return (uint32_t)(uint8_t)(int8_t)t0 | ((uint32_t)(uint8_t)(int8_t)t1 << 8) | (s0 << 16) | (s1 << 24);
}
constexpr uint32_t kLastNone = pack_last(-1, -1, 1u, 1u);   // {null, null} / {OOB, OOB}: a slot without a point, or a point no residual was made for
// The arrays an issue writes: the first set of point / slot buffers as build_point_layout sized them. ng / last are NULL for a window without a history.
struct IssueDev {
    int W, Ppad;
    float4 *geo, *col0, *col1, *w0, *w1; float* prior; uint8_t* flags; int* ng; uint32_t* last;
    float4 *acc, *hcd; float *step, *backup, *relbs, *relbs2; uint8_t* ngood;
    uint8_t* state; float2* energy; float4 *jp0, *jp1, *cpt;          // [W][Ppad]
};
struct IssuePoint {                             // the values of one point; the defaults are the filler of a padding slot
    float4 geo = make_float4(8.f, 8.f, 1.f, 1.f), c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0, w0 = c0, w1 = c0;
    float prior = 0.f; uint8_t flags = 0; int ng = 0; uint32_t last = kLastNone;
};
// One lane writes one slot with plain vector stores; there is no floating-point arithmetic here, so a file built with FMA contraction and one built without mean the same.
__device__ __forceinline__ void issue_store_point(const IssueDev& I, int d, const IssuePoint& p) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    I.geo[d] = p.geo; I.col0[d] = p.c0; I.col1[d] = p.c1; I.w0[d] = p.w0; I.w1[d] = p.w1;
    I.prior[d] = p.prior; I.flags[d] = p.flags;
    if (I.ng) { I.ng[d] = p.ng; I.last[d] = p.last; }
    I.acc[d] = z4; I.hcd[d] = z4; I.step[d] = 0.f; I.backup[d] = 0.f; I.relbs[d] = 0.f; I.relbs2[d] = 0.f; I.ngood[d] = 0;
}
__device__ __forceinline__ void issue_store_row(const IssueDev& I, int t, int d, uint8_t st) {   // state IN, energies zero, resetOOB: what nalo_ba_set_residuals leaves
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const size_t si = (size_t)t * (size_t)I.Ppad + d;
    I.state[si] = st; I.energy[si] = make_float2(0.f, 0.f); I.jp0[si] = z4; I.jp1[si] = z4; I.cpt[si] = z4;
}

// Operands of ba_carry_kernel (kernels_ba_carry.hip): the old window's arrays (o_*), the second set they are gathered into with what is zeroed beside them (I),
// and the pending activation's rows. o_ng / o_last are read only where I.ng is set; imm / a_* are read only where src names a selected point.
struct CarryDev {
    const int* src;                             // [I.Ppad]: old slot, -1 padding, -(k + 2) the k-th selected point
    int trow[16];                               // [I.W]: old residual row, -1 the entering frame
    int Ppad_old, enter;
    const float4 *o_geo, *o_col0, *o_col1, *o_w0, *o_w1; const float* o_prior; const uint8_t *o_flags, *o_state; const int* o_ng; const uint32_t* o_last;
    IssueDev I;
    const float* imm; int immN;                 // the resident immature block ([30][immN], host_api.hip) and its size
    const int* a_sel; const float* a_idepth; const uint8_t* a_in;   // selected indices, idepth_out, res_in [k][I.W] of the pending activation
};
void ba_launch_carry(hipStream_t s, const CarryDev& A, int nblocks);
// Operands of iw_gather_kernel (kernels_init_window.hip): the kept level-0 points of the initialiser gathered into a two-frame window's arrays (I, with a history).
// src[d]: level-0 index or -1 for padding. Every pointer is device memory.
struct InitWindowDev {
    const int* src; int n, w, h;
    const float4* dI; const float *u, *v, *iR; float rescale, prior;
    IssueDev I;
};

// Launchers of kernels_ba.hip and kernels_ba_lin.hip
void ba_launch_sc(hipStream_t s, const BADev& B, int T, int shift, float priorScaleMarg, int margOnly);
void ba_launch_linearize(hipStream_t s, const BADev& B, int mode, int fix, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void ba_launch_reset_oob(hipStream_t s, const BADev& B);
void ba_launch_restore(hipStream_t s, const BADev& B, const float4* geo, const uint8_t* state, const uint8_t* flags, const float* prior, const float* th);
void ba_launch_reduce(hipStream_t s, const BADev& B, const int* host_blk, int NPL, double* acc13, double* misc, double* G, bool top, bool sc,
                      const float* step_partial, int step_blocks, double* step_out, bool with_th, double* pub, double seq, unsigned* ticket);
void ba_launch_resub_step(hipStream_t s, const BADev& B, float stepfacD, float* partial, const XadArg& karg, bool karg_is_x);
int ba_launch_stitch(hipStream_t s, const StitchDev& D, size_t* lds_allowed, bool top, bool sc, double* mapped, int ntail, double seq);
void ba_launch_resub(hipStream_t s, const BADev& B, const XadArg& karg, bool karg_is_x);
void ba_launch_resub_step_gated(hipStream_t s, const BADev& B, float stepfacD, float* partial, const GateArg& gate);
void ba_launch_pull(hipStream_t s, float* dst, const float* src_mapped, int n);
void ba_launch_step(hipStream_t s, const BADev& B, float stepfacD, float* partial, double* out3);
void ba_launch_step_sums(hipStream_t s, const BADev& B, const float* partial, double* out3);
void ba_launch_publish(hipStream_t s, const double* src, double* dst_mapped, int n, double seq, unsigned* ticket);
void ba_launch_th_install(hipStream_t s, const double* tail2, float* th);
void ba_launch_th_tail(hipStream_t s, const float* th, double* tail2);
void ba_launch_energy_th(hipStream_t s, const BADev& B);
void ba_launch_set_th(hipStream_t s, float* dst, const float* th, int W);
void ba_launch_energy_th_step(hipStream_t s, const BADev& B, int step);
void ba_launch_lenergy(hipStream_t s, const BADev& B, double* partial);
void ba_launch_load_backup(hipStream_t s, const BADev& B);
void ba_launch_swgray(hipStream_t s, const BADev& B, const double* Rt, double* partial);
void ba_launch_set_idepth(hipStream_t s, const BADev& B, int mode, int host_sel, double scale);
void ba_launch_trk_ref_gather(hipStream_t s, const BADev& B, const int* kmap, float* out);
void ba_launch_hist_update(hipStream_t s, const BADev& B, int scrub_only);
void ba_launch_hist_remap(hipStream_t s, const BADev& B, int idx);
void ba_launch_flag_points(hipStream_t s, const BADev& B, unsigned frame_mask, uint8_t* decision, float* idepth_hessian, int* counts, int* counts_next);
void ba_launch_remove_flagged(hipStream_t s, const BADev& B);
// residuals that exist per (host row, target row) of the resident slots: out[h * NALO_MAX_WINDOW + t], zero before; out_next (the other buffer) is zeroed for the next call
void ba_launch_pair_count(hipStream_t s, const BADev& B, int* out, int* out_next);

}  // namespace nalo
