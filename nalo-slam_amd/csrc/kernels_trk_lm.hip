// Device-resident CoarseTracker::trackNewestCoarse (reference src/FullSystem/CoarseTracker.cpp:1073-1259) for gfx950.
//
// The reference's LM loop does up to ~180 calcRes/calcGSSSE evaluations per frame with an 8x8 solve and an SE3::exp in between. Driven from the host every
// evaluation costs a launch + a completion round trip (~19 us) although the kernels themselves run a few microseconds on a KITTI-sized point cloud: the loop
// is latency bound. Here ONE persistent launch of up to kLmMaxBlocks (64) workgroups of kLmThreads (512) lanes runs the whole pyramid descent, ALL levels:
// every workgroup evaluates its share of the level's points (fused calcRes + calcGS), reduces it (DPP quad adds -> LDS rows -> fp64 column sums) and
// publishes the partial as 8-byte {fp32 value, tag} words (agent-scope atomics: the data is the arrival flag, double-buffered by evaluation parity, bounded
// poll); then EVERY workgroup sums the partials in a fixed order and replays the control flow on its wave 0: 8x8 LDL^T with one matrix row per lane and
// v_readlane broadcasts, SE3::exp, accept / reject, lambda schedule, cutoff repeat, level descent - exactly the control flow of the host mirror in
// host_api.hip (a sharded tracker and the fixed-affine settings run that one). The workgroups must be co-resident (no cooperative launch is
// used: 64 workgroups of 512 lanes fit 256 CUs by a wide margin; a violation - the CUs held by another context's long kernel - ends in the bounded poll, not in
// a hang: the launch returns NALO_LM_LOST_BLOCK and nalo_trk_track redoes the frame with the host-driven loop and keeps to it for this context).
#include "nalo_internal.h"
#include <hip/hip_ext.h>
#include "reduce.h"
#include "trk_device.h"

namespace nalo {

// lanes per workgroup: 512 (one point per lane and round, half as many workgroups as with 256 lanes -> half as many partials to exchange and to
// sum in every workgroup per evaluation). The compiler reports 256 VGPRs with 6 spilled (28 bytes of scratch per lane), 106 SGPRs, 34424 bytes of LDS.
// Headline window, same box, back to back: 256: 696, 384: 708, **512: 717-769**, 768 (spills): 670-678, 1024 (spills): 633-640 keyframes/s.
constexpr int kLmThreads = 512;
constexpr int kLmStride = 56;
constexpr int kLmMaxBlocks = 64;                                     // workgroups of a launch: at most this many, or twice as many (trk_lm_blocks)

struct TrkLmParams {
    TrkLevel lv[NALO_MAX_LEVELS];
    double T0[12], aff0[2], ref_aff[2], minRes[5];
    float expRef, expNew;
    int coarsest, has_minres, stop_lvl, have_repeated_in;   // levels coarsest..stop_lvl run here; the caller continues below
    double* out;                             // host-mapped: T(12) aff(2) lastRes(5) flow(3) ok evals | seq at [31]
    double seq;
    unsigned long long* partial;             // [2][gridDim.x][64] block partials {fp32 value, tag}, double-buffered by evaluation parity
    unsigned tag0;                           // launch sequence << 12: tags of this launch are tag0 + evaluation number
};

// nalo_trk_track_tries: FullSystem::trackNewCoarse's loop over motion hypotheses (FullSystem.cpp:595-666) inside ONE persistent launch. The second kernel
// argument of trk_lm_tries_kernel; the first one describes try 0 (T0 = tries[0], aff0 = aff_init) and what all tries share.
struct TrkLmTries {
    const double* list;                      // host-mapped, n_tries x 12: lastF_2_fh_tries (every workgroup copies it into LDS when it starts)
    double* out;                             // host-mapped: summary (32 doubles, seq at [31]) | n_tries records of kLmRecDoubles
    double thr;                              // lastCoarseRMSE[0] * (double)setting_reTrackThreshold (:653)
    int n_tries, a_free, b_free;             // setting_affineOptModeA / B != 0 (:1243-1250; a fixed parameter, < 0, never runs here)
    unsigned launch0;                        // try i publishes under launch number launch0 + i: tags ((launch0 + i) & 0xFFFFF) << 12 | evaluation of the try
};
struct LmTriesState {                        // lives in LDS beside LmState, same rules
    double ach[5];                           // achievedRes (:595)
    double T[12], aff[2], flow[3];           // the winner so far; tries[0], aff_init, 0 while there is none (:658-664)
    int cur, have, winner, par;              // try running, haveOneGood, its index, parity of the next evaluation's slots (alternates ACROSS tries)
    unsigned tag0;                           // tag base of the try running
    int evals_lvl[NALO_MAX_LEVELS];          // evaluations per level, summed over the tries
};

struct LmState {                             // lives in LDS; written by lane 0 only, read by everyone after a barrier
    double T[12], aff[2];                    // accepted estimate
    double Tn[12], affn[2];                  // candidate
    double H[64], b[8], resOld[6], resNew[6];
    double lastRes[5], flow[3];
    float RKi[9], t[3], Ki[9], affa, affb, b0, cutoff, maxEnergy;
    float lambda, levelCutoffRepeat;
    int lvl, it, phase, haveRepeated, good, evals, done, break_pending, next_lvl;
    int evals_lvl[NALO_MAX_LEVELS];          // evaluations per pyramid level (the algorithmic bytes of the launch: sum_l evals_l n_l 64 B)
};

// ---- fp64 helpers for lane 0 -------------------------------------------------------------------------------------------
// The LM increments of the tracker are small rotations (|omega| of a few 1e-2 at most): below 0.5 rad every trigonometric factor of the exponential is an
// even power series in theta (theta^2 = |omega|^2), evaluated by Horner in fp64 with truncation error < 1e-20 - no sqrt, no sincos, no division on
// the serial path wave 0 walks between two evaluations (the general branch keeps the closed forms).
__device__ __forceinline__ void lm_se3_exp(const double (&xi)[8], double (&T)[12]) {   // Sophus SE3::exp (se3.hpp:407-428), quaternion form
    const double wx = xi[3], wy = xi[4], wz = xi[5];
    const double th2 = wx * wx + wy * wy + wz * wz;
    double qi, qr, a, bq;                      // qi = sin(th/2)/th, qr = cos(th/2), a = (1 - cos th)/th^2, bq = (th - sin th)/th^3
    if (th2 < 0.25) {
        const double u = 0.25 * th2;           // (th/2)^2
        // sin(x)/x and cos(x) in u = x^2, x = th/2 <= 0.25: 9 terms each (next term < 1e-25)
        double sc = -1.0 / 121645100408832000.0, cc = 1.0 / 6402373705728000.0;
        sc = sc * u + 1.0 / 355687428096000.0; cc = cc * u - 1.0 / 20922789888000.0;
        sc = sc * u - 1.0 / 1307674368000.0;   cc = cc * u + 1.0 / 87178291200.0;
        sc = sc * u + 1.0 / 6227020800.0;      cc = cc * u - 1.0 / 479001600.0;
        sc = sc * u - 1.0 / 39916800.0;        cc = cc * u + 1.0 / 3628800.0;
        sc = sc * u + 1.0 / 362880.0;          cc = cc * u - 1.0 / 40320.0;
        sc = sc * u - 1.0 / 5040.0;            cc = cc * u + 1.0 / 720.0;
        sc = sc * u + 1.0 / 120.0;             cc = cc * u - 1.0 / 24.0;
        sc = sc * u - 1.0 / 6.0;               cc = cc * u + 0.5;
        sc = sc * u + 1.0;                     cc = 1.0 - cc * u;
        qi = 0.5 * sc; qr = cc;
        // (1 - cos th)/th^2 and (th - sin th)/th^3 in v = th^2 <= 0.25: 10 terms each (next term < 1e-21)
        const double v = th2;
        double pa = -1.0 / 51090942171709440000.0, pb = 1.0 / 1124000727777607680000.0;
        pa = pa * v + 1.0 / 121645100408832000.0; pb = pb * v - 1.0 / 2432902008176640000.0;
        pa = pa * v - 1.0 / 355687428096000.0;    pb = pb * v + 1.0 / 6402373705728000.0;
        pa = pa * v + 1.0 / 1307674368000.0;      pb = pb * v - 1.0 / 20922789888000.0;
        pa = pa * v - 1.0 / 6227020800.0;         pb = pb * v + 1.0 / 87178291200.0;
        pa = pa * v + 1.0 / 39916800.0;           pb = pb * v - 1.0 / 479001600.0;
        pa = pa * v - 1.0 / 362880.0;             pb = pb * v + 1.0 / 3628800.0;
        pa = pa * v + 1.0 / 5040.0;               pb = pb * v - 1.0 / 40320.0;
        pa = pa * v - 1.0 / 120.0;                pb = pb * v + 1.0 / 720.0;
        pa = pa * v + 1.0 / 6.0;                  pb = pb * v - 1.0 / 24.0;
        bq = pa; a = pb * v + 0.5;
    } else {
        const double th = sqrt(th2);
        double sh, ch;
        sincos(0.5 * th, &sh, &ch);
        qi = sh / th; qr = ch;
        // 1 - cos(th) = 2 sin^2(th/2), sin(th) = 2 sin(th/2) cos(th/2): one sincos for the whole exponential
        a = (2.0 * sh * sh) / th2; bq = (th - 2.0 * sh * ch) / (th2 * th);
    }
    double q[4] = {qr, qi * wx, qi * wy, qi * wz};
    // SO3's constructor normalises the quaternion: |q|^2 = 1 + e with |e| ~ 1e-16, so 1/|q| is one Newton step of the reciprocal square root at 1
    const double qn2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const double qs = 1.5 - 0.5 * qn2;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] *= qs;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    const double O[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double O2[9], V[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * O[i] + bq * O2[i];      // theta -> 0: a -> 1/2, bq -> 1/6 (Sophus switches to V = R below 1e-10: a 1e-20 difference)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[i * 4 + j] = R[i * 3 + j];
        T[i * 4 + 3] = V[i * 3] * xi[0] + V[i * 3 + 1] * xi[1] + V[i * 3 + 2] * xi[2];
    }
}
__device__ __forceinline__ void lm_se3_mul(const double (&A)[12], const double (&B)[12], double (&C)[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i * 4 + j] = A[i * 4] * B[j] + A[i * 4 + 1] * B[4 + j] + A[i * 4 + 2] * B[8 + j];
        C[i * 4 + 3] = A[i * 4] * B[3] + A[i * 4 + 1] * B[7] + A[i * 4 + 2] * B[11] + A[i * 4 + 3];
    }
}
// ---- wave-level helpers: the serial part of an LM iteration runs on wave 0, uniform scalars computed redundantly by every lane
__device__ __forceinline__ double lm_bcast(double v, int srclane) {              // srclane is wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane), hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void lm_wave_sync() {                                  // LDS written by one lane, read by another lane of the same wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// 8x8 symmetric solve, computed REDUNDANTLY by every lane of wave 0 on registers: U = upper triangle of H with the damped diagonal (row-major, 36 entries,
// wave-uniform values), x = solution of U x = rhs. LDL^T without pivoting: the LM system H + lambda diag(H) is positive definite, and a zero / non-finite
// pivot zeroes its column and its unknown exactly like the host's pivoted variant does for an empty system. No cross-lane traffic at all: the first version
// kept one matrix row per lane and moved pivot rows and unknowns through v_readlane (72 + 60 of them, each a VALU -> SGPR round trip on the one wave
// that everybody waits for: ~2500 of the ~6000 clocks between two evaluations); here the same n^3/6 multiply-adds are plain fp64 FMAs with their
// natural instruction-level parallelism. 1/d by v_rcp_f64 + two Newton steps (full fp64 accuracy; half the length of the IEEE division sequence).
__device__ __forceinline__ constexpr int lm_ut(int r, int c) { return r * 8 - r * (r - 1) / 2 + (c - r); }      // index of (r, c), r <= c, in the packed upper triangle
__device__ __forceinline__ void lm_ldlt8_uniform(double (&U)[36], const double (&rhs)[8], double (&x)[8]) {
    double dinv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double d = U[lm_ut(k, k)];
        const bool ok = d != 0.0 && isfinite(d);
        double rd = __builtin_amdgcn_rcp(d);
        rd = rd * (2.0 - d * rd); rd = rd * (2.0 - d * rd);
        dinv[k] = ok ? rd : 0.0;
#pragma unroll
        for (int i = k + 1; i < 8; ++i) {
            const double l = U[lm_ut(k, i)] * dinv[k];           // L[i][k]
#pragma unroll
            for (int j = i; j < 8; ++j) U[lm_ut(i, j)] -= l * U[lm_ut(k, j)];
            U[lm_ut(k, i)] = l;                                  // L^T overwrites the strict upper triangle
        }
    }
    double y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {                                // L y = rhs
        double sacc = rhs[i];
#pragma unroll
        for (int j = 0; j < i; ++j) sacc -= U[lm_ut(j, i)] * y[j];
        y[i] = sacc;
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {                               // D z = y, L^T x = z
        double sacc = y[i] * dinv[i];
#pragma unroll
        for (int j = i + 1; j < 8; ++j) sacc -= U[lm_ut(i, j)] * x[j];
        x[i] = sacc;
    }
}

// prepare the float parameters of an evaluation at (T, aff) for level lvl (CoarseTracker.cpp:907-916); the caller's lane 0 passes write = true
__device__ __forceinline__ void lm_prepare_eval(LmState& S, const TrkLmParams& P, int lvl, float levelCutoffRepeat, const double (&T)[12], double aff0, double aff1, bool write) {
    const TrkLevel& L = P.lv[lvl];
    float expF = P.expRef, expT = P.expNew;
    if (expF == 0 || expT == 0) expT = expF = 1;                                        // AffLight::fromToVecExposure, util/NumType.h:173-185
    const double a = exp(aff0 - P.ref_aff[0]) * expT / expF, bq = aff1 - a * P.ref_aff[1];
    const float Ki[9] = {1.0f / L.fx, 0, -L.cx / L.fx, 0, 1.0f / L.fy, -L.cy / L.fy, 0, 0, 1};
    float Rf[9], RKi[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rf[i * 3 + j] = (float)T[i * 4 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) RKi[i * 3 + j] = Rf[i * 3] * Ki[j] + Rf[i * 3 + 1] * Ki[3 + j] + Rf[i * 3 + 2] * Ki[6 + j];
    if (!write) return;
    S.affa = (float)a; S.affb = (float)bq; S.b0 = (float)P.ref_aff[1];
#pragma unroll
    for (int i = 0; i < 9; ++i) { S.RKi[i] = RKi[i]; S.Ki[i] = Ki[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) S.t[i] = (float)T[i * 4 + 3];
    S.cutoff = kCoarseCutoffTH * levelCutoffRepeat;
    S.maxEnergy = 2 * kHuberTH * S.cutoff - kHuberTH * kHuberTH;
}
__device__ __forceinline__ double lm_scale(int r) { return r < 3 ? (double)kScaleXiRot : r < 6 ? (double)kScaleXiTrans : r == 6 ? (double)kScaleA : (double)kScaleB; }
__device__ __forceinline__ int lm_max_iterations(int lvl) { return lvl == 0 ? 10 : lvl == 1 ? 20 : 50; }      // maxIterations[] (:1085)
// Exchange of the block partials between the workgroups of the persistent LM kernel: every value travels as ONE 8-byte word
// {fp32 partial, 32-bit tag} stored with an agent-scope atomic (write-through past the XCD's L2), the tag = launch sequence and
// evaluation number. A reader polls the words of the blocks it sums until their tags match: the data IS the arrival flag, so there is no
// counter, no fence and no second round trip (the scheme of low-latency collective protocols). Slots are double-buffered by evaluation
// parity: a block can run at most one evaluation ahead of the slowest reader, because the next one needs that reader's own partial.
// The grid is small (<= 2 kLmMaxBlocks workgroups, far below the 256 CUs) so all blocks are co-resident; the poll is bounded anyway, a
// lost block ends the kernel with an error instead of hanging the device.
__device__ __forceinline__ unsigned long long lm_pack(float v, unsigned tag) { return ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v); }
// Entries I, I + 1, ... < cnt of a pass: tag test and sum, in order. cnt is wave-uniform: nested scalar branches (an unrolled loop with a break compiles back
// into a loop that indexes the registers), each waiting only for the loads up to its own entry.
template <int I, int N>
__device__ __forceinline__ void lm_exchange_sum(const unsigned long long (&w)[N], int cnt, unsigned want, bool& pending, double& s) {
    if constexpr (I < N) {
        if (I < cnt) {
            pending |= (unsigned)(w[I] >> 32) != want;
            s += (double)__uint_as_float((unsigned)w[I]);
            lm_exchange_sum<I + 1, N>(w, cnt, want, pending, s);
        }
    }
}
// One pass of a reader lane over column j of the blocks its wave group sums (g, g + 8, ... < nbl, at most N of them): all N words are loaded before any of
// them is looked at, so the pass costs one memory round trip instead of one per block. The index is clamped rather than the load guarded: with a guard per
// entry, even a wave-uniform one, the compiler branches around every load and waits for each. An entry past nbl re-reads a block that exists and is ignored.
// Returns whether a tag is still missing; s = 0 + block g + block g + 8 + ..., each the (double) of its fp32 payload, in that order.
template <int N>
__device__ __forceinline__ bool lm_exchange_pass(const unsigned long long* pp, int g, int j, int nbl, unsigned want, double& s) {
    unsigned long long w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int b2 = max(min(g + i * (kLmThreads / 64), nbl - 1), 0);
        w[i] = __hip_atomic_load(&pp[(size_t)b2 * 64 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int cnt = nbl > g ? (nbl - g + kLmThreads / 64 - 1) / (kLmThreads / 64) : 0;             // this group's blocks are the first cnt entries
    asm volatile("" : "+s"(cnt));                           // compared per pass (a scalar compare and branch per entry), not kept as N lane masks across the poll
    bool pending = false;
    s = 0;
    lm_exchange_sum<0, N>(w, cnt, want, pending, s);
    return pending;
}

// "try finished" of the hypothesis loop, on wave 0 of every workgroup (replicated like the LM control flow; every lane computes the uniform scalars, lane 0
// writes the state, workgroup 0 writes the try's record): the try's verdict with trackNewestCoarse's tail (CoarseTracker.cpp:1239-1256), the take-over rule
// (FullSystem.cpp:633-640), achievedRes (:643-650), the early-out (:653); then either S.done stays set or the state is that of try cur + 1 before its first evaluation.
__device__ __forceinline__ void lm_try_finished(LmState& S, LmTriesState& X, const TrkLmParams& P, const TrkLmTries& Q, const double* list, int lane, bool publish) {
    const int i = X.cur, good = S.good;
    double T[12], aff[2], lr[5], fl[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = good ? S.T[k] : list[i * 12 + k];           // aborted (:1227): the try wrote nothing, the record shows its input
    aff[0] = good ? S.aff[0] : P.aff0[0]; aff[1] = good ? S.aff[1] : P.aff0[1];
#pragma unroll
    for (int k = 0; k < 5; ++k) lr[k] = S.lastRes[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) fl[k] = S.flow[k];
    int ok = good;
    if (good) {                                                                      // :1243-1251 (the zeroing of a fixed parameter, :1255-1256, belongs to the host-driven loop)
        bool fine = !((Q.a_free && fabsf((float)aff[0]) > 1.2f) || (Q.b_free && fabsf((float)aff[1]) > 200.f));
        float expF = P.expRef, expT = P.expNew;
        if (expF == 0 || expT == 0) expT = expF = 1;
        const double ra = exp(aff[0] - P.ref_aff[0]) * expT / expF, rb = aff[1] - ra * P.ref_aff[1];
        if ((!Q.a_free && fabsf(logf((float)ra)) > 1.5f) || (!Q.b_free && fabsf((float)rb) > 200.f)) fine = false;
        ok = fine;
    }
    const bool taken = ok && isfinite((float)lr[0]) && !(lr[0] >= X.ach[0]);        // :633
    const int have = X.have | (taken ? 1 : 0);
    double ach[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {                                                    // :643-650
        double a = X.ach[k];
        if (have && (!isfinite((float)a) || a > lr[k])) a = lr[k];
        ach[k] = a;
    }
    const bool last = (have && ach[0] < Q.thr) || i + 1 >= Q.n_tries;               // :653
    if (publish && lane == 0) {
        double* r = Q.out + 32 + (size_t)i * kLmRecDoubles;
        r[0] = (double)ok; r[1] = taken ? 1.0 : 0.0; r[2] = good ? -1.0 : (double)S.lvl; r[3] = (double)S.haveRepeated; r[4] = (double)S.evals;
        for (int k = 0; k < 5; ++k) r[5 + k] = lr[k];
        for (int k = 0; k < 3; ++k) r[10 + k] = fl[k];
        for (int k = 0; k < 12; ++k) r[13 + k] = T[k];
        r[25] = aff[0]; r[26] = aff[1];
        for (int k = 0; k < 5; ++k) r[27 + k] = (double)S.evals_lvl[k];
    }
    double Tn[12];
    const int nx = last ? i : i + 1;
#pragma unroll
    for (int k = 0; k < 12; ++k) Tn[k] = list[nx * 12 + k];
    if (lane == 0) {
        for (int k = 0; k < 5; ++k) X.ach[k] = ach[k];
        X.have = have;
        if (taken) {
            for (int k = 0; k < 12; ++k) X.T[k] = T[k];
            X.aff[0] = aff[0]; X.aff[1] = aff[1];
            for (int k = 0; k < 3; ++k) X.flow[k] = fl[k];
            X.winner = i;
        }
        for (int k = 0; k < NALO_MAX_LEVELS; ++k) X.evals_lvl[k] += S.evals_lvl[k];
        X.cur = i + 1;
        if (!last) {                                                                 // try i + 1 starts as a launch of its own would (the kernel's prologue)
            X.tag0 = ((Q.launch0 + (unsigned)(i + 1)) & 0xFFFFFu) << 12;
            for (int k = 0; k < 12; ++k) S.T[k] = Tn[k];
            S.aff[0] = P.aff0[0]; S.aff[1] = P.aff0[1];
            for (int k = 0; k < 5; ++k) S.lastRes[k] = NAN;
            S.flow[0] = S.flow[1] = S.flow[2] = 1000;
            S.lvl = P.coarsest; S.it = 0; S.phase = 0; S.next_lvl = -1; S.haveRepeated = 0; S.good = 1; S.evals = 0; S.done = 0; S.break_pending = 0;
            S.levelCutoffRepeat = 1; S.lambda = 0.01f;
            for (int k = 0; k < NALO_MAX_LEVELS; ++k) S.evals_lvl[k] = 0;
        }
    }
    if (!last) lm_prepare_eval(S, P, P.coarsest, 1.f, Tn, P.aff0[0], P.aff0[1], lane == 0);
}

__global__ __launch_bounds__(kLmThreads) void trk_lm_kernel(TrkLmParams P) {
    constexpr bool kTries = false;
    constexpr LmTriesState* Xp = nullptr;
    constexpr double* list = nullptr;
    const TrkLmTries Q = {};
#include "trk_lm_body.h"
}
__global__ __launch_bounds__(kLmThreads) void trk_lm_tries_kernel(TrkLmParams P, TrkLmTries Q) {
    constexpr bool kTries = true;
    __shared__ LmTriesState Xs;
    __shared__ double list[NALO_TRK_MAX_TRIES * 12];
    LmTriesState* const Xp = &Xs;
#include "trk_lm_body.h"
}

// workgroups of the persistent launch for a largest level of maxn points: one per kLmThreads points, at most kLmMaxBlocks (64) on KITTI-sized clouds (the
// exchange between them is the cost that grows), twice that once the largest level has 8+ rounds of the 64-workgroup grid (8 x 64 x 512 = 262 144 points;
// 1920x1072, 250 k points: 513 us per frame with 64, 469 with 128, 499 with 192, 544 with 256)
int trk_lm_blocks(int maxn) {
    const int max_blocks = (maxn >= 8 * kLmMaxBlocks * kLmThreads ? 2 * kLmMaxBlocks : kLmMaxBlocks);
    return std::min(max_blocks, std::max(1, (maxn + kLmThreads - 1) / kLmThreads));
}

// What both launches share: the levels, the frame-wide inputs, the grid (it depends only on the clouds, so every try of a list runs on the same NB and
// sums its partials in the same grouping as a launch of its own), the launch configuration for nalo_trk_get_launch_config.
static int lm_params(nalo_ctx* c, int slot_new, const double T0[12], const double aff0[2], const double ref_aff[2], const float exposures[2], int coarsest, int stop_lvl,
                     TrkLmParams& P) {
    std::memset(&P, 0, sizeof(P));
    for (int l = 0; l < c->levels; ++l) P.lv[l] = trk_level(c, slot_new, l);
    std::memcpy(P.T0, T0, sizeof(P.T0)); P.aff0[0] = aff0[0]; P.aff0[1] = aff0[1]; P.ref_aff[0] = ref_aff[0]; P.ref_aff[1] = ref_aff[1];
    P.expRef = exposures[0]; P.expNew = exposures[1]; P.coarsest = coarsest; P.stop_lvl = stop_lvl; P.have_repeated_in = 0;
    P.has_minres = 0;
    int maxn = 1;
    for (int l = stop_lvl; l <= coarsest; ++l) maxn = std::max(maxn, c->pc_n[l]);
    const int NB = trk_lm_blocks(maxn);
    c->trk_cfg[0] = kLmThreads; c->trk_cfg[1] = NB; c->trk_cfg[2] = 1;
    for (int l = 0; l < 5; ++l) c->trk_cfg[3 + l] = (l >= stop_lvl && l <= coarsest) ? (c->pc_n[l] + NB * kLmThreads - 1) / (NB * kLmThreads) : 0;
    return NB;
}
// n consecutive launch numbers (20 bits of a tag; an evaluation number fills the 12 below). The partials buffer is zeroed on first use and whenever the
// reservation would reach or cross the wrap of the 20 bits; the count then moves to the next multiple of 2^20, so launch number 0 - the tag of a zeroed word
// - is never handed out and no number is handed out twice between two memsets. *first = the first number of the reservation.
static int lm_reserve_tags(nalo_ctx* c, unsigned n, unsigned* first) {
    const unsigned long long low = c->lm_launches & 0xFFFFFu;
    if (!c->lm_partial.p || low == 0 || low + n > 0xFFFFFu) {
        NALO_HIP(c, c->lm_partial.reserve((size_t)2 * 256 * 64));
        NALO_HIP(c, hipMemsetAsync(c->lm_partial.p, 0, (size_t)2 * 256 * 64 * 8, c->stream));
        c->lm_launches = (c->lm_launches + 0xFFFFFu) & ~0xFFFFFull;
    }
    *first = (unsigned)((c->lm_launches + 1) & 0xFFFFFu);
    c->lm_launches += n;
    return NALO_OK;
}

int trk_lm_launch(nalo_ctx* c, int slot_new, const double T0[12], const double aff0[2], const double ref_aff[2], const float exposures[2],
                  int coarsest, int stop_lvl, const double* minRes, double out24[32]) {
    TrkLmParams P;
    const int NB = lm_params(c, slot_new, T0, aff0, ref_aff, exposures, coarsest, stop_lvl, P);
    if (minRes) { P.has_minres = 1; for (int i = 0; i < 5; ++i) { P.minRes[i] = minRes[i]; } }
    double* const dout = c->trk_out_host.dev;
    P.out = dout + 64;                                   // second half of the mapped buffer (first half: per-eval results)
    P.seq = (double)(++c->trk_seq);
    unsigned launch;
    { const int rc = lm_reserve_tags(c, 1, &launch); if (rc) return rc; }      // first use / tag wrap-around: no stale word may carry a live tag
    P.partial = c->lm_partial.p;
    P.tag0 = launch << 12;
    {
        ProfScope ps(c, "trk_lm", true);                  // dispatch-attached timestamps: no barrier packets around the one launch of a tracked frame
        if (ps.a) hipExtLaunchKernelGGL(trk_lm_kernel, dim3(NB), dim3(kLmThreads), 0, c->stream, ps.a, ps.b, 0, P);
        else trk_lm_kernel<<<NB, kLmThreads, 0, c->stream>>>(P);
    }
    NALO_HIP(c, hipGetLastError());
    if (!poll_flag(c, &c->trk_out_host.p[64 + 31], P.seq)) return NALO_ERR_HIP;
    std::memcpy(out24, c->trk_out_host.p + 64, sizeof(double) * 26);
    for (int i = 0; i < 5; ++i) c->lm_evals_lvl[i] = (int)c->trk_out_host.p[64 + 26 + i];
    c->trk_cfg[8] = out24[25] != 0.0;
    if (out24[22] < 0) return NALO_LM_LOST_BLOCK;
    if (c->inject_lm_lost_block > 0 && --c->inject_lm_lost_block == 0) return NALO_LM_LOST_BLOCK;   // nalo_test_inject: the caller's degraded path
    return NALO_OK;
}

// The whole list of nalo_trk_track_tries in one persistent launch. summary: T(12) aff(2) achievedRes(5) flow(3) status have_one_good tries_run winner | evals per
// level summed over the tries (5); records: tries_run x kLmRecDoubles as lm_try_finished wrote them. The list and the outputs live in one host-mapped block:
// the host fills the list before the launch (visible to the kernel when it starts), the kernel's release store of seq publishes the rest.
int trk_lm_tries_launch(nalo_ctx* c, int slot_new, const double* tries, int n_tries, const double aff_init[2], const double ref_aff[2], const float exposures[2],
                        int coarsest, double thr, double summary[32], double* records) {
    constexpr size_t kOut = 32 + (size_t)NALO_TRK_MAX_TRIES * kLmRecDoubles;
    NALO_HIP(c, c->lm_tries_host.reserve(kOut + (size_t)NALO_TRK_MAX_TRIES * 12, hipHostMallocMapped));
    TrkLmParams P;
    const int NB = lm_params(c, slot_new, tries, aff_init, ref_aff, exposures, coarsest, 0, P);
    P.seq = (double)(++c->trk_seq);
    TrkLmTries Q;
    std::memset(&Q, 0, sizeof(Q));
    std::memcpy(c->lm_tries_host.p + kOut, tries, sizeof(double) * 12 * (size_t)n_tries);
    Q.list = c->lm_tries_host.dev + kOut; Q.out = c->lm_tries_host.dev; Q.thr = thr; Q.n_tries = n_tries;
    Q.a_free = c->set.affineOptModeA != 0; Q.b_free = c->set.affineOptModeB != 0;
    { const int rc = lm_reserve_tags(c, (unsigned)n_tries, &Q.launch0); if (rc) return rc; }      // one launch number per try: each try counts its evaluations from 0
    P.partial = c->lm_partial.p;
    {
        ProfScope ps(c, "trk_lm_tries", true);
        if (ps.a) hipExtLaunchKernelGGL(trk_lm_tries_kernel, dim3(NB), dim3(kLmThreads), 0, c->stream, ps.a, ps.b, 0, P, Q);
        else trk_lm_tries_kernel<<<NB, kLmThreads, 0, c->stream>>>(P, Q);
    }
    NALO_HIP(c, hipGetLastError());
    // poll_flag gives a single descent 10 s; this launch is legitimately up to n_tries descents long
    if (!poll_flag(c, &c->lm_tries_host.p[31], P.seq, 10.0 * n_tries)) return NALO_ERR_HIP;
    std::memcpy(summary, c->lm_tries_host.p, sizeof(double) * 32);
    if (summary[22] < 0) return NALO_LM_LOST_BLOCK;
    if (c->inject_lm_lost_block > 0 && --c->inject_lm_lost_block == 0) return NALO_LM_LOST_BLOCK;
    const int run = (int)summary[24];
    std::memcpy(records, c->lm_tries_host.p + 32, sizeof(double) * kLmRecDoubles * (size_t)run);
    for (int i = 0; i < 5; ++i) c->lm_evals_lvl[i] = (int)summary[26 + i];
    c->trk_cfg[8] = run > 0 && records[(size_t)(run - 1) * kLmRecDoubles + 3] != 0.0;
    return NALO_OK;
}

}  // namespace nalo
