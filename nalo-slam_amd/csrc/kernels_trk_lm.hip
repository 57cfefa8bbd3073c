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

__global__ __launch_bounds__(kLmThreads) void trk_lm_kernel(TrkLmParams P) {
    __shared__ float rows[(kLmThreads / 4) * kLmStride];
    __shared__ double sums[64];
    __shared__ double part[kLmThreads / 64][64];
    __shared__ LmState S;
    __shared__ int bar_ok;
    const int tid = threadIdx.x, blk = blockIdx.x, NB = gridDim.x;
    const float lambdaExtrapolationLimit = 0.001f;
    int timed_out = 0;
    if (tid == 0) bar_ok = 1;
    float c_id = 0.f, c_x = 0.f, c_y = 0.f, c_rc = 0.f;   // this lane's point of level cached_lvl (levels that fit one round of the grid)
    int cached_lvl = -1;

    // every block keeps its own copy of the LM state and advances it with the same inputs (the summed partials): the control flow is
    // replicated, not broadcast, which saves a second grid barrier per evaluation
    if (tid == 0) {
        for (int i = 0; i < 12; ++i) S.T[i] = P.T0[i];
        S.aff[0] = P.aff0[0]; S.aff[1] = P.aff0[1];
        for (int i = 0; i < 5; ++i) S.lastRes[i] = NAN;
        S.flow[0] = S.flow[1] = S.flow[2] = 1000;
        S.lvl = P.coarsest; S.it = 0; S.phase = 0; S.next_lvl = -1; S.haveRepeated = P.have_repeated_in; S.good = 1; S.evals = 0; S.done = 0; S.break_pending = 0;
        S.levelCutoffRepeat = 1; S.lambda = 0.01f;
        for (int i = 0; i < NALO_MAX_LEVELS; ++i) S.evals_lvl[i] = 0;
        double T0[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) T0[i] = P.T0[i];
        lm_prepare_eval(S, P, P.coarsest, 1.f, T0, P.aff0[0], P.aff0[1], true);
    }
    __syncthreads();

    // phase 0: first evaluation of a level at the accepted estimate (with the cutoff-repeat loop, :1104-1115)
    // phase 1: evaluation of an LM candidate (:1184)
    for (int guard = 0; guard < 4096; ++guard) {
        if (S.done) break;
        // ------------------------------------------------------------- fused calcRes + calcGS over this level's points
        const TrkLevel& L = P.lv[S.lvl];
        float acc[kTrkVals];
#pragma unroll
        for (int k = 0; k < kTrkVals; ++k) acc[k] = 0.f;
        {
            const float wlm3 = (float)(L.wl - 3), hlm3 = (float)(L.hl - 3);
            const float affa = S.affa, affb = S.affb, b0 = S.b0, cutoff = S.cutoff, maxEnergy = S.maxEnergy;
            const int lvl = S.lvl;
            float RK[9], Kq[9], tt[3];
#pragma unroll
            for (int q = 0; q < 9; ++q) { RK[q] = S.RKi[q]; Kq[q] = S.Ki[q]; }
            tt[0] = S.t[0]; tt[1] = S.t[1]; tt[2] = S.t[2];
            // G = 1 point per lane per round in flight (point loads, then the texel gathers, then the arithmetic); the rounds stride over the grid. Two
            // points per lane measured within +-2 %. The [G] arrays and one-trip g loops stay: written with scalars, the same
            // evaluation compiles to a different instruction schedule
            constexpr int G = 1;
            const int gthreads = NB * kLmThreads;
            // A level whose points fit ONE round of the grid (<= 64 x 512 points) gives each lane one point for all the ~5 evaluations of the level: it is
            // loaded once and stays in four registers, which takes one of the two dependent memory round trips (point -> texels) out of every later
            // evaluation. Not every level of a KITTI-sized cloud does: the headline cloud (8750 inputs) has 41 711 and 36 103 points on levels 0 and 1, two
            // rounds each, the second ragged (18 and 7 of the 64 workgroups); its levels 2 and 3 (21 381 and 6 249 points) fit one round.
            const bool one_round = L.n <= gthreads;
            if (one_round && cached_lvl != lvl) {
                const int i = blk * kLmThreads + tid, ii = i < L.n ? i : 0;
                c_id = L.id[ii]; c_x = L.u[ii]; c_y = L.v[ii]; c_rc = L.col[ii];
                cached_lvl = lvl;
            }
            for (int base = blk * kLmThreads + tid; base < L.n; base += G * gthreads) {
                float id[G], x[G], y[G], rc[G], Ku[G], Kv[G], uu[G], vv[G], nid[G];
                bool inb[G], ok[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int i = base + g * gthreads;
                    inb[g] = i < L.n;
                    const int ii = inb[g] ? i : 0;
                    if (one_round) { id[g] = c_id; x[g] = c_x; y[g] = c_y; rc[g] = c_rc; }
                    else { id[g] = L.id[ii]; x[g] = L.u[ii]; y[g] = L.v[ii]; rc[g] = L.col[ii]; }
                }
                float4 p00[G], p10[G], p01[G], p11[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    trk_project(RK, tt, L, x[g], y[g], id[g], uu[g], vv[g], Ku[g], Kv[g], nid[g]);
                    ok[g] = inb[g] && (Ku[g] > 2.f && Kv[g] > 2.f && Ku[g] < wlm3 && Kv[g] < hlm3 && nid[g] > 0.f);        // :981
                    const int ix = ok[g] ? (int)Ku[g] : 2, iy = ok[g] ? (int)Kv[g] : 2;
                    const float4* bp = L.dI + ix + iy * L.wl;
                    p00[g] = bp[0]; p10[g] = bp[1]; p01[g] = bp[L.wl]; p11[g] = bp[1 + L.wl];
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int i = base + g * gthreads;
                    if (inb[g] && lvl == 0 && (i & 31) == 0) trk_flow(acc, RK, Kq, tt, L, x[g], y[g], id[g], Ku[g], Kv[g]);
                    if (!ok[g]) continue;
                    const float3 hit = trk_interp(Ku[g], Kv[g], p00[g], p10[g], p01[g], p11[g]);
                    if (!isfinite(hit.x)) continue;
                    float hw; const float residual = trk_residual(hit.x, rc[g], affa, affb, hw);
                    acc[kTrkNE] += 1.f;
                    if (fabsf(residual) > cutoff) { acc[kTrkE] += maxEnergy; acc[kTrkNSat] += 1.f; }
                    else {
                        acc[kTrkE] += hw * residual * residual * (2.f - hw);
                        acc[kTrkNWarped] += 1.f;
                        float J[9];
                        trk_jacobian(J, hit, rc[g], uu[g], vv[g], nid[g], L.fx, L.fy, affa, b0, residual);
#pragma unroll
                        for (int r = 0; r < 9; ++r) {
                            const float Jw = J[r] * hw;
#pragma unroll
                            for (int c2 = r; c2 < 9; ++c2) acc[trk_ut(r, c2)] += Jw * J[c2];
                        }
                    }
                }
            }
        }
        // ------------------------------------------------------------- block reduction (same scheme as reduce.h), then the grid sum
        const int nbl = min(NB, (L.n + kLmThreads - 1) / kLmThreads);          // blocks that own points of this level
        if (blk < nbl) {
#pragma unroll
            for (int k = 0; k < kTrkVals; ++k) acc[k] = dpp_quad_sum(acc[k]);
            if ((tid & 3) == 0) {
                float* row = rows + (tid >> 2) * kLmStride;
#pragma unroll
                for (int k = 0; k < kTrkVals; ++k) row[k] = acc[k];
            }
            __syncthreads();
            {                                                // fp64 column sums over the quad rows: (T/64) lane groups x 16 rows, fixed order
                const int j = tid & 63, g = tid >> 6;
                double s = 0;
                if (j < kTrkVals) for (int r = g * 16; r < g * 16 + 16; ++r) s += (double)rows[r * kLmStride + j];
                part[g][j] = s;
            }
            __syncthreads();
            if (tid < kTrkVals) {
                double s = 0; for (int g = 0; g < kLmThreads / 64; ++g) s += part[g][tid];
                if (NB == 1) sums[tid] = s;
                else __hip_atomic_store(&P.partial[((size_t)(S.evals & 1) * NB + blk) * 64 + tid], lm_pack((float)s, P.tag0 + (unsigned)S.evals), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (NB > 1) {                                        // block partials -> every block sums them in the same fixed order
            // the wave's group as a scalar, made here in every evaluation (the empty asm keeps what derives from it - block indices, guards - from being hoisted
            // out of the evaluation loop, where it would be live across the gather, the kernel's register peak)
            const int j = tid & 63;
            int g = __builtin_amdgcn_readfirstlane(tid >> 6);
            asm volatile("" : "+s"(g));
            const unsigned long long* pp = P.partial + (size_t)(S.evals & 1) * NB * 64;
            const unsigned want = P.tag0 + (unsigned)S.evals;
            double s = 0;
            bool pending = j < kTrkVals;
            // a pass loads all words of this lane's blocks back to back and waits once (lm_exchange_pass: 8 words on a grid of <= kLmMaxBlocks workgroups, 16
            // on the double grid); a pass that finds a tag missing is repeated whole until every tag matches
            constexpr int kWords = kLmMaxBlocks / (kLmThreads / 64);
            for (unsigned spins = 0; pending; ++spins) {
                pending = NB <= kLmMaxBlocks ? lm_exchange_pass<kWords>(pp, g, j, nbl, want, s) : lm_exchange_pass<2 * kWords>(pp, g, j, nbl, want, s);
                if (pending) { if (spins > (1u << 21)) { bar_ok = 0; break; } __builtin_amdgcn_s_sleep(1); }
            }
            part[g][j] = s;
            __syncthreads();
            if (!bar_ok) { timed_out = 1; break; }
            if (tid < kTrkVals) { double t2 = 0; for (int g2 = 0; g2 < kLmThreads / 64; ++g2) t2 += part[g2][tid]; sums[tid] = t2; }
        }
        __syncthreads();
        // ------------------------------------------------------------- wave 0 = the host of the reference
        // Scalars of the control flow are computed by every lane of the wave (uniform); the 8x8 solve puts one row per lane; lane 0 writes
        // the state back. Nothing here waits on memory other than a handful of LDS broadcasts.
        if (tid < 64) {
            const int lane = tid;
            int phase = S.phase, it = S.it, lvl = S.lvl, brk = S.break_pending, haveRep = S.haveRepeated, good = S.good, done = 0, next_lvl = S.next_lvl;
            float lambda = S.lambda, lcr = S.levelCutoffRepeat;
            const int evals = S.evals + 1;
            if (lane == 0) S.evals_lvl[S.lvl] += 1;
            // sums (52 doubles) -> stats6 and this lane's entry of the scaled H / b (CoarseTracker.cpp:1040-1046, 869-884)
            const double E = sums[kTrkE], nE = sums[kTrkNE], nSat = sums[kTrkNSat], nW = sums[kTrkNWarped], sT = sums[kTrkST], sRT = sums[kTrkSRT], sN = sums[kTrkSN];
            // (round 4: the three fp64 divisions an evaluation does not need are off wave 0's path - the two flow indicators are divided when a level ends, from the
            // sums kept meanwhile; the accepted estimate's E / nE is kept as a quotient instead of being divided again at every later test; same operands, same bits)
            const double st[6] = {E, nE, sT, sN, sRT, E / nE};
            const double inv = 1.0 / (double)(((long)nW + 3) & ~3L);
            const int hr = lane >> 3, hc = lane & 7, lo = hr < hc ? hr : hc, hi = hr < hc ? hc : hr;
            // trk_ut(lo, hi) and trk_ut(bl, 8) written out: through the function the same index compiles to a different instruction schedule
            const double Hval = sums[lo * 9 - lo * (lo - 1) / 2 + (hi - lo)] * inv * lm_scale(hr) * lm_scale(hc);
            const int bl = lane & 7;
            const double bval = sums[bl * 9 - bl * (bl - 1) / 2 + (8 - bl)] * inv * lm_scale(bl);
            double ro[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) ro[i] = S.resOld[i];
            int next_action;                                 // 0 = evaluate again at the accepted estimate, 1 = propose, 2 = finish level
            bool store_H = false, take_T = false;
            if (phase == 0) {
                store_H = true;
                if ((double)((float)nSat / (float)nE) > 0.6 && lcr < 50) { lcr *= 2; next_action = 0; }   // :1106-1113
                else { lambda = 0.01f; it = 0; brk = 0; next_action = 1; }
            } else {
                const bool accept = st[5] < ro[5];                                               // :1186 (resNew[0] / resNew[1]) < (resOld[0] / resOld[1])
                if (accept) { store_H = true; take_T = true; lambda *= 0.5f; }                   // :1202-1209
                else { lambda *= 4; if (lambda < lambdaExtrapolationLimit) lambda = lambdaExtrapolationLimit; }
                it++;
                next_action = brk ? 2 : 1;                                                       // `if(!(inc.norm() > 1e-3)) break;` (:1216-1221)
            }
            if (store_H) {
                S.H[lane] = Hval;
                if (lane < 8) S.b[lane] = bval;
#pragma unroll
                for (int i = 0; i < 6; ++i) ro[i] = st[i];
            }
            if (take_T) { if (lane < 12) S.T[lane] = S.Tn[lane]; else if (lane < 14) S.aff[lane - 12] = S.affn[lane - 12]; }
            lm_wave_sync();
            double T[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = S.T[i];
            const double aff0 = S.aff[0], aff1 = S.aff[1];
            if (next_action == 1) {
                if (it < lm_max_iterations(lvl)) {                                               // :1133-1184
                    double U[36], rhs[8], iv[8], is[8];
                    const float opl = 1 + lambda;
#pragma unroll
                    for (int r = 0; r < 8; ++r) {                // wave-uniform LDS reads (broadcast): every lane holds the whole system
#pragma unroll
                        for (int cc = r; cc < 8; ++cc) U[lm_ut(r, cc)] = S.H[r * 8 + cc];
                        U[lm_ut(r, r)] *= opl;
                        rhs[r] = -S.b[r];
                    }
                    lm_ldlt8_uniform(U, rhs, iv);
                    float extrapFac = 1;
                    if (lambda < lambdaExtrapolationLimit) extrapFac = sqrtf(sqrtf(lambdaExtrapolationLimit / lambda));
                    // labels swapped vs tangent order in the reference (:1172-1173): entries 0-2 scale with SCALE_XI_ROT, 3-5 with SCALE_XI_TRANS
#pragma unroll
                    for (int i = 0; i < 8; ++i) { iv[i] *= extrapFac; is[i] = iv[i] * (i < 3 ? (double)kScaleXiRot : i < 6 ? (double)kScaleXiTrans : i == 6 ? (double)kScaleA : (double)kScaleB); }
                    double ssum = 0, nrm = 0;
#pragma unroll
                    for (int i = 0; i < 8; ++i) { ssum += is[i]; nrm += iv[i] * iv[i]; }
                    if (!isfinite(ssum)) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) is[i] = 0;
                    }
                    double E12[12], Tn[12];
                    lm_se3_exp(is, E12);
                    lm_se3_mul(E12, T, Tn);
                    const double affn0 = aff0 + is[6], affn1 = aff1 + is[7];
                    brk = !(sqrt(nrm) > 1e-3);
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < 12; ++i) S.Tn[i] = Tn[i];
                        S.affn[0] = affn0; S.affn[1] = affn1;
                    }
                    lm_prepare_eval(S, P, lvl, lcr, Tn, affn0, affn1, lane == 0);
                    phase = 1;
                } else next_action = 2;
            }
            if (next_action == 0) lm_prepare_eval(S, P, lvl, lcr, T, aff0, aff1, lane == 0);
            if (next_action == 2) {                                                              // level finished (:1225-1235)
                const double lr = (double)sqrtf((float)ro[5]);
                if (lane == 0) { S.lastRes[lvl] = lr; S.flow[0] = ro[2] / (ro[3] + 0.1); S.flow[1] = 0; S.flow[2] = ro[4] / (ro[3] + 0.1); }
                if (P.has_minres && lr > 1.5 * P.minRes[lvl]) { good = 0; done = 1; }
                else {
                    int next = lvl - 1;
                    if (lcr > 1 && !haveRep) { next = lvl; haveRep = 1; }                        // repeat this level once
                    if (next < P.stop_lvl) { done = 1; next_lvl = next; }
                    else { lvl = next; lcr = 1; phase = 0; lm_prepare_eval(S, P, lvl, lcr, T, aff0, aff1, lane == 0); }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 6; ++i) S.resOld[i] = ro[i];
                S.phase = phase; S.it = it; S.lvl = lvl; S.break_pending = brk; S.haveRepeated = haveRep; S.good = good; S.next_lvl = next_lvl;
                S.lambda = lambda; S.levelCutoffRepeat = lcr; S.evals = evals; S.done = done;
            }
        }
        __syncthreads();
    }
    if (blk == 0 && tid == 0) {
        double* o = P.out;
        int ok = S.good;
        for (int i = 0; i < 12; ++i) o[i] = S.T[i];
        o[12] = S.aff[0]; o[13] = S.aff[1];
        for (int i = 0; i < 5; ++i) o[14 + i] = S.lastRes[i];
        for (int i = 0; i < 3; ++i) o[19 + i] = S.flow[i];
        if (ok && (fabsf((float)S.aff[0]) > 1.2f || fabsf((float)S.aff[1]) > 200.f)) ok = 2;   // :1243-1245: pose is still written, return false
        if (timed_out) ok = -1;
        for (int i = 0; i < 5; ++i) o[26 + i] = (double)S.evals_lvl[i];
        o[22] = (double)ok; o[23] = (double)S.evals; o[24] = (double)S.next_lvl; o[25] = (double)S.haveRepeated;
        __threadfence_system();
        __hip_atomic_store(&o[31], P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// workgroups of the persistent launch for a largest level of maxn points: one per kLmThreads points, at most kLmMaxBlocks (64) on KITTI-sized clouds (the
// exchange between them is the cost that grows), twice that once the largest level has 8+ rounds of the 64-workgroup grid (8 x 64 x 512 = 262 144 points;
// 1920x1072, 250 k points: 513 us per frame with 64, 469 with 128, 499 with 192, 544 with 256)
int trk_lm_blocks(int maxn) {
    const int max_blocks = (maxn >= 8 * kLmMaxBlocks * kLmThreads ? 2 * kLmMaxBlocks : kLmMaxBlocks);
    return std::min(max_blocks, std::max(1, (maxn + kLmThreads - 1) / kLmThreads));
}

int trk_lm_launch(nalo_ctx* c, int slot_new, const double T0[12], const double aff0[2], const double ref_aff[2], const float exposures[2],
                  int coarsest, int stop_lvl, const double* minRes, double out24[32]) {
    TrkLmParams P;
    std::memset(&P, 0, sizeof(P));
    for (int l = 0; l < c->levels; ++l) P.lv[l] = trk_level(c, slot_new, l);
    std::memcpy(P.T0, T0, sizeof(P.T0)); P.aff0[0] = aff0[0]; P.aff0[1] = aff0[1]; P.ref_aff[0] = ref_aff[0]; P.ref_aff[1] = ref_aff[1];
    P.expRef = exposures[0]; P.expNew = exposures[1]; P.coarsest = coarsest; P.stop_lvl = stop_lvl; P.have_repeated_in = 0;
    P.has_minres = 0;
    if (minRes) { P.has_minres = 1; for (int i = 0; i < 5; ++i) { P.minRes[i] = minRes[i]; } }
    double* const dout = c->trk_out_host.dev;
    P.out = dout + 64;                                   // second half of the mapped buffer (first half: per-eval results)
    P.seq = (double)(++c->trk_seq);
    int maxn = 1;
    for (int l = stop_lvl; l <= coarsest; ++l) maxn = std::max(maxn, c->pc_n[l]);
    const int NB = trk_lm_blocks(maxn);
    c->trk_cfg[0] = kLmThreads; c->trk_cfg[1] = NB; c->trk_cfg[2] = 1;
    for (int l = 0; l < 5; ++l) c->trk_cfg[3 + l] = (l >= stop_lvl && l <= coarsest) ? (c->pc_n[l] + NB * kLmThreads - 1) / (NB * kLmThreads) : 0;
    if (!c->lm_partial.p || (c->lm_launches & 0xFFFFFu) == 0) {      // first use / tag wrap-around: no stale word may carry a live tag
        NALO_HIP(c, c->lm_partial.reserve((size_t)2 * 256 * 64));
        NALO_HIP(c, hipMemsetAsync(c->lm_partial.p, 0, (size_t)2 * 256 * 64 * 8, c->stream));
    }
    P.partial = c->lm_partial.p;
    P.tag0 = (unsigned)((++c->lm_launches & 0xFFFFFu) << 12);
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

}  // namespace nalo
