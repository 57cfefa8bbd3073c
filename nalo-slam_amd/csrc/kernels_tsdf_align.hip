// nalo_tsdf_align_eval's kernel (include/nalo_gpu.h, "The alignment"): one lane per VISITED pixel of the depth plane takes the field's value and central
// difference at the pixel's world point (seven trilinear samples through the ray-cast's tsdf_rc_field) and forms its row of the Gauss-Newton system. Built
// WITHOUT FMA contraction: every float expression below is the header's definition, one rounding per operation. As in the ray-cast a wave is an 8 x 8 tile (of
// visited pixels), so its lanes' samples share lines; a workgroup is 16 x 16.
// The 37 sums are double, every term an exact product of two floats. A lane never holds all 37: the terms are formed a row of H at a time (at most eight
// doubles live), reduced over the wave with shuffles in a fixed order and left in LDS by lane 0; the four waves are added in wave order into the workgroup's
// partial record, and the workgroup that draws the last ticket adds the records in workgroup order and publishes the result to host-mapped memory. No float or
// double atomic: the same bytes on every run of the same launch configuration.
#include "nalo_internal.h"
#include "tsdf_device.h"

namespace nalo {

constexpr int kAlignNT = 256;
constexpr int kAlignStage = 96;                                                 // records the last workgroup stages in LDS at a time: 96 x 320 B = 30 KB, 15 loads a lane in flight
static_assert(kAlignStage * kTsdfAlignStride % kAlignNT == 0, "whole rounds of one load per lane");

__device__ __forceinline__ double align_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    return v;                                                                   // lane 0 holds the sum
}

// row I of the system: H[I][I..6] and b[I], reduced over the wave; lane 0 leaves them in `row` (the wave's 37 doubles in LDS)
template <int I>
__device__ __forceinline__ void align_row(const float (&J)[7], const float (&Jw)[7], float r, int lane, double* row) {
    constexpr int base = I * 7 - I * (I - 1) / 2;                               // the index of H[I][I] in the row-major upper triangle
#pragma unroll
    for (int j = I; j < 7; ++j) {
        const double s = align_wave_sum((double)Jw[I] * (double)J[j]);
        if (lane == 0) row[base + j - I] = s;
    }
    const double s = align_wave_sum((double)Jw[I] * (double)r);
    if (lane == 0) row[28 + I] = s;
}

__global__ __launch_bounds__(kAlignNT) void tsdf_align_kernel(TsdfAlignDev P, int gx) {
    __shared__ double wsum[4][kTsdfAlignSums];
    __shared__ unsigned wcnt[4][4];
    __shared__ bool is_last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bx = (int)(blockIdx.x % (unsigned)gx), by = (int)(blockIdx.x / (unsigned)gx);
    const int iu = bx * 16 + (wv & 1) * 8 + (lane & 7), iv = by * 16 + (wv >> 1) * 8 + (lane >> 3);      // the pixel's number among the visited ones
    const bool in_view = iu < P.vw && iv < P.vh;     // a lane without a pixel loads nothing; it still takes part in the ballots and the reductions
    int state = -1;
    float r = 0.0f, hw = 0.0f, J[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int u = 0, v = 0;
    if (in_view) {
        u = iu * P.step; v = iv * P.step;                                       // iu < vw = ceil(w / step): u <= w - 1
        const float D = *reinterpret_cast<const float*>(P.depth + (long long)v * P.sy + (long long)u * P.sx);
        state = 1;
        if (D >= P.min_depth && D <= P.max_depth) {                            // a NaN fails
            const float rx = ((float)u - P.cx) / P.fx, ry = ((float)v - P.cy) / P.fy;
            const float pc[3] = {rx * D, ry * D, D};
            float pw[3], q[3], S = 0.0f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                pw[a] = ((P.M[4 * a] * pc[0] + P.M[4 * a + 1] * pc[1]) + P.M[4 * a + 2] * pc[2]) + P.M[4 * a + 3];
                q[a] = ((pw[a] - P.g.origin[a]) / P.g.vs) - 0.5f;
            }
            state = 2;
            if (tsdf_rc_field<true>(P.g, P.min_weight, P.g.tsdf, q[0], q[1], q[2], S)) {
                float G[3];
                bool all = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float qp[3] = {q[0], q[1], q[2]}, qm[3] = {q[0], q[1], q[2]}, sp = 0.0f, sm = 0.0f;
                    qp[a] = q[a] + 1.0f; qm[a] = q[a] - 1.0f;
                    const bool okp = tsdf_rc_field<true>(P.g, P.min_weight, P.g.tsdf, qp[0], qp[1], qp[2], sp);
                    const bool okm = tsdf_rc_field<true>(P.g, P.min_weight, P.g.tsdf, qm[0], qm[1], qm[2], sm);
                    all = all && okp && okm;
                    G[a] = sp - sm;
                }
                state = 3;
                if (all) {
                    state = 0;
                    r = S;
                    const float k = 0.5f / P.g.vs;
                    const float g[3] = {G[0] * k, G[1] * k, G[2] * k};
                    J[0] = g[0]; J[1] = g[1]; J[2] = g[2];
                    J[3] = pw[1] * g[2] - pw[2] * g[1];
                    J[4] = pw[2] * g[0] - pw[0] * g[2];
                    J[5] = pw[0] * g[1] - pw[1] * g[0];
                    if (P.dof == 7) J[6] = (g[0] * (pw[0] - P.M[3]) + g[1] * (pw[1] - P.M[7])) + g[2] * (pw[2] - P.M[11]);
                    hw = fabsf(r) <= P.huber ? 1.0f : P.huber / fabsf(r);
                }
            }
        }
        if (P.records) {
            float* rec = P.records + ((size_t)v * P.w + u) * 10;
            rec[0] = r; rec[1] = hw;
#pragma unroll
            for (int i = 0; i < 7; ++i) rec[2 + i] = J[i];
            rec[9] = (float)state;
        }
    }
    float Jw[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) Jw[i] = hw * J[i];                             // a lane that is not used holds zeros: its terms are +0.0
    double* row = wsum[wv];
    align_row<0>(J, Jw, r, lane, row); align_row<1>(J, Jw, r, lane, row); align_row<2>(J, Jw, r, lane, row); align_row<3>(J, Jw, r, lane, row);
    align_row<4>(J, Jw, r, lane, row); align_row<5>(J, Jw, r, lane, row); align_row<6>(J, Jw, r, lane, row);
    {
        const double ar = (double)fabsf(r), hb = (double)P.huber, rr = (double)r * (double)r;
        const double rho = state == 0 ? (fabsf(r) <= P.huber ? rr : hb * (2.0 * ar - hb)) : 0.0;
        const double e = align_wave_sum(rho), e2 = align_wave_sum(rr);
        if (lane == 0) { row[35] = e; row[36] = e2; }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const unsigned n = (unsigned)__popcll(__ballot(state == s));
        if (lane == 0) wcnt[wv][s] = n;
    }
    __syncthreads();
    // the workgroup's record leaves as agent-scope words, acknowledged before its ticket (the idiom of trk_eval_kernel's tail)
    const int t = threadIdx.x;
    if (t < kTsdfAlignSums) __hip_atomic_store(&P.partial[(size_t)blockIdx.x * kTsdfAlignStride + t], ((wsum[0][t] + wsum[1][t]) + wsum[2][t]) + wsum[3][t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (t < kTsdfAlignSums + 2) {                                          // words 37 and 38 of the record: the four counts, two 32-bit integers to a word
        const int s = 2 * (t - kTsdfAlignSums);
        const unsigned lo = ((wcnt[0][s] + wcnt[1][s]) + wcnt[2][s]) + wcnt[3][s], hi = ((wcnt[0][s + 1] + wcnt[1][s + 1]) + wcnt[2][s + 1]) + wcnt[3][s + 1];
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(P.partial) + (size_t)blockIdx.x * kTsdfAlignStride + t, ((unsigned long long)hi << 32) | lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (t == 0) is_last = __hip_atomic_fetch_add(P.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
    __syncthreads();
    if (!is_last) return;
    // The records in workgroup order. One lane per sum adding straight from memory waited for 8 loads in 1760 / 8 dependent round trips (318 us at 1224x368);
    // instead all 256 lanes bring kAlignStage records at a time into LDS - the records are contiguous, so the loads are coalesced and each lane has
    // kAlignStage * kTsdfAlignStride / 256 of them in flight - and 37 lanes add them from there, in order. The loads are plain ones behind ONE agent-scope acquire:
    // every word they read was stored write-through at agent scope and acknowledged before its workgroup's ticket.
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __shared__ double stage[kAlignStage * kTsdfAlignStride];
    const unsigned nb = gridDim.x;
    const double* __restrict__ part = P.partial;
    double s = 0.0;
    unsigned long long n_lo = 0, n_hi = 0;
    for (unsigned b0 = 0; b0 < nb; b0 += kAlignStage) {
        const unsigned words = min((unsigned)kAlignStage, nb - b0) * kTsdfAlignStride;
        double x[kAlignStage * kTsdfAlignStride / kAlignNT];
#pragma unroll
        for (int k = 0; k < kAlignStage * kTsdfAlignStride / kAlignNT; ++k) {
            const unsigned i = (unsigned)t + kAlignNT * k;
            x[k] = i < words ? part[(size_t)b0 * kTsdfAlignStride + i] : 0.0;     // word 39 of a record is never written and never used; words 37, 38 travel as bits
        }
#pragma unroll
        for (int k = 0; k < kAlignStage * kTsdfAlignStride / kAlignNT; ++k) stage[t + kAlignNT * k] = x[k];
        __syncthreads();
        if (t < kTsdfAlignSums)
            for (unsigned r = 0; r < words; r += kTsdfAlignStride) s += stage[r + t];
        else if (t < kTsdfAlignSums + 2)
            for (unsigned r = 0; r < words; r += kTsdfAlignStride) {
                const unsigned long long v = (unsigned long long)__double_as_longlong(stage[r + t]);
                n_lo += v & 0xFFFFFFFFull; n_hi += v >> 32;
            }
        __syncthreads();
    }
    if (t < kTsdfAlignSums) __hip_atomic_store(&P.out[t], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (t < kTsdfAlignSums + 2) {
        unsigned long long* cnt = reinterpret_cast<unsigned long long*>(P.out) + kTsdfAlignSums + 2 * (t - kTsdfAlignSums);
        __hip_atomic_store(cnt, n_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(cnt + 1, n_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (t == 0) __hip_atomic_store(P.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // re-armed for the next (stream-ordered) launch
}

int tsdf_align_launch(nalo_ctx* c, const TsdfAlignDev& D) {
    if (D.vw < 1 || D.vh < 1 || D.step < 1 || !D.depth || !D.partial || !D.ticket || !D.out) return fail(c, NALO_ERR_ARG, "tsdf_align_launch: bad arguments");
    const int gx = (D.vw + 15) / 16;
    const long long blocks = (long long)gx * ((D.vh + 15) / 16);
    if (blocks > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_align_launch: the plane needs more workgroups than a grid has");
    ProfScope ps(c, "tsdf_align");
    tsdf_align_kernel<<<(unsigned)blocks, kAlignNT, 0, c->stream>>>(D, gx);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

long long tsdf_align_blocks(int vw, int vh) { return (long long)((vw + 15) / 16) * ((vh + 15) / 16); }

}  // namespace nalo
