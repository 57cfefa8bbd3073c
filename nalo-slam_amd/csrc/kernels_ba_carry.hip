// nalo_ba_carry_window: the BA window re-issued from what is resident (reference paths relative to src/).
//
//  ba_carry_kernel   the device half of FullSystem::makeKeyFrame's seam between two keyframes: the frames that remain after marginalizeFrame
//                    (FullSystemMarginalize.cpp:155-212), EnergyFunctional::insertFrame's new residuals (FullSystem.cpp:1335-1348) and step 4 of
//                    activatePointsMT with the tail of optimizeImmaturePoint (FullSystem.cpp:893-917, FullSystemOptPoint.cpp:170-200).
//
// The host (host_ba.hip) works out two integer maps from mirrors it keeps anyway and sends nothing else:
//   src[d_new]   >= 0: the old device slot the point comes from   -1: padding   <= -2: -(k + 2), the k-th selected point of the pending activation
//   trow[t_new]  the old residual row of the frame, -1 for the entering frame
// One lane writes one new slot, one workgroup the 256 slots of one host: every store is a plain coalesced vector store into the SECOND set of point / slot
// buffers (the first set is the gather's source), nothing is accumulated, no lane reads what another lane of this launch writes. Inside a host src is monotone
// for the carried points (the stable Hilbert order of nalo_ba_set_points survives a renumbering), so the five 16-byte record gathers run over ascending
// addresses with holes where points left. The residual rows are t-major on both sides: a wave reads 64 scattered bytes of an old row and writes 64
// consecutive bytes of a new one.
// What nalo_ba_set_points zeroes with fills - the per-point accumulators, steps and backups, relBS, the per-slot energies and Jacobian products - this launch
// zeroes too: the whole re-issue is one kernel behind one copy of the maps.
#include "nalo_internal.h"
#include "ba_device.h"

namespace nalo {

__device__ __forceinline__ uint32_t carry_pack_last(int t0, int t1, uint32_t s0, uint32_t s1) {
    return (uint32_t)(uint8_t)(int8_t)t0 | ((uint32_t)(uint8_t)(int8_t)t1 << 8) | (s0 << 16) | (s1 << 24);
}

__global__ __launch_bounds__(256) void ba_carry_kernel(CarryDev A) {
    const int d = blockIdx.x * kBlk + threadIdx.x;                     // grid = the new window's point blocks: d < Ppad_new
    const size_t N = (size_t)A.Ppad_new;
    const int W = A.W_new;
    const int s = A.src[d];
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // the filler of a padding slot (nalo_ba_set_points)
    float4 geo = make_float4(8.f, 8.f, 1.f, 1.f), c0 = z4, c1 = z4, w0 = z4, w1 = z4;
    float prior = 0.f;
    uint8_t flags = 0;
    int ng = 0;
    uint32_t last = carry_pack_last(-1, -1, 1u, 1u);
    if (s >= 0) {                                                       // a carried point
        geo = A.o_geo[s]; c0 = A.o_col0[s]; c1 = A.o_col1[s]; w0 = A.o_w0[s]; w1 = A.o_w1[s];
        prior = A.o_prior[s];
        flags = (uint8_t)(A.o_flags[s] & (PT_VALID | PT_HAS_PRIOR));     // a decision nobody consumed does not outlive the window it was made for
        if (A.ng) {
            ng = A.o_ng[s];
            last = A.o_last[s];
            // FullSystem.cpp:1344-1345: lastResiduals[1] = lastResiduals[0]; lastResiduals[0] = (the residual to the new keyframe, IN)
            if (A.enter) last = carry_pack_last(W - 1, (int)(int8_t)(last & 0xFF), 0u, (last >> 16) & 0xFF);
        }
    } else if (s < -1) {                                                // the k-th selected point: an ImmaturePoint becomes a PointHessian (FullSystemOptPoint.cpp:170-200)
        const int k = -s - 2, i = A.a_sel[k];
        const size_t M = (size_t)A.immN;
        const float id = A.a_idepth[k];
        geo = make_float4(A.imm[i], A.imm[M + i], id, id);              // setIdepth / setIdepthZero of the optimised value
        const float2* col = reinterpret_cast<const float2*>(A.imm + 2 * M) + 4 * (size_t)i;      // 8 floats per point, 8-byte aligned whatever the set's size
        const float2* wgt = reinterpret_cast<const float2*>(A.imm + 10 * M) + 4 * (size_t)i;
        const float2 a0 = col[0], a1 = col[1], a2 = col[2], a3 = col[3], b0 = wgt[0], b1 = wgt[1], b2 = wgt[2], b3 = wgt[3];
        c0 = make_float4(a0.x, a0.y, a1.x, a1.y); c1 = make_float4(a2.x, a2.y, a3.x, a3.y);
        w0 = make_float4(b0.x, b0.y, b1.x, b1.y); w1 = make_float4(b2.x, b2.y, b3.x, b3.y);
        flags = PT_VALID;                                               // hasDepthPrior = false
        if (A.ng) {                                                     // :173-199: [0] = the residual to the newest frame, [1] to the one before, where it was made
            const bool e0 = A.a_in[(size_t)k * W + (W - 1)] != 0, e1 = A.a_in[(size_t)k * W + (W - 2)] != 0;
            last = carry_pack_last(e0 ? W - 1 : -1, e1 ? W - 2 : -1, e0 ? 0u : 1u, e1 ? 0u : 1u);
        }
    }
    A.geo[d] = geo; A.col0[d] = c0; A.col1[d] = c1; A.w0[d] = w0; A.w1[d] = w1;
    A.prior[d] = prior; A.flags[d] = flags;
    if (A.ng) { A.ng[d] = ng; A.last[d] = last; }
    A.acc[d] = z4; A.hcd[d] = z4; A.step[d] = 0.f; A.backup[d] = 0.f; A.relbs[d] = 0.f; A.relbs2[d] = 0.f; A.ngood[d] = 0;
    for (int t = 0; t < W; ++t) {                                       // t-major rows: one coalesced store per row and wave
        uint8_t st = 0;
        if (s >= 0) {
            const int r = A.trow[t];                                    // uniform: a scalar load of the kernel arguments
            st = r < 0 ? (uint8_t)RS_EXISTS : (uint8_t)(A.o_state[(size_t)r * A.Ppad_old + s] & RS_EXISTS);
        } else if (s < -1) {
            st = A.a_in[(size_t)(-s - 2) * W + t] ? (uint8_t)RS_EXISTS : (uint8_t)0;
        }
        const size_t si = (size_t)t * N + d;
        A.state[si] = st;                                               // state IN, energies zero, resetOOB: what nalo_ba_set_residuals leaves
        A.energy[si] = make_float2(0.f, 0.f);
        A.jp0[si] = z4; A.jp1[si] = z4; A.cpt[si] = z4;
    }
}

void ba_launch_carry(hipStream_t s, const CarryDev& A, int nblocks) { ba_carry_kernel<<<nblocks, kBlk, 0, s>>>(A); }

}  // namespace nalo
