// nalo_ba_carry_window: the BA window re-issued from what is resident (reference paths relative to src/).
//
//  ba_carry_kernel   the device half of FullSystem::makeKeyFrame's seam between two keyframes: the frames that remain after marginalizeFrame
//                    (FullSystemMarginalize.cpp:155-212), EnergyFunctional::insertFrame's new residuals (FullSystem.cpp:1335-1348) and step 4 of
//                    activatePointsMT with the tail of optimizeImmaturePoint (FullSystem.cpp:893-917, FullSystemOptPoint.cpp:170-200).
//
// The host (host_ba.hip) works out two integer maps from mirrors it keeps anyway and sends nothing else:
//   src[d_new]   >= 0: the old device slot the point comes from   -1: padding   <= -2: -(k + 2), the k-th selected point of the pending activation
//   trow[t_new]  the old residual row of the frame, -1 for the entering frame
// src travels in the pinned block every device issue stages, [src | blk_host | host_blk | sc_grp | blk_order] (stage_issue_tables); trow, 16 words, is a kernel argument.
// One lane writes one new slot, one workgroup the 256 slots of one host: every store is a plain coalesced vector store into the SECOND set of point / slot
// buffers (the first set is the gather's source), nothing is accumulated, no lane reads what another lane of this launch writes. Inside a host src is monotone
// for the carried points (the stable Hilbert order of nalo_ba_set_points survives a renumbering), so the five 16-byte record gathers run over ascending
// addresses with holes where points left. The residual rows are t-major on both sides: a wave reads 64 scattered bytes of an old row and writes 64
// consecutive bytes of a new one.
// What nalo_ba_set_points zeroes with fills - the per-point accumulators, steps and backups, relBS, the per-slot energies and Jacobian products - this launch
// zeroes too: the whole re-issue is one kernel behind one copy of the maps. The kernel keeps only where a point comes from; what a slot holds and how it is
// written is ba_device.h's (IssuePoint, issue_store_point, issue_store_row), shared with iw_gather_kernel.
#include "nalo_internal.h"
#include "ba_device.h"

namespace nalo {

__global__ __launch_bounds__(256) void ba_carry_kernel(CarryDev A) {
    const int d = blockIdx.x * kBlk + threadIdx.x;                     // grid = the new window's point blocks: d < I.Ppad
    const int W = A.I.W;
    const int s = A.src[d];
    IssuePoint p;                                                       // the filler of a padding slot
    if (s >= 0) {                                                       // a carried point
        p.geo = A.o_geo[s]; p.c0 = A.o_col0[s]; p.c1 = A.o_col1[s]; p.w0 = A.o_w0[s]; p.w1 = A.o_w1[s];
        p.prior = A.o_prior[s];
        p.flags = (uint8_t)(A.o_flags[s] & (PT_VALID | PT_HAS_PRIOR));   // a decision nobody consumed does not outlive the window it was made for
        if (A.I.ng) {
            p.ng = A.o_ng[s];
            p.last = A.o_last[s];
            // FullSystem.cpp:1344-1345: lastResiduals[1] = lastResiduals[0]; lastResiduals[0] = (the residual to the new keyframe, IN)
            if (A.enter) p.last = pack_last(W - 1, (int)(int8_t)(p.last & 0xFF), 0u, (p.last >> 16) & 0xFF);
        }
    } else if (s < -1) {                                                // the k-th selected point: an ImmaturePoint becomes a PointHessian (FullSystemOptPoint.cpp:170-200)
        const int k = -s - 2, i = A.a_sel[k];
        const size_t M = (size_t)A.immN;
        const float id = A.a_idepth[k];
        p.geo = make_float4(A.imm[i], A.imm[M + i], id, id);            // setIdepth / setIdepthZero of the optimised value
        const float2* col = reinterpret_cast<const float2*>(A.imm + 2 * M) + 4 * (size_t)i;      // 8 floats per point, 8-byte aligned whatever the set's size
        const float2* wgt = reinterpret_cast<const float2*>(A.imm + 10 * M) + 4 * (size_t)i;
        const float2 a0 = col[0], a1 = col[1], a2 = col[2], a3 = col[3], b0 = wgt[0], b1 = wgt[1], b2 = wgt[2], b3 = wgt[3];
        p.c0 = make_float4(a0.x, a0.y, a1.x, a1.y); p.c1 = make_float4(a2.x, a2.y, a3.x, a3.y);
        p.w0 = make_float4(b0.x, b0.y, b1.x, b1.y); p.w1 = make_float4(b2.x, b2.y, b3.x, b3.y);
        p.flags = PT_VALID;                                             // hasDepthPrior = false
        if (A.I.ng) {                                                   // :173-199: [0] = the residual to the newest frame, [1] to the one before, where it was made
            const bool e0 = A.a_in[(size_t)k * W + (W - 1)] != 0, e1 = A.a_in[(size_t)k * W + (W - 2)] != 0;
            p.last = pack_last(e0 ? W - 1 : -1, e1 ? W - 2 : -1, e0 ? 0u : 1u, e1 ? 0u : 1u);
        }
    }
    issue_store_point(A.I, d, p);
    for (int t = 0; t < W; ++t) {                                       // t-major rows: one coalesced store per row and wave
        uint8_t st = 0;
        if (s >= 0) {
            const int r = A.trow[t];                                    // uniform: a scalar load of the kernel arguments
            st = r < 0 ? (uint8_t)RS_EXISTS : (uint8_t)(A.o_state[(size_t)r * A.Ppad_old + s] & RS_EXISTS);
        } else if (s < -1) {
            st = A.a_in[(size_t)(-s - 2) * W + t] ? (uint8_t)RS_EXISTS : (uint8_t)0;
        }
        issue_store_row(A.I, t, d, st);
    }
}

void ba_launch_carry(hipStream_t s, const CarryDev& A, int nblocks) { ba_carry_kernel<<<nblocks, kBlk, 0, s>>>(A); }

}  // namespace nalo
