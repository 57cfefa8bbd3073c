// nalo_ba_window_from_initializer: the first BA window issued from the initialiser's level-0 points where they live (reference paths relative to src/FullSystem/):
//   FullSystem::initializeFromInitializer   FullSystem.cpp:1567-1654   the mean-scale sum, the PointHessians of the kept points
//   FullSystem::makeKeyFrame                FullSystem.cpp:1327-1348   the second frame enters: one residual per point, the shift of lastResiduals
//
//   iw_sum_kernel      sumID = 1e-5f; sumID += iR[i] for i = 0 .. n-1 (:1589-1594): a chain of n dependent float adds whose result depends on the order, so ONE wave
//                      runs it in index order. Every lane loads one value of a 64-value run (four runs are in flight), then all lanes add the 64 lanes' values one
//                      after the other (v_readlane, a uniform operand): no tree, no atomic, no partial sums. ~61 k adds at 1920x1072, once per session.
//   iw_flag_kernel     one lane per level-0 point: the ImmaturePoint constructor at (int)(u + 0.5f), (int)(v + 0.5f) for its verdict - is energyTH finite (:1612)? One
//                      byte per point goes up; the host, which owns the draws of the keep rule (:1607), lays the kept points out with nalo_ba_set_points' function.
//   iw_gather_kernel   one lane per slot of the new window, one workgroup per point block: the constructor again for colour and weights (cheaper than storing
//                      16 floats per level-0 point for the few that are kept), idepth = idepth_zero = iR * rescaleFactor (:1620-1621), the depth prior (:1622), the
//                      residual to frame 1 in the state nalo_ba_set_residuals leaves, the history {1, -1} / {IN, IN}, and every zero nalo_ba_set_points fills in.
// Plain vector stores only. Built without FMA contraction (the constructor's arithmetic is the reference's).
#include "nalo_internal.h"
#include "ba_device.h"
#include "imm_ctor_body.h"
#include "ordered_sum.h"

namespace nalo {

__global__ __launch_bounds__(64) void iw_sum_kernel(const float* __restrict__ iR, int n, float* __restrict__ out) {
    const float s = wave_ordered_sum(1e-5f, n, [&](int i) { return iR[i]; });      // ordered_sum.h, shared with fitPlane's mid_z (kernels_plane.hip)
    if (threadIdx.x == 0) out[0] = s;
}

// the pixel initializeFromInitializer constructs the ImmaturePoint at (:1610), and whether imm_ctor may read its pattern
__device__ __forceinline__ bool iw_pixel(const float* __restrict__ u, const float* __restrict__ v, int i, int w, int h, int& ui, int& vi) {
    ui = (int)(u[i] + 0.5f); vi = (int)(v[i] + 0.5f);
    return ui >= 2 && ui <= w - 4 && vi >= 2 && vi <= h - 4;
}

__global__ __launch_bounds__(256) void iw_flag_kernel(const float4* __restrict__ dI, int w, int h, const float* __restrict__ u, const float* __restrict__ v, int n,
                                                      uint8_t* __restrict__ ok) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int ui, vi;
    bool fin = false;
    if (iw_pixel(u, v, i, w, h, ui, vi)) fin = isfinite(imm_ctor(dI, w, ui, vi).energyTH);      // :1612 (a PointHessian copies the same energyTH: :1618 decides alike)
    ok[i] = fin ? 1 : 0;
}

__global__ __launch_bounds__(256) void iw_gather_kernel(InitWindowDev A) {
    const int d = blockIdx.x * kBlk + threadIdx.x;                      // grid = the window's point blocks: d < I.Ppad
    const int s = A.src[d];
    IssuePoint p;                                                       // the filler of a padding slot, without a history
    uint8_t st1 = 0;
    int ui, vi;
    if (s >= 0 && s < A.n && iw_pixel(A.u, A.v, s, A.w, A.h, ui, vi)) {
        const ImmCtor c = imm_ctor(A.dI, A.w, ui, vi);
        const float id = A.iR[s] * A.rescale;                           // setIdepthScaled(iR * rescaleFactor), setIdepthZero(idepth) (SCALE_IDEPTH = 1)
        p.geo = make_float4((float)ui, (float)vi, id, id);
        p.c0 = make_float4(c.color[0], c.color[1], c.color[2], c.color[3]); p.c1 = make_float4(c.color[4], c.color[5], c.color[6], c.color[7]);
        p.w0 = make_float4(c.weights[0], c.weights[1], c.weights[2], c.weights[3]); p.w1 = make_float4(c.weights[4], c.weights[5], c.weights[6], c.weights[7]);
        p.prior = A.prior;                                              // hasDepthPrior = true: EFPoint::takeData's priorF
        p.flags = PT_VALID | PT_HAS_PRIOR;
        st1 = RS_EXISTS;                                                // the residual to the entering frame (:1340-1343)
        // lastResiduals is value-initialised to {(0, IN), (0, IN)} by PointHessian and then shifted (:1344-1345): [0] = (frame 1, IN), [1] = (null, IN)
        p.last = pack_last(1, -1, 0u, 0u);
    }
    issue_store_point(A.I, d, p);
#pragma unroll
    for (int t = 0; t < 2; ++t) issue_store_row(A.I, t, d, t == 1 ? st1 : (uint8_t)0);     // t-major rows of the two-frame window
}

int init_window_scan_launch(nalo_ctx* c, const float4* dI, const float* u, const float* v, const float* iR, int n, uint8_t* ok, float* sum) {
    ProfScope ps(c, "init_window_scan");
    iw_sum_kernel<<<1, 64, 0, c->stream>>>(iR, n, sum);
    if (n > 0) iw_flag_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(dI, c->w, c->h, u, v, n, ok);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

int init_window_gather_launch(nalo_ctx* c, const InitWindowDev& A, int nblocks) {
    ProfScope ps(c, "init_window_gather");
    iw_gather_kernel<<<nblocks, kBlk, 0, c->stream>>>(A);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
