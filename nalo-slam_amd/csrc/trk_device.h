// One point of the tracker's photometric evaluation, calcRes + calcGSSSE (reference src/FullSystem/CoarseTracker.cpp:891-1049), shared by
// trk_eval_kernel (kernels_tracker.hip: nalo_trk_eval, the host-driven LM loop, the sharded tracker) and trk_lm_kernel (kernels_trk_lm.hip: the
// persistent LM loop). The helpers take the four texels as arguments: each kernel keeps its own load pattern. The :981 bounds test, the cutoff branch
// and the J^T hw J sum into acc[] stay written out in both kernels: the compiler optimises a helper on its own before inlining it, and as helpers
// these parts gave trk_lm_kernel a different schedule (26 spilled VGPRs instead of 6).
#pragma once
#include "nalo_internal.h"

namespace nalo {

// The 52 sums of an evaluation: slots 0-44 the upper triangle of the 9x9 sum of J^T hw J (J = 8 parameters + residual), trk_ut(r, c) for r <= c, then:
constexpr int kTrkE = 45, kTrkNE = 46, kTrkNSat = 47, kTrkNWarped = 48;     // energy, numTermsInE, numSaturated, numTermsInWarped
constexpr int kTrkST = 49, kTrkSRT = 50, kTrkSN = 51;                        // flow indicators: sumSquaredShiftT, sumSquaredShiftRT, sumSquaredShiftNum
constexpr int kTrkVals = 52;
__host__ __device__ constexpr int trk_ut(int r, int c) { return r * 9 - r * (r - 1) / 2 + (c - r); }

// one pyramid level of the tracking reference's point cloud and of the new frame
struct TrkLevel { const float *u, *v, *id, *col; const float4* dI; int n, wl, hl; float fx, fy, cx, cy; };
inline TrkLevel trk_level(const nalo_ctx* c, int slot_new, int l) {
    return {c->pc_u[l].p, c->pc_v[l].p, c->pc_id[l].p, c->pc_col[l].p, c->slots[slot_new].dI[l].p, c->pc_n[l], c->wl[l], c->hl[l], c->fx[l], c->fy[l], c->cx[l], c->cy[l]};
}

// the point (x, y) with inverse depth id warped into the new frame (:941-946)
__device__ __forceinline__ void trk_project(const float (&RKi)[9], const float (&t)[3], const TrkLevel& L, float x, float y, float id,
                                            float& u, float& v, float& Ku, float& Kv, float& new_idepth) {
    const float pt0 = RKi[0] * x + RKi[1] * y + RKi[2] + t[0] * id;
    const float pt1 = RKi[3] * x + RKi[4] * y + RKi[5] + t[1] * id;
    const float pt2 = RKi[6] * x + RKi[7] * y + RKi[8] + t[2] * id;
    u = pt0 / pt2; v = pt1 / pt2;
    Ku = L.fx * u + L.cx; Kv = L.fy * v + L.cy;
    new_idepth = id / pt2;
}
// flow indicators (:948-979) into kTrkST, kTrkSRT, kTrkSN; the caller takes every 32nd point of level 0
__device__ __forceinline__ void trk_flow(float (&acc)[kTrkVals], const float (&RKi)[9], const float (&Ki)[9], const float (&t)[3], const TrkLevel& L,
                                         float x, float y, float id, float Ku, float Kv) {
    const float a0 = Ki[0] * x + Ki[1] * y + Ki[2], a1 = Ki[3] * x + Ki[4] * y + Ki[5], a2 = Ki[6] * x + Ki[7] * y + Ki[8];
    const float T2 = a2 + t[2] * id, U2 = a2 - t[2] * id, r2 = RKi[6] * x + RKi[7] * y + RKi[8] - t[2] * id;
    const float KuT = L.fx * ((a0 + t[0] * id) / T2) + L.cx, KvT = L.fy * ((a1 + t[1] * id) / T2) + L.cy;
    const float KuT2 = L.fx * ((a0 - t[0] * id) / U2) + L.cx, KvT2 = L.fy * ((a1 - t[1] * id) / U2) + L.cy;
    const float Ku3 = L.fx * ((RKi[0] * x + RKi[1] * y + RKi[2] - t[0] * id) / r2) + L.cx;
    const float Kv3 = L.fy * ((RKi[3] * x + RKi[4] * y + RKi[5] - t[1] * id) / r2) + L.cy;
    acc[kTrkST] += (KuT - x) * (KuT - x) + (KvT - y) * (KvT - y);
    acc[kTrkST] += (KuT2 - x) * (KuT2 - x) + (KvT2 - y) * (KvT2 - y);
    acc[kTrkSRT] += (Ku - x) * (Ku - x) + (Kv - y) * (Kv - y);
    acc[kTrkSRT] += (Ku3 - x) * (Ku3 - x) + (Kv3 - y) * (Kv3 - y);
    acc[kTrkSN] += 2.f;
}
// getInterpolatedElement33 (util/globalFuncs.h:75-89) from the 16-byte texels at (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1): {I, dx, dy}
__device__ __forceinline__ float3 trk_interp(float x, float y, float4 p00, float4 p10, float4 p01, float4 p11) {
    const float dx = x - (int)x, dy = y - (int)y, dxdy = dx * dy;
    const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
    return make_float3(w11 * p11.x + w01 * p01.x + w10 * p10.x + w00 * p00.x,
                       w11 * p11.y + w01 * p01.y + w10 * p10.y + w00 * p00.y,
                       w11 * p11.z + w01 * p01.z + w10 * p10.z + w00 * p00.z);
}
// residual and Huber weight (:988-989)
__device__ __forceinline__ float trk_residual(float I, float refColor, float affa, float affb, float& hw) {
    const float residual = I - (affa * refColor + affb);
    const float ar = fabsf(residual);
    hw = ar < kHuberTH ? 1.f : kHuberTH / ar;
    return residual;
}
// the 8 parameters' Jacobian and the residual of a point inside the cutoff (calcGSSSE, :828-885)
__device__ __forceinline__ void trk_jacobian(float (&J)[9], float3 hit, float refColor, float u, float v, float new_idepth, float fx, float fy, float affa, float b0,
                                             float residual) {
    const float dx = hit.y * fx, dy = hit.z * fy;
    J[0] = new_idepth * dx; J[1] = new_idepth * dy; J[2] = -(new_idepth * (u * dx + v * dy));
    J[3] = -(u * v * dx + dy * (1.f + v * v)); J[4] = u * v * dy + dx * (1.f + u * u); J[5] = u * dy - v * dx;
    J[6] = affa * (b0 - refColor); J[7] = -1.f; J[8] = residual;
}

}  // namespace nalo
