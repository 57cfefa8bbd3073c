// ImmaturePoint::ImmaturePoint (FullSystem/ImmaturePoint.cpp:32-60) for one pixel, shared by imm_create_kernel (kernels_imm.hip) and the append of
// nalo_imm_resident_carry (kernels_imm_carry.hip). Both files are built with -ffp-contract=off: the arithmetic is the reference's scalar fp32 code,
// operation for operation, and the results are bit-identical to it.
#pragma once
#include "nalo_internal.h"

namespace nalo {

enum { IPS_GOOD = 0, IPS_OOB, IPS_OUTLIER, IPS_SKIPPED, IPS_BADCONDITION, IPS_UNINITIALIZED };   // ImmaturePoint.h:47-53

struct ImmCtor {
    float color[8], weights[8], gxx, gxy, gyy, energyTH;
    int n_ok;                                                                  // pattern pixels before the first colour that is not finite (8: none); the
};                                                                             // constructor returns there (:50): color[n_ok] is set, weights[n_ok..] are not

// the pattern of pixel (u, v) must lie inside the image with one texel to spare to the right and below (u, v in [2, w - 4] x [2, h - 4])
__device__ __forceinline__ ImmCtor imm_ctor(const float4* __restrict__ dI, int w, int u, int v) {
    ImmCtor r;
    r.gxx = r.gxy = r.gyy = 0;
    r.n_ok = 8;
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) { r.color[idx] = 0; r.weights[idx] = 0; }
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) {
        const float x = (float)(u + kPatternDx[idx]), y = (float)(v + kPatternDy[idx]);
        const int ix = (int)x, iy = (int)y;
        const float4* bp = dI + ix + iy * w;                                   // getInterpolatedElement33BiLin, globalFuncs.h:166-188
        const float tl = bp[0].x, tr = bp[1].x, bl = bp[w].x, br = bp[w + 1].x;
        const float dx = x - ix, dy = y - iy;
        const float topInt = dx * tr + (1 - dx) * tl, botInt = dx * br + (1 - dx) * bl, leftInt = dy * bl + (1 - dy) * tl, rightInt = dy * br + (1 - dy) * tr;
        const float c0 = dx * rightInt + (1 - dx) * leftInt, g0 = rightInt - leftInt, g1 = botInt - topInt;
        r.color[idx] = c0;
        if (!isfinite(c0)) { r.n_ok = idx; break; }
        r.gxx += g0 * g0; r.gxy += g0 * g1; r.gyy += g1 * g1;
        r.weights[idx] = sqrtf(kOutlierTHSumComponent / (kOutlierTHSumComponent + (g0 * g0 + g1 * g1)));
    }
    if (r.n_ok < 8) { r.energyTH = NAN; return r; }
    float eth = 8 * kOutlierTH;
    eth *= kOverallEnergyTHWeight * kOverallEnergyTHWeight;
    r.energyTH = eth;
    return r;
}

}  // namespace nalo
