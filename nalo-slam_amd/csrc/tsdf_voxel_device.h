// The per-voxel predicate of the TSDF integration (include/nalo_gpu.h, nalo_tsdf_integrate_depth and "The replacement"), stated ONCE: which pixel a voxel
// reads, whether its depth is usable, and d; and the colour mean of an add. kernels_tsdf.hip (the integration), kernels_tsdf_replace.hip (remove / add at an
// estimate) and kernels_tsdf_replace_n.hip (the window's pairs in one launch) call them, and all three are built WITHOUT FMA contraction (build.py: NO_CONTRACT): one rounding per operation. Nothing else belongs here.
#pragma once
#include "tsdf_device.h"

namespace nalo {

struct TsdfRow { float m1y, m2z, m5y, m6z, m9y, m10z; };                        // the products of M with py and pz: a row's own, the same operands as per voxel
__device__ __forceinline__ TsdfRow tsdf_row(const float* M, float py, float pz) { return {M[1] * py, M[2] * pz, M[5] * py, M[6] * pz, M[9] * py, M[10] * pz}; }

// C: a camera and its plane (TsdfIntegrateDev, TsdfSideDev: M, fx, fy, cx, cy, w, h, depth, sy, sx, min_depth, max_depth). false: the voxel is left alone.
// true: d, and the pixel (pu, pv) it was read at. kScale: sdf = (D - zc) * s, the estimate's scale; without it the integration's own sdf = D - zc, the same
// bits as s == 1.0f (a product with 1.0f is exact)
template <bool kScale, class Cam>
__device__ __forceinline__ bool tsdf_sample(const TsdfGridDev& g, const Cam& C, float trunc, float s, const TsdfRow& R, int i, float& d, int& pu, int& pv) {
    const float px = tsdf_centre(g, 0, i);
    const float xc = ((C.M[0] * px + R.m1y) + R.m2z) + C.M[3];
    const float yc = ((C.M[4] * px + R.m5y) + R.m6z) + C.M[7];
    const float zc = ((C.M[8] * px + R.m9y) + R.m10z) + C.M[11];
    const float uf = ((C.fx * (xc / zc)) + C.cx) + 0.5f;
    const float vf = ((C.fy * (yc / zc)) + C.cy) + 0.5f;
    if (!(zc > 0.0f && uf >= 0.0f && uf < (float)C.w && vf >= 0.0f && vf < (float)C.h)) return false;
    pu = (int)uf; pv = (int)vf;                                                 // 0 <= pu < w, 0 <= pv < h: the comparisons above were made in float
    const float D = *reinterpret_cast<const float*>(C.depth + (long long)pv * C.sy + (long long)pu * C.sx);
    if (!(D >= C.min_depth && D <= C.max_depth)) return false;
    float sdf = D - zc;
    if constexpr (kScale) sdf = sdf * s;
    if (sdf < -trunc) return false;
    d = fminf(1.0f, sdf / trunc);
    return true;
}
// the pixel's colour bytes, packed B | G << 8 | R << 16 (csc already holds the B, G, R order of the caller's channels)
template <class Cam>
__device__ __forceinline__ unsigned tsdf_pixel_bgr(const Cam& C, int pu, int pv) {
    const unsigned char* px = C.colour + (long long)pv * C.csy + (long long)pu * C.csx;
    return (unsigned)px[C.csc[0]] | ((unsigned)px[C.csc[1]] << 8) | ((unsigned)px[C.csc[2]] << 16);
}
// plane X of a voxel an add updated: X = (X0 * w0 + (float)x) / (w0 + 1.0f), w0 the weight BEFORE the add, x the pixel's byte for that plane
__device__ __forceinline__ float tsdf_colour(float x0, float w0, unsigned bgr, int plane) {
    return (x0 * w0 + (float)((bgr >> (8 * plane)) & 0xFFu)) / (w0 + 1.0f);
}

}  // namespace nalo
