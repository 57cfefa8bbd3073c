// One mesh triangle of nalo_map_render_mesh from its three view-space vertices to its class, its snapped coordinates and its clipped pixel box: steps 2-5 of the
// definition in include/nalo_gpu.h ("The mesh in the 3-D panel"). ONE function for mr_tris_kernel (kernels_map_render_mesh.hip) and for the host entry
// nalo_view_triangle (host_map_render_mesh.cpp), so that what a CPU test pins is what the device runs. Plain C++ without a device call; both files are built
// without FMA contraction: every float operation below rounds on its own, in the order the header writes it.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NALO_MR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define NALO_MR_HD inline
#endif

namespace nalo {

struct MrCam { int vw, vh; float fx, fy, cx, cy, znear, zfar; };

constexpr float kMrGuard = 131072.0f;                                            // |u|, |v| below 2^17 pixels: 2^25 in sub-pixels, every edge product below 2^52
constexpr long long kMrDefaultBox = 65536;                                       // max_box_pixels == 0
constexpr int kMrMaxView = 65536;                                                // vw, vh of a mesh call
enum { MR_TRI_DRAWN = 0, MR_TRI_BAD_INDEX = 1, MR_TRI_NEAR = 2, MR_TRI_GUARD = 3, MR_TRI_DEGENERATE = 4, MR_TRI_LARGE = 5 };

// cls: the first rule that fires. X, Y: the snapped vertices (from rule 4 on: after the exchange; 0 before rule 3 has passed). box: the clipped pixel box
// x0, x1, y0, y1, inclusive, (0, -1, 0, -1) when it is empty or was not reached. swapped: vertices 1 and 2 were exchanged - the caller exchanges what they carry
struct MrTri { int cls; int X[3], Y[3]; int box[4]; bool swapped; };

NALO_MR_HD bool mr_finite(float v) { return fabsf(v) <= 3.402823466e38f; }     // false for a NaN and for an infinity

NALO_MR_HD void mr_tri_classify(const MrCam& cam, const float P[3][3], long long max_box, MrTri& T) {
    T.cls = MR_TRI_DRAWN; T.swapped = false;
    for (int i = 0; i < 3; ++i) T.X[i] = T.Y[i] = 0;
    T.box[0] = 0; T.box[1] = -1; T.box[2] = 0; T.box[3] = -1;
    bool behind = false;
    for (int i = 0; i < 3; ++i) behind = behind || !mr_finite(P[i][0]) || !mr_finite(P[i][1]) || !mr_finite(P[i][2]) || !(P[i][2] > cam.znear);
    if (behind) { T.cls = MR_TRI_NEAR; return; }
    bool guard = false;
    int X[3], Y[3];
    for (int i = 0; i < 3; ++i) {
        const float u = cam.fx * (P[i][0] / P[i][2]) + cam.cx, v = cam.fy * (P[i][1] / P[i][2]) + cam.cy;
        const bool in = u > -kMrGuard && u < kMrGuard && v > -kMrGuard && v < kMrGuard;
        guard = guard || !in;
        X[i] = in ? (int)floorf(u * 256.0f + 0.5f) : 0;                          // |u * 256 + 0.5| <= 2^25: the conversion is defined
        Y[i] = in ? (int)floorf(v * 256.0f + 0.5f) : 0;
    }
    if (guard) { T.cls = MR_TRI_GUARD; return; }
    const long long A = (long long)(X[1] - X[0]) * (long long)(Y[2] - Y[0]) - (long long)(Y[1] - Y[0]) * (long long)(X[2] - X[0]);
    if (A < 0) { int t = X[1]; X[1] = X[2]; X[2] = t; t = Y[1]; Y[1] = Y[2]; Y[2] = t; T.swapped = true; }
    for (int i = 0; i < 3; ++i) { T.X[i] = X[i]; T.Y[i] = Y[i]; }
    if (A == 0) { T.cls = MR_TRI_DEGENERATE; return; }
    const int mnx = X[0] < X[1] ? (X[0] < X[2] ? X[0] : X[2]) : (X[1] < X[2] ? X[1] : X[2]), mxx = X[0] > X[1] ? (X[0] > X[2] ? X[0] : X[2]) : (X[1] > X[2] ? X[1] : X[2]);
    const int mny = Y[0] < Y[1] ? (Y[0] < Y[2] ? Y[0] : Y[2]) : (Y[1] < Y[2] ? Y[1] : Y[2]), mxy = Y[0] > Y[1] ? (Y[0] > Y[2] ? Y[0] : Y[2]) : (Y[1] > Y[2] ? Y[1] : Y[2]);
    // pixel ix has its centre at 256 ix + 128: the first with centre >= mn is ceil((mn - 128) / 256), the last with centre <= mx is floor((mx - 128) / 256); >> 8 is
    // the floor of a division by 256 for either sign
    int x0 = (mnx + 127) >> 8, x1 = (mxx - 128) >> 8, y0 = (mny + 127) >> 8, y1 = (mxy - 128) >> 8;
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > cam.vw - 1) x1 = cam.vw - 1;
    if (y1 > cam.vh - 1) y1 = cam.vh - 1;
    if (x1 < x0 || y1 < y0) return;                                              // drawn, and nothing to draw
    if ((long long)(x1 - x0 + 1) * (long long)(y1 - y0 + 1) > max_box) T.cls = MR_TRI_LARGE;
    T.box[0] = x0; T.box[1] = x1; T.box[2] = y0; T.box[3] = y1;
}

}  // namespace nalo
