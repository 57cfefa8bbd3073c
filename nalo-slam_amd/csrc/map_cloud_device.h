// Device functions the clouds (kernels_map.hip: nalo_map_frame_cloud, nalo_map_dense_cloud) and the 3-D panel (kernels_map_render.hip: nalo_map_render) share: the
// virtual record list, KeyFrameDisplay::setFromKF's records, refreshPC's filter, vertices and colours (IOWrapper/Pangolin/KeyFrameDisplay.cpp:92-177, 225-248, 297-410).
// Every file that includes it is built without FMA contraction (build.py: NO_CONTRACT): the arithmetic is the reference's, operation by operation.
#pragma once
#include "nalo_internal.h"
#include "ba_device.h"
#include "plot_device.h"

namespace nalo {

struct MapRec { float u, v, idepth, H, relbs; int status, frame; float col[8]; };   // frame: the listed frame the record belongs to (the row of nalo_map_render's transform table)

// the segment of entry i of a virtual list and i's position in it: the last segment that starts at or before i (a binary search per lane; the lanes of a wave agree
// except at a segment's border); false past the list's end
__device__ __forceinline__ bool map_find_seg(const MapSeg* segs, int nseg, int total, int i, MapSeg& sg, int& t) {
    if (i >= total || nseg <= 0) return false;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (segs[mid].start <= i) lo = mid; else hi = mid - 1; }
    sg = segs[lo];
    t = i - sg.start;
    return t >= 0 && t < sg.n;
}

// entry t of segment sg: false when it is no record of the frame (another host's immature point, an invalid slot, an archive record of the other status)
template <bool COLOR>
__device__ __forceinline__ bool map_fetch_seg(const MapSrcDev& S, const MapSeg& sg, int t, MapRec& R) {
    R.frame = sg.frame;
    if (sg.kind == 0) {                                                         // setFromKF :121-134; the set's layout: kernels_imm_carry.hip
        const size_t N = (size_t)S.immN;
        const int host = ((const int*)(S.imm + 22 * N))[t];
        if (host < 0 || host >= NALO_MAX_WINDOW || S.imm_frame[host] < 0) return false;
        R.frame = S.imm_frame[host];
        R.u = S.imm[t]; R.v = S.imm[N + t];
        R.idepth = (S.imm[24 * N + t] + S.imm[23 * N + t]) * 0.5f;
        R.H = 1000.f; R.relbs = 0.f; R.status = 0;
        if (COLOR) {
#pragma unroll
            for (int q = 0; q < 8; ++q) R.col[q] = S.imm[2 * N + 8 * (size_t)t + q];
        }
        return true;
    }
    if (sg.kind == 1) {                                                         // :136-149
        const int d = ((const int*)sg.p)[t];
        if (!(S.flags[d] & PT_VALID)) return false;
        const float4 g = S.geo[d], pa = S.acc[d];
        float H = 0.f;
        if (pa.z != 0.f) { H = pa.x + S.prior[d]; if (H < 1e-10f) H = 1e-10f; }   // ba_flag_points_kernel's idepth_hessian
        R.u = g.x; R.v = g.y; R.idepth = kScaleIdepth * g.z; R.H = H; R.relbs = S.relbs[d]; R.status = 1;
        if (COLOR) {
            const float4 a = S.col0[d], b = S.col1[d];
            R.col[0] = a.x; R.col[1] = a.y; R.col[2] = a.z; R.col[3] = a.w; R.col[4] = b.x; R.col[5] = b.y; R.col[6] = b.z; R.col[7] = b.w;
        }
        return true;
    }
    const float4* q = reinterpret_cast<const float4*>((const nalo_map_record*)sg.p + t);   // :151-177
    const float4 a = q[0], b = q[1];
    if (__float_as_int(b.y) != sg.kind) return false;
    R.u = a.x; R.v = a.y; R.idepth = a.z; R.H = a.w; R.relbs = b.x; R.status = sg.kind;
    if (COLOR) {
        const float4 x = q[2], y = q[3];
        R.col[0] = x.x; R.col[1] = x.y; R.col[2] = x.z; R.col[3] = x.w; R.col[4] = y.x; R.col[5] = y.y; R.col[6] = y.z; R.col[7] = y.w;
    }
    return true;
}

// entry i of the virtual list
template <bool COLOR>
__device__ __forceinline__ bool map_fetch(const MapSrcDev& S, int i, MapRec& R) {
    MapSeg sg; int t;
    return map_find_seg(S.segs, S.nseg, S.total, i, sg, t) && map_fetch_seg<COLOR>(S, sg, t, R);
}

// refreshPC's tests in their order and precision (:313-331); depth comes out for the vertices
__device__ __forceinline__ bool map_cloud_keep(int mode, float scaledTH, float absTH, float minRelBS, const MapRec& R, float& depth) {
    depth = 0.f;
    if (mode == 1 && R.status != 1 && R.status != 2) return false;
    if (mode == 2 && R.status != 1) return false;
    if (mode > 2) return false;
    if (R.idepth < 0) return false;
    depth = 1.0f / R.idepth;
    float depth4 = depth * depth; depth4 *= depth4;
    const float var = (float)(1.0 / ((double)R.H + 0.01));                       // the literal 0.01 is a double
    if (var * depth4 > scaledTH) return false;
    if (var > absTH) return false;
    if (R.relbs < minRelBS) return false;
    return true;
}

// x and y of vertex pnt of a survivor (:334-340); z is depth times the jitter bracket, which is exactly 1 in the no-jitter form
__device__ __forceinline__ void map_cloud_vertex_xy(const float ci[4], const MapRec& R, float depth, int dx, int dy, float& x, float& y) {
    x = ((R.u + dx) * ci[0] + ci[2]) * depth;
    y = ((R.v + dy) * ci[1] + ci[3]) * depth;
}
// display_mode 0's constant triple of a status (:349-372), bytes {c0, c1, c2}
__device__ __forceinline__ void map_cloud_mode0(int status, unsigned t[3]) {
    t[0] = status == 3 ? 255u : 0u; t[1] = (status == 0 || status == 1) ? 255u : 0u; t[2] = (status == 0 || status == 2) ? 255u : 0u;
}

// the dense point {u | v << 16, idepth, colour, b | g << 8 | r << 16}: refreshPC() :225-248, `if(idpeth < 0) continue;` - a NaN stays
__device__ __forceinline__ bool map_dense_keep(const uint4& r) { return !(__uint_as_float(r.y) < 0); }
// its x, y and depth (z = depth times the jitter bracket) and its colour bytes {bgr[2], bgr[1], bgr[0]} as r << 16 | g << 8 | b
__device__ __forceinline__ void map_dense_vertex(const uint4& r, const float ci[4], float& x, float& y, float& depth) {
    depth = 1.0f / __uint_as_float(r.y);
    const float u = (float)(r.x & 0xFFFFu), v = (float)(r.x >> 16);
    x = (u * ci[0] + ci[2]) * depth; y = (v * ci[1] + ci[3]) * depth;
}

}  // namespace nalo
