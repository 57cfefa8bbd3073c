// The 3-D panel of PangolinDSOViewer (IOWrapper/Pangolin/PangolinDSOViewer.cpp:186-236, 448-526; KeyFrameDisplay::drawCam / drawPC, KeyFrameDisplay.cpp:609-722)
// as a DEFINED rasteriser on the device, for nalo_map_render (host_map.hip; the definition: include/nalo_gpu.h).
//
//  mr_points_kernel    one lane per entry of the virtual record list of ALL listed frames (MapSeg, nalo_internal.h; MapSeg::frame selects the row of the transform
//                      table). setFromKF's record, refreshPC's filter, vertices and colours come from map_cloud_device.h, the functions nalo_map_frame_cloud and
//                      nalo_map_dense_cloud run. A vertex inside the frustum lowers the pixel's 64-bit key to (depth bits << 32) | R << 16 | G << 8 | B with ONE
//                      integer atomicMin: a positive float orders like its bits, so the smallest key is the nearest candidate and, among equal depths, the smallest colour.
//  mr_lines_kernel     one wave per clipped segment (MrLine: the host has dropped, near-clipped, projected and viewport-clipped it in double), lanes striding over
//                      its samples; the same key update for every pixel of the width block.
//  (mr_tris_kernel     nalo_map_render_mesh's triangles enter the same plane between the lines and the resolve pass: kernels_map_render_mesh.hip)
//  mr_resolve_kernel   one lane per four pixels: the winner's colour and depth or the background and +inf, between the painters' shared front end and tail
//                      (plot_take_keys with all-ones as the idle key, plot_store4: plot_device.h); R and B change places first, the image being R first.
//
// The counts are integer atomics, summed per workgroup in LDS first. No float atomic; an integer minimum does not depend on arrival order: the bytes are the same on
// every run. Built without FMA contraction (build.py: NO_CONTRACT), the host half below included.
#include "nalo_internal.h"
#include "map_cloud_device.h"
#include "plot_device.h"

#include <cmath>

namespace nalo {

namespace {

constexpr unsigned long long kMrEmpty = ~0ull;              // a key of the idle plane (KeyPlane<unsigned long long, 0xFF>)

// the sum of v over the wave's 64 lanes, valid in lane 0 (every lane calls)
__device__ __forceinline__ unsigned mr_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// one vertex (camera space of its frame) through M, the depth range, the projection and the viewport; 1 when it was drawn
__device__ __forceinline__ int mr_vertex(const MapRenderDev& D, const float* __restrict__ M, float x, float y, float z, unsigned col) {
    const float xv = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
    const float yv = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    const float zv = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
    if (!(zv > D.cam.znear && zv < D.cam.zfar)) return 0;
    const float u = D.cam.fx * (xv / zv) + D.cam.cx, v = D.cam.fy * (yv / zv) + D.cam.cy;
    if (!(u >= 0.f && u < (float)D.cam.vw && v >= 0.f && v < (float)D.cam.vh)) return 0;
    const int ix = (int)floorf(u), iy = (int)floorf(v);
    if (ix < 0 || ix >= D.cam.vw || iy < 0 || iy >= D.cam.vh) return 0;        // ((float)vw rounds up above 2^24: never at the sizes the host accepts)
    atomicMin(&D.key[(size_t)iy * D.cam.vw + ix], ((unsigned long long)__float_as_uint(zv) << 32) | col);
    return 1;
}

__global__ __launch_bounds__(256) void mr_points_kernel(MapRenderDev D) {
    __shared__ unsigned sums[2];
    const int tid = threadIdx.x;
    if (tid < 2) sums[tid] = 0u;
    __syncthreads();
    MapSeg sg; int t;
    unsigned nv = 0, nd = 0;
    if (map_find_seg(D.S.segs, D.S.nseg, D.S.total, blockIdx.x * 256 + tid, sg, t)) {
        if (sg.kind == 4) {
            const float* const M = D.M + 12 * (size_t)sg.frame;                  // the second loop (:229-233): one vertex per dense point
            const uint4 r = reinterpret_cast<const uint4*>(sg.p)[t];
            if (map_dense_keep(r)) {
                float x, y, depth;
                map_dense_vertex(r, D.ci, x, y, depth);
                nv = 1;
                nd = mr_vertex(D, M, x, y, depth, r.w & 0xFFFFFFu);
            }
        } else {
            MapRec R;
            float depth;
            if (map_fetch_seg<true>(D.S, sg, t, R) && map_cloud_keep(D.mode, D.scaledTH, D.absTH, D.minRelBS, R, depth)) {
                constexpr int dx[8] = NALO_PATTERN_DX, dy[8] = NALO_PATTERN_DY;
                const float* const M = D.M + 12 * (size_t)R.frame;
                unsigned c0[3];
                map_cloud_mode0(R.status, c0);
                nv = 8;
#pragma unroll
                for (int pnt = 0; pnt < 8; ++pnt) {
                    float x, y;
                    map_cloud_vertex_xy(D.ci, R, depth, dx[pnt], dy[pnt], x, y);
                    const unsigned col = D.mode == 0 ? (c0[0] << 16) | (c0[1] << 8) | c0[2] : plot_byte(R.col[pnt]) * 0x010101u;
                    nd += mr_vertex(D, M, x, y, depth, col);
                }
            }
        }
    }
    nv = mr_wave_sum(nv); nd = mr_wave_sum(nd);                                 // one LDS add per wave, one global add per workgroup
    if ((tid & 63) == 0) { if (nv) atomicAdd(&sums[0], nv); if (nd) atomicAdd(&sums[1], nd); }
    __syncthreads();
    if (tid < 2 && sums[tid]) atomicAdd(&D.cnt[tid], (unsigned long long)sums[tid]);
}

__global__ __launch_bounds__(256) void mr_lines_kernel(MapRenderDev D) {
    __shared__ unsigned sum;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) sum = 0u;
    __syncthreads();
    const int li = blockIdx.x * 4 + (tid >> 6);
    unsigned ns = 0;
    if (li < D.n_lines) {
        const MrLine L = D.lines[li];
        const double du = L.ub - L.ua, dv = L.vb - L.va;
        const int lo = -(L.width / 2), hi = (L.width - 1) / 2;
        for (int j = lane; j < L.count; j += 64) {
            const double k = L.k0 + (double)j;
            const double t = L.n == 0.0 ? 0.0 : k / L.n;
            const double u = L.ua + t * du, v = L.va + t * dv;
            const float z = (float)(1.0 / ((1.0 - t) / L.za + t / L.zb));
            if (!(z > D.cam.znear && z < D.cam.zfar)) continue;
            ++ns;
            const double px = floor(u), py = floor(v);
            const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | L.col;
            for (int oy = lo; oy <= hi; ++oy) {
                const double y = py + oy;
                if (!(y >= 0.0 && y < (double)D.cam.vh)) continue;
                for (int ox = lo; ox <= hi; ++ox) {
                    const double x = px + ox;
                    if (!(x >= 0.0 && x < (double)D.cam.vw)) continue;
                    atomicMin(&D.key[(size_t)y * D.cam.vw + (size_t)x], key);
                }
            }
        }
    }
    ns = mr_wave_sum(ns);
    if (lane == 0 && ns) atomicAdd(&sum, ns);
    __syncthreads();
    if (tid == 0 && sum) atomicAdd(&D.cnt[2], (unsigned long long)sum);
}

__global__ __launch_bounds__(256) void mr_resolve_kernel(MapRenderDev D) {
    __shared__ unsigned stage[3 * 256];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid < kMrCounters) D.cnt_next[tid] = 0ull;            // the NEXT call's counters (two buffers): no fill on the path
    const size_t g0 = ((size_t)blockIdx.x * 256 + tid) * 4;                      // < padded: the grid is padded / kResolvePix workgroups
    unsigned long long key[4];
    plot_take_keys<0xFF>(D.key, g0, key);
    unsigned col[4];
    float z[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool hit = key[k] != kMrEmpty;
        const unsigned rgb = hit ? (unsigned)key[k] : D.background;              // R << 16 | G << 8 | B; the image is R first, so R goes where plot_store4 reads B
        col[k] = (rgb >> 16 & 0xFFu) | (rgb & 0xFF00u) | (rgb & 0xFFu) << 16;
        z[k] = hit ? __uint_as_float((unsigned)(key[k] >> 32)) : __uint_as_float(0x7F800000u);
    }
    *reinterpret_cast<float4*>(D.depth + g0) = make_float4(z[0], z[1], z[2], z[3]);
    plot_store4(stage, col, D.rgb + (size_t)blockIdx.x * (3 * kResolvePix));
}

}  // namespace

int map_render_launch(nalo_ctx* c, const MapRenderDev& D, MrTrisDev* T) {
    if (D.S.nb > 0) {
        ProfScope ps(c, "map_render_points");
        mr_points_kernel<<<D.S.nb, 256, 0, c->stream>>>(D);
    }
    if (D.n_lines > 0) {
        ProfScope ps(c, "map_render_lines");
        mr_lines_kernel<<<(D.n_lines + 3) / 4, 256, 0, c->stream>>>(D);
    }
    if (T && T->n_src > 0) {                                                     // nalo_map_render_mesh: a third kind of candidate in the same key plane
        T->cam = D.cam; T->key = D.key; T->cnt = D.cnt;
        const int rc = map_render_tris_launch(c, *T);
        if (rc) return rc;
    }
    {
        ProfScope ps(c, "map_render_resolve");
        mr_resolve_kernel<<<(unsigned)(D.padded / kResolvePix), 256, 0, c->stream>>>(D);
    }
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ the host half: every product as include/nalo_gpu.h writes it
void map_render_transform(const double V[12], const double C[12], float M[12]) {
    for (int r = 0; r < 3; ++r) for (int q = 0; q < 4; ++q) {
        double s = V[4 * r] * C[q];
        s = s + V[4 * r + 1] * C[4 + q];
        s = s + V[4 * r + 2] * C[8 + q];
        if (q == 3) s = s + V[4 * r + 3];
        M[4 * r + q] = (float)s;
    }
}

void map_render_apply(const float M[12], const float p[3], float out[3]) {
    for (int r = 0; r < 3; ++r) out[r] = ((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3];
}

void map_render_frustum(const float cf[4], int w, int h, float sz, float pts[5][3]) {
    const float fx = cf[0], fy = cf[1], cx = cf[2], cy = cf[3];
    const float x0 = sz * (0 - cx) / fx, x1 = sz * (w - 1 - cx) / fx, y0 = sz * (0 - cy) / fy, y1 = sz * (h - 1 - cy) / fy;
    const float p[5][3] = {{0, 0, 0}, {x0, y0, sz}, {x0, y1, sz}, {x1, y1, sz}, {x1, y0, sz}};
    std::memcpy(pts, p, sizeof(p));
}

bool map_render_line(const MrCam& cam, const float a[3], const float b[3], unsigned col, int width, MrLine* out) {
    double A[3] = {a[0], a[1], a[2]}, B[3] = {b[0], b[1], b[2]};
    for (int i = 0; i < 3; ++i) if (!std::isfinite(A[i]) || !std::isfinite(B[i])) return false;
    const double zn = cam.znear;
    if (A[2] <= zn && B[2] <= zn) return false;
    if (A[2] < zn || B[2] < zn) {                                                // at most one end is behind the plane here
        const double t = (zn - A[2]) / (B[2] - A[2]);
        double P[3];
        for (int i = 0; i < 3; ++i) P[i] = A[i] + t * (B[i] - A[i]);
        if (A[2] < zn) std::memcpy(A, P, sizeof(P)); else std::memcpy(B, P, sizeof(P));
    }
    const double fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
    MrLine L{};
    L.ua = fx * (A[0] / A[2]) + cx; L.va = fy * (A[1] / A[2]) + cy; L.ub = fx * (B[0] / B[2]) + cx; L.vb = fy * (B[1] / B[2]) + cy;
    L.za = A[2]; L.zb = B[2]; L.col = col; L.width = width;
    if (!std::isfinite(L.ua) || !std::isfinite(L.va) || !std::isfinite(L.ub) || !std::isfinite(L.vb)) return false;
    const double du = L.ub - L.ua, dv = L.vb - L.va;
    L.n = std::ceil(std::fmax(std::fabs(du), std::fabs(dv)));
    // Liang-Barsky against the viewport grown by 2 pixels
    double t0 = 0.0, t1 = 1.0;
    bool inside = true;
    const double p[4] = {-du, du, -dv, dv}, q[4] = {L.ua - (-2.0), ((double)cam.vw + 2.0) - L.ua, L.va - (-2.0), ((double)cam.vh + 2.0) - L.va};
    for (int e = 0; e < 4 && inside; ++e) {
        if (p[e] == 0.0) { if (q[e] < 0.0) inside = false; continue; }
        const double r = q[e] / p[e];
        if (p[e] < 0.0) { if (r > t1) inside = false; else if (r > t0) t0 = r; }
        else { if (r < t0) inside = false; else if (r < t1) t1 = r; }
    }
    L.k0 = 0.0; L.count = 0;
    if (inside) {
        if (L.n == 0.0) L.count = 1;
        else {
            L.k0 = std::ceil(t0 * L.n);
            const double k1 = std::floor(t1 * L.n);
            if (k1 >= L.k0) L.count = (int)std::fmin(k1 - L.k0 + 1.0, (double)cam.vw + (double)cam.vh + 10.0);
        }
    }
    *out = L;
    return true;
}

}  // namespace nalo

using namespace nalo;

extern "C" int nalo_view_look_at(const double eye[3], const double target[3], const double up[3], double viewFromWorld[12]) {
    if (!eye || !target || !up || !viewFromWorld) return NALO_ERR_ARG;
    // pangolin::ModelViewLookAt (= ModelViewLookAtRUB): z = normalised (eye - target), x = up x z, y = z x x, both normalised
    double z[3] = {eye[0] - target[0], eye[1] - target[1], eye[2] - target[2]};
    const double lz = std::sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
    for (int i = 0; i < 3; ++i) z[i] = z[i] / lz;
    double x[3] = {up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]};
    double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    const double lx = std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), ly = std::sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
    if (!(lx > 0.0) || !(ly > 0.0) || !std::isfinite(lx) || !std::isfinite(ly)) return NALO_ERR_ARG;      // pangolin throws here
    // GL's camera has x right, y up, z backward: rows x, -y, -z give x right, y down, z forward
    double R[3][3];
    for (int i = 0; i < 3; ++i) { R[0][i] = x[i] / lx; R[1][i] = -(y[i] / ly); R[2][i] = -z[i]; }
    double out[12];
    for (int r = 0; r < 3; ++r) {
        for (int i = 0; i < 3; ++i) out[4 * r + i] = R[r][i];
        out[4 * r + 3] = -((R[r][0] * eye[0] + R[r][1] * eye[1]) + R[r][2] * eye[2]);
    }
    for (int i = 0; i < 12; ++i) if (!std::isfinite(out[i])) return NALO_ERR_ARG;
    std::memcpy(viewFromWorld, out, sizeof(out));                                // written on success only
    return NALO_OK;
}
