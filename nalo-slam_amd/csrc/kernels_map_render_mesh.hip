// The triangles of nalo_map_render_mesh: a DEFINED rasteriser for the TSDF meshes (the welded archive, the live mesh, a caller's mesh) that paints into the 64-bit
// key plane of nalo_map_render between its lines and its resolve pass (kernels_map_render.hip). The definition: include/nalo_gpu.h, "The mesh in the 3-D panel";
// tests/render_mesh_model.py is its literal model.
//
//  mr_tris_kernel   one lane per triangle, the sources behind one another in one grid (MrTrisDev::blk0). The lane gathers its three vertices, takes them through
//                   V_f = (float)viewFromWorld and mr_tri_classify (map_render_tri.h - the function nalo_view_triangle runs on the host) to a class, snapped
//                   coordinates and a clipped pixel box. A box of at most kMrLaneBox pixels is rasterised by its lane. Bigger boxes are rasterised by the whole
//                   wave: a loop over the ballot of the lanes that hold one, that lane's set-up broadcast, the 64 lanes striding over the box - no list, no
//                   append atomic, no lane left alone in a long loop. Coverage is integer edge functions with the top-left rule; depth and colour are
//                   perspective-correct in double; every candidate is ONE integer atomicMin of (depth bits << 32) | R << 16 | G << 8 | B, so the picture does
//                   not depend on arrival order, nor on kMrLaneBox. The six counts are summed per wave, then in LDS, then with one global add per workgroup.
//
// Built without FMA contraction (build.py: NO_CONTRACT); the double divisions and the square root are the correctly rounded ones.
#include "nalo_internal.h"

namespace nalo {

namespace {

constexpr int kMrLaneBox = 64;                                                  // a box of up to this many pixels stays with its lane (the measurement)

// what a lane (or, broadcast, the wave) needs to rasterise one triangle: the snapped vertices after the exchange, their depths, their colour words (colour_mode 1:
// c0 is the triangle's grey) and the box
struct MrTriDraw { int X0, Y0, X1, Y1, X2, Y2; float z0, z1, z2; unsigned c0, c1, c2; int x0, x1, y0, y1; };

__device__ __forceinline__ bool mr_edge_in(long long E, long long dx, long long dy) { return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0))); }

__device__ __forceinline__ unsigned mr_byte(double val) { const int b = (int)floor(val + 0.5); return (unsigned)(b < 255 ? b : 255); }

// pixel (ix, iy) of a triangle: 1 when it entered a candidate
__device__ __forceinline__ unsigned mr_tri_pixel(const MrTrisDev& T, const MrTriDraw& d, int ix, int iy) {
    const long long px = 256ll * ix + 128, py = 256ll * iy + 128;
    const long long dx01 = d.X1 - d.X0, dy01 = d.Y1 - d.Y0, dx12 = d.X2 - d.X1, dy12 = d.Y2 - d.Y1, dx20 = d.X0 - d.X2, dy20 = d.Y0 - d.Y2;
    const long long w2 = dx01 * (py - d.Y0) - dy01 * (px - d.X0);
    const long long w0 = dx12 * (py - d.Y1) - dy12 * (px - d.X1);
    const long long w1 = dx20 * (py - d.Y2) - dy20 * (px - d.X2);
    if (!(mr_edge_in(w2, dx01, dy01) && mr_edge_in(w0, dx12, dy12) && mr_edge_in(w1, dx20, dy20))) return 0u;
    const long long A = (w0 + w1) + w2;                                          // the edge functions sum to the area term at every point
    const double t0 = (double)w0 / (double)d.z0, t1 = (double)w1 / (double)d.z1, t2 = (double)w2 / (double)d.z2;
    const double q = (t0 + t1) + t2;
    const float depth = (float)((double)A / q);
    if (!(depth > T.cam.znear && depth < T.cam.zfar)) return 0u;
    unsigned col = d.c0;
    if (T.colour_mode == 0) {
        col = 0u;
#pragma unroll
        for (int sh = 16; sh >= 0; sh -= 8) {
            const double a = (double)((d.c0 >> sh) & 255u), b = (double)((d.c1 >> sh) & 255u), e = (double)((d.c2 >> sh) & 255u);
            col |= mr_byte((((t0 * a) + (t1 * b)) + (t2 * e)) / q) << sh;
        }
    }
    atomicMin(&T.key[(size_t)iy * T.cam.vw + ix], ((unsigned long long)__float_as_uint(depth) << 32) | col);
    return 1u;
}

// colour_mode 1: the grey of a triangle from its view-space vertices in submitted order
__device__ __forceinline__ unsigned mr_tri_grey(const float P[3][3]) {
    const double e1x = (double)P[1][0] - (double)P[0][0], e1y = (double)P[1][1] - (double)P[0][1], e1z = (double)P[1][2] - (double)P[0][2];
    const double e2x = (double)P[2][0] - (double)P[0][0], e2y = (double)P[2][1] - (double)P[0][1], e2z = (double)P[2][2] - (double)P[0][2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const double s = len > 0.0 ? fabs(nz) / len : 0.0;
    const int g = (int)floor(64.0 + 191.0 * s);
    return (unsigned)g * 0x010101u;
}

__device__ __forceinline__ unsigned long long mr_wave_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

__global__ __launch_bounds__(256) void mr_tris_kernel(MrTrisDev T) {
    __shared__ unsigned long long sums[6];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 6) sums[tid] = 0ull;
    __syncthreads();
    int s = 0;                                                                   // the workgroup's source
    if (T.n_src > 1 && blockIdx.x >= T.blk0[1]) s = 1;
    if (T.n_src > 2 && blockIdx.x >= T.blk0[2]) s = 2;
    const MrTriSrc S = s == 0 ? T.src[0] : s == 1 ? T.src[1] : T.src[2];
    const unsigned b0 = s == 0 ? T.blk0[0] : s == 1 ? T.blk0[1] : T.blk0[2];
    const long long t = (long long)(blockIdx.x - b0) * 256 + tid;
    int cls = -1;                                                                // no triangle
    unsigned long long npix = 0;
    bool big = false;
    MrTriDraw d{};
    if (t < S.nt) {
        const int i0 = S.tri[3 * t], i1 = S.tri[3 * t + 1], i2 = S.tri[3 * t + 2];
        if (i0 < 0 || i0 >= S.nv || i1 < 0 || i1 >= S.nv || i2 < 0 || i2 >= S.nv) cls = MR_TRI_BAD_INDEX;
        else {
            const int idx[3] = {i0, i1, i2};
            float P[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float* const p = S.xyz + 3 * (size_t)idx[k];
                const float x = p[0], y = p[1], z = p[2];
#pragma unroll
                for (int r = 0; r < 3; ++r) P[k][r] = ((T.V[4 * r] * x + T.V[4 * r + 1] * y) + T.V[4 * r + 2] * z) + T.V[4 * r + 3];
            }
            MrTri R;
            mr_tri_classify(T.cam, P, T.max_box, R);
            cls = R.cls;
            if (cls == MR_TRI_DRAWN && R.box[1] >= R.box[0]) {
                d.X0 = R.X[0]; d.Y0 = R.Y[0]; d.X1 = R.X[1]; d.Y1 = R.Y[1]; d.X2 = R.X[2]; d.Y2 = R.Y[2];
                d.z0 = P[0][2]; d.z1 = R.swapped ? P[2][2] : P[1][2]; d.z2 = R.swapped ? P[1][2] : P[2][2];
                if (T.colour_mode == 0) {
                    unsigned cw[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { const uint8_t* const q = S.rgba + 4 * (size_t)idx[k]; cw[k] = ((unsigned)q[0] << 16) | ((unsigned)q[1] << 8) | q[2]; }
                    d.c0 = cw[0]; d.c1 = R.swapped ? cw[2] : cw[1]; d.c2 = R.swapped ? cw[1] : cw[2];
                } else d.c0 = d.c1 = d.c2 = mr_tri_grey(P);
                d.x0 = R.box[0]; d.x1 = R.box[1]; d.y0 = R.box[2]; d.y1 = R.box[3];
                const int bw = d.x1 - d.x0 + 1, bh = d.y1 - d.y0 + 1;
                big = (long long)bw * bh > kMrLaneBox;
                if (!big)
                    for (int iy = d.y0; iy <= d.y1; ++iy)
                        for (int ix = d.x0; ix <= d.x1; ++ix) npix += mr_tri_pixel(T, d, ix, iy);
            }
        }
    }
    // the boxes a lane does not rasterise alone: the wave takes them one by one
    for (unsigned long long todo = __ballot(big); todo; todo &= todo - 1) {
        const int src = __ffsll((long long)todo) - 1;
        MrTriDraw w;
        w.X0 = __shfl(d.X0, src); w.Y0 = __shfl(d.Y0, src); w.X1 = __shfl(d.X1, src); w.Y1 = __shfl(d.Y1, src); w.X2 = __shfl(d.X2, src); w.Y2 = __shfl(d.Y2, src);
        w.z0 = __shfl(d.z0, src); w.z1 = __shfl(d.z1, src); w.z2 = __shfl(d.z2, src);
        w.c0 = __shfl(d.c0, src); w.c1 = __shfl(d.c1, src); w.c2 = __shfl(d.c2, src);
        w.x0 = __shfl(d.x0, src); w.x1 = __shfl(d.x1, src); w.y0 = __shfl(d.y0, src); w.y1 = __shfl(d.y1, src);
        const long long bw = w.x1 - w.x0 + 1, n = bw * (w.y1 - w.y0 + 1);        // <= max_box pixels
        for (long long k = lane; k < n; k += 64) {
            const long long row = k / bw;
            npix += mr_tri_pixel(T, w, w.x0 + (int)(k - row * bw), w.y0 + (int)row);
        }
    }
    // the counts: ballots for the classes, a wave sum for the pixels; one LDS add per wave, one global add per workgroup
    unsigned nc[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) nc[k] = (unsigned)__popcll(__ballot(cls == MR_TRI_BAD_INDEX + k));
    npix = mr_wave_sum64(npix);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) if (nc[k]) atomicAdd(&sums[k], (unsigned long long)nc[k]);
        if (npix) atomicAdd(&sums[5], npix);
    }
    __syncthreads();
    if (tid < 6 && sums[tid]) atomicAdd(&T.cnt[4 + tid], sums[tid]);
}

}  // namespace

int map_render_tris_launch(nalo_ctx* c, const MrTrisDev& T) {
    const unsigned nb = T.blk0[T.n_src];
    if (nb == 0) return NALO_OK;
    ProfScope ps(c, "map_render_tris");
    mr_tris_kernel<<<nb, 256, 0, c->stream>>>(T);
    return NALO_OK;
}

}  // namespace nalo
