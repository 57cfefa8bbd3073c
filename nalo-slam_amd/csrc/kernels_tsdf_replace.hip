// nalo_tsdf_replace_depth's kernel (include/nalo_gpu.h, "The replacement"): per voxel the removal of one plane's contribution at one estimate, then the add of
// another plane at another, in ONE pass over the hull of the two sides' boxes. Built WITHOUT FMA contraction: every expression below is the header's
// definition, one rounding per operation. The predicate and d are tsdf_voxel_device.h's, the statement the integration reads too; the steps of tsdf, weight
// and colour are tsdf_replace_device.h's, the statement the window replacement (kernels_tsdf_replace_n.hip) reads too.
#include "nalo_internal.h"
#include "tsdf_device.h"
#include "tsdf_voxel_device.h"
#include "tsdf_replace_device.h"

namespace nalo {

// The integration's work split (kernels_tsdf.hip): lanes run along x, a lane owns four voxels that are consecutive in memory and 16-byte aligned, one 16-byte
// load and store per array where all four lie in the hull's x range, scalar accesses at a row's two ends; a workgroup is (1 << txl) lanes along x by
// (256 >> txl) rows. Colour is a compile-time flag: the instantiation without it serves two uncoloured sides. The coloured one keeps, per voxel and side, the
// weight before that side's step and the pixel's bytes, and touches the three colour planes only in lanes that store tsdf and weight.
struct TsdfRepColour { float wr, wa; unsigned cr, ca; };                        // wr / cr: the weight before the removal and its pixel; wa / ca: before the add

// one voxel through both sides: the flags of what fired. in_r / in_a: the voxel's row lies in that side's box (and the side is on)
template <bool kColour>
__device__ __forceinline__ unsigned tsdf_replace_voxel(const TsdfReplaceDev& P, const TsdfRow& Rr, const TsdfRow& Ra, bool in_r, bool in_a, int i, float& t, float& w, TsdfRepColour& V) {
    unsigned f = 0;
    float d; int pu, pv;
    if (in_r && i >= P.rem.lo[0] && i < P.rem.hi[0] && tsdf_sample<true>(P.g, P.rem, P.trunc, P.rem.s, Rr, i, d, pu, pv)) {
        const float w0 = w;
        f = tsdf_remove_step(t, w, d);
        if constexpr (kColour) if (P.rem.coloured) { V.wr = w0; V.cr = tsdf_pixel_bgr(P.rem, pu, pv); }
    }
    if (in_a && i >= P.add.lo[0] && i < P.add.hi[0] && tsdf_sample<true>(P.g, P.add, P.trunc, P.add.s, Ra, i, d, pu, pv)) {
        const float w0 = w;
        f |= tsdf_add_step(t, w, d, P.max_weight);
        if constexpr (kColour) if (P.add.coloured) { V.wa = w0; V.ca = tsdf_pixel_bgr(P.add, pu, pv); }
    }
    return f;
}
// plane X of a voxel with flags f: the removal X = (X0 * w0 - (float)x) / (w0 - 1.0f), or 0.0f where the voxel went back to its initial values; then the add
__device__ __forceinline__ float tsdf_replace_colour(const TsdfReplaceDev& P, float x, unsigned f, const TsdfRepColour& V, int plane) {
    if ((f & kTsdfRemoved) && P.rem.coloured) x = tsdf_remove_colour(x, V.wr, V.cr, plane, (f & kTsdfReset) != 0);
    if ((f & kTsdfAdded) && P.add.coloured) x = tsdf_colour(x, V.wa, V.ca, plane);
    return x;
}

struct TsdfRepCount { int written, removed, reset, added; };
__device__ __forceinline__ void tsdf_replace_count(TsdfRepCount& n, unsigned f) {
    n.written += f != 0; n.removed += (f & kTsdfRemoved) != 0; n.reset += (f & kTsdfReset) != 0; n.added += (f & kTsdfAdded) != 0;
}

template <bool kColour>
__global__ __launch_bounds__(256) void tsdf_replace_kernel(TsdfReplaceDev P, int txl, int gx, int rows) {
    __shared__ int wsum[4][4];                                                  // [wave][count]
    const int tx = 1 << txl, ry = 256 >> txl;
    const int bx = (int)(blockIdx.x % (unsigned)gx), by = (int)(blockIdx.x / (unsigned)gx);
    const int lx = threadIdx.x & (tx - 1), ly = threadIdx.x >> txl;
    const int row = by * ry + ly;
    TsdfRepCount n = {0, 0, 0, 0};
    if (row < rows) {
        const int bny = P.hi[1] - P.lo[1];
        const int j = P.lo[1] + row % bny, k = P.lo[2] + row / bny;
        const bool in_r = P.rem.on && j >= P.rem.lo[1] && j < P.rem.hi[1] && k >= P.rem.lo[2] && k < P.rem.hi[2];
        const bool in_a = P.add.on && j >= P.add.lo[1] && j < P.add.hi[1] && k >= P.add.lo[2] && k < P.add.hi[2];
        const long long base = tsdf_index(P.g, k, j, 0);
        const long long rb = base + P.lo[0], re = base + P.hi[0];
        const long long g = (rb & ~3LL) + 4LL * ((long long)bx * tx + lx);
        if (g < re && (in_r || in_a)) {
            const float py = tsdf_centre(P.g, 1, j), pz = tsdf_centre(P.g, 2, k);
            const TsdfRow Rr = tsdf_row(P.rem.M, py, pz), Ra = tsdf_row(P.add.M, py, pz);
            if (g >= rb && g + 4 <= re) {
                float4 t = *reinterpret_cast<const float4*>(P.g.tsdf + g), w = *reinterpret_cast<const float4*>(P.g.weight + g);
                const int i = (int)(g - base);
                TsdfRepColour V0, V1, V2, V3;                                       // kColour only: of the voxels a coloured side touched
                const unsigned f0 = tsdf_replace_voxel<kColour>(P, Rr, Ra, in_r, in_a, i, t.x, w.x, V0);
                const unsigned f1 = tsdf_replace_voxel<kColour>(P, Rr, Ra, in_r, in_a, i + 1, t.y, w.y, V1);
                const unsigned f2 = tsdf_replace_voxel<kColour>(P, Rr, Ra, in_r, in_a, i + 2, t.z, w.z, V2);
                const unsigned f3 = tsdf_replace_voxel<kColour>(P, Rr, Ra, in_r, in_a, i + 3, t.w, w.w, V3);
                tsdf_replace_count(n, f0); tsdf_replace_count(n, f1); tsdf_replace_count(n, f2); tsdf_replace_count(n, f3);
                if (f0 | f1 | f2 | f3) {
                    *reinterpret_cast<float4*>(P.g.tsdf + g) = t; *reinterpret_cast<float4*>(P.g.weight + g) = w;
                    if constexpr (kColour) {
                        // a voxel that no coloured side touched goes back with the word that was loaded
#pragma unroll
                        for (int X = 0; X < 3; ++X) {
                            float4* at = reinterpret_cast<float4*>(P.g.col + (size_t)X * P.g.col_plane + g);
                            float4 cv = *at;
                            cv.x = tsdf_replace_colour(P, cv.x, f0, V0, X);
                            cv.y = tsdf_replace_colour(P, cv.y, f1, V1, X);
                            cv.z = tsdf_replace_colour(P, cv.z, f2, V2, X);
                            cv.w = tsdf_replace_colour(P, cv.w, f3, V3, X);
                            *at = cv;
                        }
                    }
                }
            } else {
                for (long long q = g < rb ? rb : g; q < g + 4 && q < re; ++q) {
                    float t = P.g.tsdf[q], w = P.g.weight[q]; TsdfRepColour V;
                    const unsigned f = tsdf_replace_voxel<kColour>(P, Rr, Ra, in_r, in_a, (int)(q - base), t, w, V);
                    if (f) {
                        P.g.tsdf[q] = t; P.g.weight[q] = w; tsdf_replace_count(n, f);
                        if constexpr (kColour) {
#pragma unroll
                            for (int X = 0; X < 3; ++X) { float* at = P.g.col + (size_t)X * P.g.col_plane + q; *at = tsdf_replace_colour(P, *at, f, V, X); }
                        }
                    }
                }
            }
        }
    }
    // the four counts: a wave reduction each, the four waves through LDS, one atomic instruction per workgroup (lane q adds count q)
    int cnt[4] = {n.written, n.removed, n.reset, n.added};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int d = 32; d > 0; d >>= 1) cnt[q] += __shfl_down(cnt[q], d, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][q] = cnt[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int s = (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
        if (s) atomicAdd(P.counts + threadIdx.x, (unsigned long long)s);
    }
}

int tsdf_replace_launch(nalo_ctx* c, const TsdfReplaceDev& D) {
    const int bnx = D.hi[0] - D.lo[0];
    const long long rows = (long long)(D.hi[1] - D.lo[1]) * (D.hi[2] - D.lo[2]);
    if (bnx < 1 || rows < 1 || rows > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_replace_launch: bad box");
    for (int a = 0; a < 3; ++a) if (D.lo[a] < 0 || D.hi[a] > (a == 0 ? D.g.nx : a == 1 ? D.g.ny : D.g.nz)) return fail(c, NALO_ERR_ARG, "tsdf_replace_launch: the box leaves the grid");
    const int groups = (bnx + 6) / 4;                                            // aligned groups of four a row's x range can touch, whatever its start
    int txl = 3;
    while (txl < 6 && (1 << txl) < groups) ++txl;                               // 8 .. 64 lanes along x
    const int tx = 1 << txl, ry = 256 >> txl, gx = (groups + tx - 1) / tx;
    const long long blocks = (long long)gx * ((rows + ry - 1) / ry);
    if (blocks > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_replace_launch: the box needs more workgroups than a grid has");
    ProfScope ps(c, "tsdf_replace");
    if (D.g.col) tsdf_replace_kernel<true><<<(unsigned)blocks, 256, 0, c->stream>>>(D, txl, gx, (int)rows);
    else tsdf_replace_kernel<false><<<(unsigned)blocks, 256, 0, c->stream>>>(D, txl, gx, (int)rows);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
