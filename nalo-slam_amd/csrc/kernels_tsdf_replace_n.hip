// nalo_tsdf_replace_depth_n's kernel (include/nalo_gpu.h, "The window replacement"): per voxel the chain remove, add, remove, add ... of up to 16 pairs, in
// ONE pass over the hull of every side's box, the voxel's tsdf, weight and colour words held in registers from one load to one store. Built WITHOUT FMA
// contraction: the predicate and d are tsdf_voxel_device.h's, the steps tsdf_replace_device.h's, the statements nalo_tsdf_replace_depth's kernel reads too, so n
// launches of that kernel and one of this one compute the same bits.
#include "nalo_internal.h"
#include "tsdf_device.h"
#include "tsdf_voxel_device.h"
#include "tsdf_replace_device.h"

namespace nalo {

// The work split is tsdf_replace_kernel's: lanes along x, four consecutive 16-byte-aligned voxels a lane, 16-byte accesses where all four lie in the hull's x
// range, scalar accesses at a row's two ends, (1 << txl) lanes by (256 >> txl) rows a workgroup. The loop nest is pairs outside, the lane's four voxels inside:
// a side's row test and its TsdfRow are computed when the side is reached, so one TsdfRow is live at a time. The sides come from a device table read at
// wave-uniform indices. A side's box lies inside the hull, so a voxel of the lane's group beyond the hull's x range fails every side's x test by itself.
//
// Colour is a compile-time flag. The coloured instantiation loads the lane's twelve colour words the first time a coloured side fires on one of its voxels
// and stores them only then: a lane no coloured side touched never names the colour planes.
//
// Counts: a wave ballot per flag and voxel, population counts summed in scalar registers, lane 0 of the wave adds the pair's four sums into LDS (integer
// LDS atomics), and behind the last pair lanes 0 .. 4n add the workgroup's sums to memory: one atomic instruction per counter per workgroup.
struct TsdfLane4 { float t[4], w[4]; };

template <bool kColour>
__global__ __launch_bounds__(256) void tsdf_replace_n_kernel(TsdfReplaceNDev P, int txl, int gx, int rows) {
    __shared__ int lsum[4 * kTsdfReplaceMaxPairs + 1];
    const TsdfSideDev* __restrict__ sides = P.sides;
    const int nside = 2 * P.n;
    if (threadIdx.x < 4 * kTsdfReplaceMaxPairs + 1) lsum[threadIdx.x] = 0;
    __syncthreads();
    const int tx = 1 << txl, ry = 256 >> txl;
    const int bx = (int)(blockIdx.x % (unsigned)gx), by = (int)(blockIdx.x / (unsigned)gx);
    const int lx = threadIdx.x & (tx - 1), ly = threadIdx.x >> txl;
    const int row = by * ry + ly;
    const bool lane0 = (threadIdx.x & 63) == 0;

    // ---- the lane's group, and which sides' boxes hold its row (bit s of `in`): rows of the hull in no box leave before any voxel is loaded
    bool live = false, full = false;
    int j = 0, k = 0, i0 = 0;
    long long g = 0, rb = 0, re = 0;
    unsigned in = 0;
    if (row < rows) {
        const int bny = P.hi[1] - P.lo[1];
        j = P.lo[1] + row % bny; k = P.lo[2] + row / bny;
        const long long base = tsdf_index(P.g, k, j, 0);
        rb = base + P.lo[0]; re = base + P.hi[0];
        g = (rb & ~3LL) + 4LL * ((long long)bx * tx + lx);
        i0 = (int)(g - base);
        if (g < re) {
            for (int s = 0; s < nside; ++s) {
                const TsdfSideDev& S = sides[s];
                if (S.on && j >= S.lo[1] && j < S.hi[1] && k >= S.lo[2] && k < S.hi[2] && i0 + 4 > S.lo[0] && i0 < S.hi[0]) in |= 1u << s;
            }
            live = in != 0;
            full = g >= rb && g + 4 <= re;
        }
    }
    if (__ballot(live) != 0ull) {                                               // wave-uniform: a wave with no live lane has nothing to count either
        TsdfLane4 V;
        float col[3][4];
        bool have_col = false;                                                  // kColour only: the colour words are in registers (and go back)
        unsigned any = 0;                                                       // bit v: some pair fired at voxel v
#pragma unroll
        for (int v = 0; v < 4; ++v) { V.t[v] = 0.0f; V.w[v] = 0.0f; }
        if (live) {
            if (full) {
                const float4 t4 = *reinterpret_cast<const float4*>(P.g.tsdf + g), w4 = *reinterpret_cast<const float4*>(P.g.weight + g);
                V.t[0] = t4.x; V.t[1] = t4.y; V.t[2] = t4.z; V.t[3] = t4.w; V.w[0] = w4.x; V.w[1] = w4.y; V.w[2] = w4.z; V.w[3] = w4.w;
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) if (g + v >= rb && g + v < re) { V.t[v] = P.g.tsdf[g + v]; V.w[v] = P.g.weight[g + v]; }
            }
        }
        const float py = tsdf_centre(P.g, 1, j), pz = tsdf_centre(P.g, 2, k);
        for (int pr = 0; pr < P.n; ++pr) {
            unsigned f[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
            for (int h = 0; h < 2; ++h) {                                       // h = 0: the pair's remove side, 1: its add side
                const int s = 2 * pr + h;
                if (!((in >> s) & 1u)) continue;
                const TsdfSideDev& S = sides[s];
                const TsdfRow R = tsdf_row(S.M, py, pz);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int i = i0 + v;
                    float d; int pu, pv;
                    if (!(i >= S.lo[0] && i < S.hi[0] && tsdf_sample<true>(P.g, S, P.trunc, S.s, R, i, d, pu, pv))) continue;
                    const float w0 = V.w[v];
                    const unsigned fs = h == 0 ? tsdf_remove_step(V.t[v], V.w[v], d) : tsdf_add_step(V.t[v], V.w[v], d, P.max_weight);
                    f[v] |= fs;
                    if constexpr (kColour) {
                        if (S.coloured) {
                            if (!have_col) {                                    // the lane's twelve words, once
                                have_col = true;
#pragma unroll
                                for (int X = 0; X < 3; ++X) {
                                    const float* cp = P.g.col + (size_t)X * P.g.col_plane + g;
                                    if (full) { const float4 c4 = *reinterpret_cast<const float4*>(cp); col[X][0] = c4.x; col[X][1] = c4.y; col[X][2] = c4.z; col[X][3] = c4.w; }
                                    else {
#pragma unroll
                                        for (int u = 0; u < 4; ++u) col[X][u] = (g + u >= rb && g + u < re) ? cp[u] : 0.0f;
                                    }
                                }
                            }
                            const unsigned bgr = tsdf_pixel_bgr(S, pu, pv);
#pragma unroll
                            for (int X = 0; X < 3; ++X) col[X][v] = h == 0 ? tsdf_remove_colour(col[X][v], w0, bgr, X, (fs & kTsdfReset) != 0) : tsdf_colour(col[X][v], w0, bgr, X);
                        }
                    }
                }
            }
            // the pair's four counts over the wave: removed, reset, added, written
            int n_rem = 0, n_rst = 0, n_add = 0, n_wr = 0;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                n_rem += __popcll(__ballot((f[v] & kTsdfRemoved) != 0)); n_rst += __popcll(__ballot((f[v] & kTsdfReset) != 0));
                n_add += __popcll(__ballot((f[v] & kTsdfAdded) != 0)); n_wr += __popcll(__ballot(f[v] != 0));
                any |= (f[v] != 0 ? 1u : 0u) << v;
            }
            if (lane0 && n_wr) {
                if (n_rem) atomicAdd(&lsum[4 * pr + 0], n_rem);
                if (n_rst) atomicAdd(&lsum[4 * pr + 1], n_rst);
                if (n_add) atomicAdd(&lsum[4 * pr + 2], n_add);
                atomicAdd(&lsum[4 * pr + 3], n_wr);
            }
        }
        if (any) {
            if (full) {
                *reinterpret_cast<float4*>(P.g.tsdf + g) = make_float4(V.t[0], V.t[1], V.t[2], V.t[3]);
                *reinterpret_cast<float4*>(P.g.weight + g) = make_float4(V.w[0], V.w[1], V.w[2], V.w[3]);
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) if ((any >> v) & 1u) { P.g.tsdf[g + v] = V.t[v]; P.g.weight[g + v] = V.w[v]; }      // a voxel that fired lies in the hull's x range
            }
            if constexpr (kColour) {
                if (have_col) {
                    // a voxel that no coloured side touched goes back with the word that was loaded
#pragma unroll
                    for (int X = 0; X < 3; ++X) {
                        float* cp = P.g.col + (size_t)X * P.g.col_plane + g;
                        if (full) *reinterpret_cast<float4*>(cp) = make_float4(col[X][0], col[X][1], col[X][2], col[X][3]);
                        else {
#pragma unroll
                            for (int v = 0; v < 4; ++v) if ((any >> v) & 1u) cp[v] = col[X][v];
                        }
                    }
                }
            }
        }
        const int n_any = __popc(any);
        int tot = n_any;
        for (int d = 32; d > 0; d >>= 1) tot += __shfl_down(tot, d, 64);
        if (lane0 && tot) atomicAdd(&lsum[4 * P.n], tot);
    }
    __syncthreads();
    if ((int)threadIdx.x <= 4 * P.n) {
        const int s = lsum[threadIdx.x];
        if (s) atomicAdd(P.counts + threadIdx.x, (unsigned long long)s);
    }
}

int tsdf_replace_n_launch(nalo_ctx* c, const TsdfReplaceNDev& D) {
    const int bnx = D.hi[0] - D.lo[0];
    const long long rows = (long long)(D.hi[1] - D.lo[1]) * (D.hi[2] - D.lo[2]);
    if (D.n < 1 || D.n > kTsdfReplaceMaxPairs || !D.sides || !D.counts) return fail(c, NALO_ERR_ARG, "tsdf_replace_n_launch: bad argument");
    if (bnx < 1 || rows < 1 || rows > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_replace_n_launch: bad box");
    for (int a = 0; a < 3; ++a) if (D.lo[a] < 0 || D.hi[a] > (a == 0 ? D.g.nx : a == 1 ? D.g.ny : D.g.nz)) return fail(c, NALO_ERR_ARG, "tsdf_replace_n_launch: the box leaves the grid");
    const int groups = (bnx + 6) / 4;                                            // aligned groups of four a row's x range can touch, whatever its start
    int txl = 3;
    while (txl < 6 && (1 << txl) < groups) ++txl;                               // 8 .. 64 lanes along x
    const int tx = 1 << txl, ry = 256 >> txl, gx = (groups + tx - 1) / tx;
    const long long blocks = (long long)gx * ((rows + ry - 1) / ry);
    if (blocks > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_replace_n_launch: the box needs more workgroups than a grid has");
    ProfScope ps(c, "tsdf_replace_n");
    if (D.g.col) tsdf_replace_n_kernel<true><<<(unsigned)blocks, 256, 0, c->stream>>>(D, txl, gx, (int)rows);
    else tsdf_replace_n_kernel<false><<<(unsigned)blocks, 256, 0, c->stream>>>(D, txl, gx, (int)rows);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
