// The TSDF volume's kernels (include/nalo_gpu.h, "tsdf=1"): the projective integration of one depth plane over the culling box, the sub-block copies, the whole-voxel shift
// (nalo_tsdf_shift) and the plane nalo_tsdf_integrate_frame makes of a frame's dense list. (The surface points are kernels_tsdf_mesh.hip's: the mesh's passes on the axis edges.) Built
// WITHOUT FMA contraction: every expression below is the header's definition, one rounding per operation.
#include "nalo_internal.h"
#include "tsdf_device.h"
#include "tsdf_voxel_device.h"

namespace nalo {

// ---- integration. Lanes run along x: a lane owns four voxels that are consecutive in memory and 16-byte aligned (the arrays are allocations of their own, so
// alignment is a matter of the linear index), one 16-byte load and store per array where all four lie in the box's x range, scalar accesses at a row's two ends.
// A workgroup is (1 << txl) lanes along x by (256 >> txl) rows of the box, so that a narrow box does not idle most of a wave.
// Colour (nalo_tsdf_color_enable) is a compile-time flag: the uncoloured kernel is the instantiation without it. The coloured one keeps w0 and the colour bytes
// of the voxels it updates and touches the three colour planes only in lanes that store tsdf and weight, so the visited-but-untouched box moves no colour byte.
// kColour: a voxel that is updated also hands back the weight BEFORE the update and its pixel's colour bytes, packed B | G << 8 | R << 16. The predicate and d
// are tsdf_voxel_device.h's, the one statement nalo_tsdf_replace_depth's kernel reads too
template <bool kColour>
__device__ __forceinline__ bool tsdf_voxel(const TsdfIntegrateDev& P, const TsdfRow& R, int i, float& t, float& w, float& wb, unsigned& bgr) {
    float d; int pu, pv;
    if (!tsdf_sample<false>(P.g, P, P.trunc, 1.0f, R, i, d, pu, pv)) return false;
    const float t0 = t, w0 = w;
    t = (t0 * w0 + d) / (w0 + 1.0f);
    w = fminf(w0 + 1.0f, P.max_weight);
    if constexpr (kColour) {
        wb = w0;
        bgr = tsdf_pixel_bgr(P, pu, pv);
    }
    return true;
}

template <bool kColour>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfIntegrateDev P, int txl, int gx, int rows) {
    __shared__ int wsum[4];
    const int tx = 1 << txl, ry = 256 >> txl;
    const int bx = (int)(blockIdx.x % (unsigned)gx), by = (int)(blockIdx.x / (unsigned)gx);
    const int lx = threadIdx.x & (tx - 1), ly = threadIdx.x >> txl;
    const int row = by * ry + ly;
    int n = 0;
    if (row < rows) {
        const int bny = P.hi[1] - P.lo[1];
        const int j = P.lo[1] + row % bny, k = P.lo[2] + row / bny;
        const long long base = tsdf_index(P.g, k, j, 0);
        const long long rb = base + P.lo[0], re = base + P.hi[0];
        const long long g = (rb & ~3LL) + 4LL * ((long long)bx * tx + lx);
        if (g < re) {
            const float py = tsdf_centre(P.g, 1, j), pz = tsdf_centre(P.g, 2, k);
            const TsdfRow R = tsdf_row(P.M, py, pz);
            if (g >= rb && g + 4 <= re) {
                float4 t = *reinterpret_cast<const float4*>(P.g.tsdf + g), w = *reinterpret_cast<const float4*>(P.g.weight + g);
                const int i = (int)(g - base);
                float4 wb; uint4 bgr;                                               // kColour only: of the voxels that were updated
                const bool u0 = tsdf_voxel<kColour>(P, R, i, t.x, w.x, wb.x, bgr.x);
                const bool u1 = tsdf_voxel<kColour>(P, R, i + 1, t.y, w.y, wb.y, bgr.y);
                const bool u2 = tsdf_voxel<kColour>(P, R, i + 2, t.z, w.z, wb.z, bgr.z);
                const bool u3 = tsdf_voxel<kColour>(P, R, i + 3, t.w, w.w, wb.w, bgr.w);
                n += (int)u0 + (int)u1 + (int)u2 + (int)u3;
                if (n) { *reinterpret_cast<float4*>(P.g.tsdf + g) = t; *reinterpret_cast<float4*>(P.g.weight + g) = w; }
                if constexpr (kColour) {
                    // the colour of a lane moves only when one of its four voxels was updated; a voxel that was not goes back with the word that was loaded
                    if (n) {
#pragma unroll
                        for (int X = 0; X < 3; ++X) {
                            float4* at = reinterpret_cast<float4*>(P.g.col + (size_t)X * P.g.col_plane + g);
                            float4 cv = *at;
                            if (u0) cv.x = tsdf_colour(cv.x, wb.x, bgr.x, X);
                            if (u1) cv.y = tsdf_colour(cv.y, wb.y, bgr.y, X);
                            if (u2) cv.z = tsdf_colour(cv.z, wb.z, bgr.z, X);
                            if (u3) cv.w = tsdf_colour(cv.w, wb.w, bgr.w, X);
                            *at = cv;
                        }
                    }
                }
            } else {
                for (long long q = g < rb ? rb : g; q < g + 4 && q < re; ++q) {
                    float t = P.g.tsdf[q], w = P.g.weight[q], wb; unsigned bgr;
                    if (tsdf_voxel<kColour>(P, R, (int)(q - base), t, w, wb, bgr)) {
                        P.g.tsdf[q] = t; P.g.weight[q] = w; ++n;
                        if constexpr (kColour) {
#pragma unroll
                            for (int X = 0; X < 3; ++X) { float* at = P.g.col + (size_t)X * P.g.col_plane + q; *at = tsdf_colour(*at, wb, bgr, X); }
                        }
                    }
                }
            }
        }
    }
    // the updated count: a wave reduction, the four waves through LDS, one atomic per workgroup
    for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (s) atomicAdd(P.updated, (unsigned long long)s);
    }
}

int tsdf_integrate_launch(nalo_ctx* c, const TsdfIntegrateDev& D) {
    const int bnx = D.hi[0] - D.lo[0];
    const long long rows = (long long)(D.hi[1] - D.lo[1]) * (D.hi[2] - D.lo[2]);
    if (bnx < 1 || rows < 1 || rows > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_integrate_launch: bad box");
    const int groups = (bnx + 6) / 4;                                            // aligned groups of four a row's x range can touch, whatever its start
    int txl = 3;
    while (txl < 6 && (1 << txl) < groups) ++txl;                               // 8 .. 64 lanes along x
    const int tx = 1 << txl, ry = 256 >> txl, gx = (groups + tx - 1) / tx;
    const long long blocks = (long long)gx * ((rows + ry - 1) / ry);
    if (blocks > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_integrate_launch: the box needs more workgroups than a grid has");
    ProfScope ps(c, "tsdf_integrate");
    if (D.g.col) tsdf_integrate_kernel<true><<<(unsigned)blocks, 256, 0, c->stream>>>(D, txl, gx, (int)rows);
    else tsdf_integrate_kernel<false><<<(unsigned)blocks, 256, 0, c->stream>>>(D, txl, gx, (int)rows);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

__global__ __launch_bounds__(256) void tsdf_fill_kernel(float* tsdf, float* weight, size_t n) {
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += stride) {
        reinterpret_cast<float4*>(tsdf)[q] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        reinterpret_cast<float4*>(weight)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) { tsdf[4 * n4 + threadIdx.x] = 1.0f; weight[4 * n4 + threadIdx.x] = 0.0f; }
}
int tsdf_fill_launch(nalo_ctx* c, float* tsdf, float* weight, size_t n) {
    const size_t want = (n / 4 + 255) / 256;
    tsdf_fill_kernel<<<(unsigned)std::min<size_t>(std::max<size_t>(want, 1), 2048), 256, 0, c->stream>>>(tsdf, weight, n);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

struct TsdfBlock { int nx, ny, lo[3], size[3]; };                               // the copy serves any one array of the grid: it takes the two dims the index needs
__global__ __launch_bounds__(256) void tsdf_block_kernel(float* vol, float* block, TsdfBlock B, int total, int to_volume) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const int x = q % B.size[0], y = (q / B.size[0]) % B.size[1], z = q / (B.size[0] * B.size[1]);
    const size_t at = ((size_t)(B.lo[2] + z) * B.ny + (B.lo[1] + y)) * B.nx + (B.lo[0] + x);      // tsdf_index of the voxel, on the two dims the copy holds
    if (to_volume) vol[at] = block[q]; else block[q] = vol[at];
}
int tsdf_block_launch(nalo_ctx* c, float* vol, float* block, const int dims[3], const int lo[3], const int size[3], int to_volume) {
    TsdfBlock B = {dims[0], dims[1], {lo[0], lo[1], lo[2]}, {size[0], size[1], size[2]}};
    const int total = size[0] * size[1] * size[2];                               // <= 2^29, checked by the caller
    tsdf_block_kernel<<<(total + 255) / 256, 256, 0, c->stream>>>(vol, block, B, total, to_volume);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// ---- nalo_tsdf_shift. A pure copy, driven from the destination and out of place: dst voxel (i, j, k) takes the words of src voxel (i + s0, j + s1, k + s2), or
// the initial values where that lies outside the grid. As in the integration a lane owns four voxels that are consecutive in memory and 16-byte aligned by
// linear index, here over the whole array, so where nx is no multiple of four a group straddles rows. The n % 4 voxels behind the last whole group go one to a
// lane, word by word: no access reaches past the arrays. A group is classified once and every array (tsdf, weight, the three colour planes) moves by it:
//   kTsdfShiftInit   the group lies in one row and all four sources lie outside the grid: the initial values are stored, nothing is loaded
//   kTsdfShiftRow    the group lies in one row and so do its four sources, inside the grid: they are consecutive at g + delta, one 16-byte load where delta is a
//                    multiple of four (for nx a multiple of four: s0 % 4 == 0), else four words
//   kTsdfShiftMixed  everything else (a row's two ends, a group that straddles rows): each voxel on its own index
// Words move as unsigned: no float operation touches them, so NaN payloads, -0.0f and denormals pass. Colour is a compile-time flag.
enum { kTsdfShiftInit = 0, kTsdfShiftRow = 1, kTsdfShiftMixed = 2 };
struct TsdfShiftGroup { long long g, at[4]; int mode, in; };                   // at[e]: the source index of voxel g + e where bit e of `in` is set

// the source of the voxel with linear index idx (below 2^29: its split into (i, j, k) is 32-bit arithmetic, the addresses are not); false: outside the grid
__device__ __forceinline__ bool tsdf_shift_source(const TsdfShiftDev& P, unsigned idx, long long& at) {
    const unsigned row = idx / (unsigned)P.nx, k = row / (unsigned)P.ny;
    const int si = (int)(idx - row * (unsigned)P.nx) + P.s[0], sj = (int)(row - k * (unsigned)P.ny) + P.s[1], sk = (int)k + P.s[2];
    at = ((long long)sk * P.ny + sj) * P.nx + si;
    return si >= 0 && si < P.nx && sj >= 0 && sj < P.ny && sk >= 0 && sk < P.nz;
}

// V4: four words as one access. tsdf and weight are allocations of their own, so a group is 16-byte aligned: uint4. A colour plane begins n words into its
// block, 16-byte aligned only where n is a multiple of four: TsdfWords4 says so to the compiler, which still issues one 16-byte access (global memory takes it
// at any 4-byte aligned address), at full rate where the address is aligned
typedef uint4 __attribute__((aligned(4))) TsdfWords4;
template <typename V4>
__device__ __forceinline__ void tsdf_shift_array(const unsigned* __restrict__ src, unsigned* __restrict__ dst, const TsdfShiftGroup& G, long long delta, unsigned init) {
    uint4 v = make_uint4(init, init, init, init);
    if (G.mode == kTsdfShiftRow) {
        const unsigned* p = src + (G.g + delta);
        if ((delta & 3) == 0) v = *reinterpret_cast<const V4*>(p);
        else { v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3]; }
    } else if (G.mode == kTsdfShiftMixed) {
        if (G.in & 1) v.x = src[G.at[0]];
        if (G.in & 2) v.y = src[G.at[1]];
        if (G.in & 4) v.z = src[G.at[2]];
        if (G.in & 8) v.w = src[G.at[3]];
    }
    *reinterpret_cast<V4*>(dst + G.g) = v;
}

template <bool kColour>
__global__ __launch_bounds__(256) void tsdf_shift_kernel(TsdfShiftDev P) {
    const long long groups = P.n / 4, stride = (long long)gridDim.x * blockDim.x;  // whole groups
    const long long delta = ((long long)P.s[2] * P.ny + P.s[1]) * P.nx + P.s[0];   // source index - destination index wherever both lie in the grid
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
        TsdfShiftGroup G;
        G.g = 4 * q;
        G.in = 0;
        const unsigned gu = (unsigned)G.g, row = gu / (unsigned)P.nx, k = row / (unsigned)P.ny;
        const int i = (int)(gu - row * (unsigned)P.nx), j = (int)(row - k * (unsigned)P.ny);
        const int si = i + P.s[0], sj = j + P.s[1], sk = (int)k + P.s[2];
        const bool one_row = i + 3 < P.nx, row_in = sj >= 0 && sj < P.ny && sk >= 0 && sk < P.nz;
        if (one_row && (!row_in || si + 3 < 0 || si >= P.nx)) G.mode = kTsdfShiftInit;
        else if (one_row && si >= 0 && si + 3 < P.nx) G.mode = kTsdfShiftRow;      // row_in holds here: the branch above took the rest
        else {
            G.mode = kTsdfShiftMixed;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (tsdf_shift_source(P, gu + (unsigned)e, G.at[e])) G.in |= 1 << e;
        }
        tsdf_shift_array<uint4>(P.src_tsdf, P.dst_tsdf, G, delta, 0x3F800000u);   // 1.0f
        tsdf_shift_array<uint4>(P.src_weight, P.dst_weight, G, delta, 0u);
        if constexpr (kColour) {
#pragma unroll
            for (int X = 0; X < 3; ++X) tsdf_shift_array<TsdfWords4>(P.src_col + (size_t)X * P.n, P.dst_col + (size_t)X * P.n, G, delta, 0u);
        }
    }
    // the n % 4 voxels behind the last whole group
    if (blockIdx.x == 0 && (long long)threadIdx.x < P.n - 4 * groups) {
        const long long idx = 4 * groups + threadIdx.x;
        long long at;
        const bool in = tsdf_shift_source(P, (unsigned)idx, at);
        P.dst_tsdf[idx] = in ? P.src_tsdf[at] : 0x3F800000u;
        P.dst_weight[idx] = in ? P.src_weight[at] : 0u;
        if constexpr (kColour) {
#pragma unroll
            for (int X = 0; X < 3; ++X) P.dst_col[(size_t)X * P.n + idx] = in ? P.src_col[(size_t)X * P.n + at] : 0u;
        }
    }
}
int tsdf_shift_launch(nalo_ctx* c, const TsdfShiftDev& D) {
    if (D.n < 1 || D.n > (1LL << 29) || D.n != (long long)D.nx * D.ny * D.nz) return fail(c, NALO_ERR_ARG, "tsdf_shift_launch: bad grid");
    for (int a = 0; a < 3; ++a) { const int n = a == 0 ? D.nx : a == 1 ? D.ny : D.nz; if (D.s[a] > n || D.s[a] < -n) return fail(c, NALO_ERR_ARG, "tsdf_shift_launch: shift not clamped"); }
    const long long want = std::max<long long>((D.n / 4 + 255) / 256, 1);        // memory-bound: at most 2048 workgroups, the rest by the grid stride
    ProfScope ps(c, "tsdf_shift");
    if (D.src_col) tsdf_shift_kernel<true><<<(unsigned)std::min<long long>(want, 2048), 256, 0, c->stream>>>(D);
    else tsdf_shift_kernel<false><<<(unsigned)std::min<long long>(want, 2048), 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// ---- nalo_tsdf_integrate_frame's plane. A record's key is (its position in the frame's list + 1) << 32 | the bits of its idepth: the maximum per pixel is the
// last record in append order whatever order the lanes arrive in. The resolve pass leaves the key plane zero for the next call.
struct TsdfSegs { const nalo_dense_point* p[kTsdfSegsPerLaunch]; int start[kTsdfSegsPerLaunch + 1]; int nseg; };   // start: list positions; [nseg] = the end
__global__ __launch_bounds__(256) void tsdf_frame_scatter_kernel(TsdfSegs S, unsigned long long* key, int w, int h) {
    const long long ql = (long long)S.start[0] + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ql >= S.start[S.nseg]) return;
    const int q = (int)ql;
    int s = 0;
    while (s + 1 < S.nseg && q >= S.start[s + 1]) ++s;
    const nalo_dense_point r = S.p[s][q - S.start[s]];
    if (r.u >= w || r.v >= h) return;
    atomicMax(&key[(size_t)r.v * w + r.u], ((unsigned long long)(q + 1) << 32) | (unsigned long long)__float_as_uint(r.idepth));
}
// behind every scatter launch: the record whose position the pixel's key holds is the one winner, and it alone stores its colour, packed B | G << 8 | R << 16
__global__ __launch_bounds__(256) void tsdf_frame_colour_kernel(TsdfSegs S, const unsigned long long* key, unsigned* colour, int w, int h) {
    const long long ql = (long long)S.start[0] + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ql >= S.start[S.nseg]) return;
    const int q = (int)ql;
    int s = 0;
    while (s + 1 < S.nseg && q >= S.start[s + 1]) ++s;
    const nalo_dense_point r = S.p[s][q - S.start[s]];
    if (r.u >= w || r.v >= h) return;
    const size_t p = (size_t)r.v * w + r.u;
    if ((unsigned)(key[p] >> 32) == (unsigned)q + 1u) colour[p] = (unsigned)r.bgr[0] | ((unsigned)r.bgr[1] << 8) | ((unsigned)r.bgr[2] << 16);
}
template <bool kColour>
__global__ __launch_bounds__(256) void tsdf_frame_resolve_kernel(unsigned long long* key, float* plane, unsigned* colour, int n) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const unsigned long long k = key[p];
    plane[p] = k ? 1.0f / __uint_as_float((unsigned)(k & 0xFFFFFFFFull)) : 0.0f;
    if (k) key[p] = 0;
    if constexpr (kColour) if (!k) colour[p] = 0;                                 // a pixel without a record is (0, 0, 0)
}
int tsdf_frame_plane_launch(nalo_ctx* c, const MapSeg* segs, int nseg, unsigned long long* key, float* plane, unsigned* colour, int w, int h) {
    for (int pass = 0; pass < (colour ? 2 : 1); ++pass)                           // every scatter is queued before the first colour pass
        for (int s0 = 0; s0 < nseg; s0 += kTsdfSegsPerLaunch) {
            TsdfSegs S{};
            S.nseg = std::min(kTsdfSegsPerLaunch, nseg - s0);
            for (int k = 0; k < S.nseg; ++k) { S.p[k] = static_cast<const nalo_dense_point*>(segs[s0 + k].p); S.start[k] = segs[s0 + k].start; }
            S.start[S.nseg] = segs[s0 + S.nseg - 1].start + segs[s0 + S.nseg - 1].n;
            const int n = S.start[S.nseg] - S.start[0];
            if (n <= 0) continue;
            if (pass == 0) tsdf_frame_scatter_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(S, key, w, h);
            else tsdf_frame_colour_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(S, key, colour, w, h);
            NALO_HIP(c, hipGetLastError());
        }
    const int n = w * h;
    if (colour) tsdf_frame_resolve_kernel<true><<<(n + 255) / 256, 256, 0, c->stream>>>(key, plane, colour, n);
    else tsdf_frame_resolve_kernel<false><<<(n + 255) / 256, 256, 0, c->stream>>>(key, plane, colour, n);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
