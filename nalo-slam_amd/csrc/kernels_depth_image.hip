// CoarseTracker::debugPlotIDepthMap (CoarseTracker.cpp:1263-1359) on the device: the jet-coloured depth image FullSystem::makeKeyFrame hands to
// Output3DWrapper::pushDepthImage (FullSystem.cpp:1408), from the level-0 inverse-depth map of the tracking reference and the planar irradiance of its slot.
//
//  di_fill_kernel<0/1/2>   allID's two order statistics (:1271-1281) WITHOUT the sort: a three-level radix select on the float bit patterns (monotone for
//                          x > 0, +inf included, NaN fails `> 0`): bits 30..20 (2048 bins), 19..9 (2048 bins), 8..0 (512 bins), as ba_th_fill_kernel does for
//                          setNewFrameEnergyTH (kernels_ba.hip). Both ranks ride in the same three passes: level A's histogram is shared, levels B and C keep one
//                          histogram per rank. The ranks (int)(n * 0.05) / (int)(n * 0.95), n = size - 1, are formed on the device from level A's total, so the
//                          count never visits the host. Every workgroup of a pass repeats the (tiny) search of the previous level itself.
//  di_final_kernel         level C's search, then the scalar smoothing of :1283-1313 in one lane, float arithmetic as written.
//  di_paint_kernel         the grey base image (:1318-1323), the plot rule and makeJet3B (:1325-1344, globalFuncs.h:350-367), and setPixelCirc
//                          (MinimalImage.h:112-126) as a GATHER. A plotting source writes the 40 pixels at Chebyshev distance 2 or 3 from it, sources are visited in
//                          raster order and the last writer wins; so output pixel q takes the colour of the plotting source with the largest (y, x) among q - d, d in
//                          that ring, and keeps its grey value when there is none. A 64 x 16 tile of outputs reads the sources of its 3-pixel halo (plot flag + colour
//                          packed in one word, in LDS) and those read idepth with one more pixel of halo for the five-point stencil. No atomics, no scatter.
//
// Conversions the reference leaves undefined are DEFINED (include/nalo_gpu.h): float -> int of the grey value saturates with NaN -> 0 (__float2int_rz), a NaN id
// (maxID == minID, 0 / 0) paints the white pixel x86 produces. The file is compiled without FMA contraction (build.py: NO_CONTRACT).
#include "nalo_internal.h"
#include "plot_device.h"

namespace nalo {

namespace {

constexpr int kDiBinsAB = 2048, kDiBinsC = 512;
// the scratch words (unsigned): histogram A | B of rank 0, 1 | C of rank 0, 1 | state | results
constexpr int kDiOffA = 0, kDiOffB = kDiBinsAB, kDiOffC = kDiOffB + 2 * kDiBinsAB, kDiOffState = kDiOffC + 2 * kDiBinsC, kDiOffRes = kDiOffState + 16;
static_assert(kDiOffRes + 8 == kDepthImageScratchWords, "nalo_internal.h sizes the scratch");
// state: [0] count, per rank r: [1 + 2r] bin A, [2 + 2r] rank below it, [5 + 2r] bin B, [6 + 2r] rank below it
// results: [0] n_positive, [1] min_new, [2] max_new, [3] min_used, [4] max_used, [5] / [6] the rewritten minmax_io pair
constexpr int kDiTW = 64, kDiTH = 16;                       // outputs per workgroup: 256 lanes x 4 rows
constexpr int kDiSW = kDiTW + 6, kDiSH = kDiTH + 6;        // sources: 3 pixels of halo
constexpr int kDiIW = kDiTW + 8, kDiIH = kDiTH + 8;        // idepth: one more for the stencil
constexpr unsigned kDiPlot = 0x80000000u;

template <int LEVEL>
__global__ __launch_bounds__(256) void di_fill_kernel(const float* __restrict__ id, int n, unsigned* __restrict__ scr) {
    constexpr int NB = LEVEL == 2 ? kDiBinsC : kDiBinsAB, NH = LEVEL == 0 ? 1 : 2;
    __shared__ unsigned hist[NH * NB];
    __shared__ unsigned s[8];
    const int tid = threadIdx.x;
    unsigned* const state = scr + kDiOffState;
    unsigned pre[2] = {0u, 0u};
    if (LEVEL == 1) {                                                            // both ranks' search of level A; workgroup 0 keeps the result
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            unsigned total, bin, kres;
            plot_search<kDiBinsAB>(scr + kDiOffA, r, 0u, s, total, bin, kres);
            if (blockIdx.x == 0 && tid == 0) { state[0] = total; state[1 + 2 * r] = bin; state[2 + 2 * r] = kres; }
            pre[r] = bin;
        }
    }
    if (LEVEL == 2) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            unsigned total, bin, kres;
            const unsigned binA = state[1 + 2 * r];                              // written by the previous launch of this stream
            plot_search<kDiBinsAB>(scr + kDiOffB + r * kDiBinsAB, -1, state[2 + 2 * r], s, total, bin, kres);
            if (blockIdx.x == 0 && tid == 0) { state[5 + 2 * r] = bin; state[6 + 2 * r] = kres; }
            pre[r] = (binA << 11) | bin;
        }
    }
    for (int b = tid; b < NH * NB; b += 256) hist[b] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
        const float f = id[i];
        if (!(f > 0.f)) continue;                                                // `if(idepth[lvl][i] > 0)`: NaN, zeros and negatives stay out, +inf goes in
        const unsigned u = __float_as_uint(f);
        if (LEVEL == 0) atomicAdd(&hist[u >> 20], 1u);
        if (LEVEL == 1) {
            if ((u >> 20) == pre[0]) atomicAdd(&hist[(u >> 9) & 2047u], 1u);
            if ((u >> 20) == pre[1]) atomicAdd(&hist[kDiBinsAB + ((u >> 9) & 2047u)], 1u);
        }
        if (LEVEL == 2) {
            if ((u >> 9) == pre[0]) atomicAdd(&hist[u & 511u], 1u);
            if ((u >> 9) == pre[1]) atomicAdd(&hist[kDiBinsC + (u & 511u)], 1u);
        }
    }
    __syncthreads();
    unsigned* const out = scr + (LEVEL == 0 ? kDiOffA : LEVEL == 1 ? kDiOffB : kDiOffC);
    for (int b = tid; b < NH * NB; b += 256) { const unsigned c = hist[b]; if (c) atomicAdd(&out[b], c); }   // integer counts: exact, order independent
}

// level C's search for both ranks, then :1283-1313 in one lane
__global__ __launch_bounds__(256) void di_final_kernel(unsigned* __restrict__ scr, float io_min, float io_max, int have_io) {
    __shared__ unsigned s[8];
    const unsigned* const state = scr + kDiOffState;
    unsigned val[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        unsigned total, bin, kres;
        plot_search<kDiBinsC>(scr + kDiOffC + r * kDiBinsC, -1, state[6 + 2 * r], s, total, bin, kres);
        val[r] = (state[1 + 2 * r] << 20) | (state[5 + 2 * r] << 9) | bin;
    }
    if (threadIdx.x != 0) return;
    unsigned* const res = scr + kDiOffRes;
    const unsigned n = state[0];
    res[0] = n;
    if (n == 0) { for (int i = 1; i < 8; ++i) res[i] = 0u; return; }             // the reference indexes an empty vector here: refused on the host, nothing painted
    const float minID_new = __uint_as_float(val[0]), maxID_new = __uint_as_float(val[1]);
    float minID = minID_new, maxID = maxID_new;
    if (have_io) {
        if (io_min < 0 || io_max < 0) { io_max = maxID; io_min = minID; }
        else {
            const float maxChange = (float)(0.3 * (double)(io_max - io_min));    // `float maxChange = 0.3*(*maxID_pt - *minID_pt);`
            if (minID < io_min - maxChange) minID = io_min - maxChange;
            if (minID > io_min + maxChange) minID = io_min + maxChange;
            if (maxID < io_max - maxChange) maxID = io_max - maxChange;
            if (maxID > io_max + maxChange) maxID = io_max + maxChange;
            io_max = maxID; io_min = minID;
        }
    }
    res[1] = __float_as_uint(minID_new); res[2] = __float_as_uint(maxID_new);
    res[3] = __float_as_uint(minID); res[4] = __float_as_uint(maxID);
    res[5] = __float_as_uint(io_min); res[6] = __float_as_uint(io_max); res[7] = 0u;
}

__global__ __launch_bounds__(256) void di_paint_kernel(const float* __restrict__ id, const float* __restrict__ I, int w, int h, const unsigned* __restrict__ scr, uint8_t* __restrict__ bgr) {
    __shared__ float t_id[kDiIH * kDiIW];
    __shared__ unsigned t_src[kDiSH * kDiSW];
    const unsigned* const res = scr + kDiOffRes;
    if (res[0] == 0u) return;                                                    // no positive value: nothing is painted (uniform over the grid)
    const float minID = __uint_as_float(res[3]), maxID = __uint_as_float(res[4]);
    const int tid = threadIdx.x, x0 = blockIdx.x * kDiTW, y0 = blockIdx.y * kDiTH;
    for (int e = tid; e < kDiIH * kDiIW; e += 256) {
        const int gx = x0 - 4 + e % kDiIW, gy = y0 - 4 + e / kDiIW;
        t_id[e] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? id[(size_t)gy * w + gx] : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < kDiSH * kDiSW; e += 256) {
        const int lx = e % kDiSW, ly = e / kDiSW, sx = x0 - 3 + lx, sy = y0 - 3 + ly;
        unsigned v = 0u;
        if (sx >= 3 && sx < w - 3 && sy >= 3 && sy < h - 3) {                    // :1325-1326; the stencil stays inside the image, hence inside the tile's values
            const float* bp = t_id + (ly + 1) * kDiIW + lx + 1;
            float sid = 0, nid = 0;
            if (bp[0] > 0) { sid += bp[0]; nid++; }
            if (bp[1] > 0) { sid += bp[1]; nid++; }
            if (bp[-1] > 0) { sid += bp[-1]; nid++; }
            if (bp[kDiIW] > 0) { sid += bp[kDiIW]; nid++; }
            if (bp[-kDiIW] > 0) { sid += bp[-kDiIW]; nid++; }
            if (bp[0] > 0 || nid >= 3) v = kDiPlot | plot_jet(((sid / nid) - minID) / ((maxID - minID)));
        }
        t_src[e] = v;
    }
    __syncthreads();
    const int lx = tid & 63, qx = x0 + lx;
    if (qx >= w) return;
#pragma unroll
    for (int j = 0; j < kDiTH / 4; ++j) {
        const int ly = (tid >> 6) + 4 * j, qy = y0 + ly;
        if (qy >= h) continue;
        const size_t q = (size_t)qy * w + qx;
        unsigned col = plot_grey(I[q]);                                          // `int c = dIp[0][i][0]*0.9f;` saturating, NaN -> 0
        // the last writer: sources from raster-last to raster-first, the first that plots wins
        bool hit = false;
        for (int dy = 3; dy >= -3 && !hit; --dy)
            for (int dx = 3; dx >= -3; --dx) {
                if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) continue;        // setPixelCirc leaves the source and its eight neighbours alone
                const unsigned v = t_src[(ly + 3 + dy) * kDiSW + lx + 3 + dx];
                if (v & kDiPlot) { col = v; hit = true; break; }
            }
        bgr[3 * q] = (uint8_t)col; bgr[3 * q + 1] = (uint8_t)(col >> 8); bgr[3 * q + 2] = (uint8_t)(col >> 16);
    }
}

}  // namespace

int depth_image_launch(nalo_ctx* c, const float* idepth, const float* I, float io_min, float io_max, int have_io, unsigned* scr, uint8_t* bgr) {
    const int n = c->w * c->h;
    const int grid = std::min(256, std::max(1, (n + 1023) / 1024));             // one workgroup per CU at most: each flushes its non-empty bins with global atomics
    NALO_HIP(c, hipMemsetAsync(scr, 0, (size_t)kDepthImageScratchWords * 4, c->stream));
    di_fill_kernel<0><<<grid, 256, 0, c->stream>>>(idepth, n, scr);
    di_fill_kernel<1><<<grid, 256, 0, c->stream>>>(idepth, n, scr);
    di_fill_kernel<2><<<grid, 256, 0, c->stream>>>(idepth, n, scr);
    di_final_kernel<<<1, 256, 0, c->stream>>>(scr, io_min, io_max, have_io);
    di_paint_kernel<<<dim3((c->w + kDiTW - 1) / kDiTW, (c->h + kDiTH - 1) / kDiTH), 256, 0, c->stream>>>(idepth, I, c->w, c->h, scr, bgr);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
