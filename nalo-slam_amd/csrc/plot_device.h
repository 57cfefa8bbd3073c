// Device functions the painters share (kernels_depth_image.hip: debugPlotIDepthMap, kernels_window_plot.hip: FullSystem::debugPlot, kernels_init_plot.hip:
// CoarseInitializer::debugPlot, kernels_residual_plot.hip: debugPlotTracking, kernels_map_render.hip: the 3-D panel): the grey base value, the colour maps of
// util/globalFuncs.h, the float -> byte conversion of a colour (kernels_map.hip's clouds too), the two ends of a resolve pass - the key load that leaves the
// plane idle and the packed store -, and the search step of the radix select. Every file that
// includes it is built without FMA contraction (build.py: NO_CONTRACT). Conversions the reference leaves undefined are DEFINED as include/nalo_gpu.h states them.
#pragma once
#include "nalo_internal.h"

namespace nalo {

// `int c = I*0.9f; if(c>255) c=255; Vec3b(c,c,c)`: the float -> int conversion saturates with NaN -> 0 (__float2int_rz), a negative c wraps as int -> unsigned char
// does. The byte on all three channels, byte k of the Vec3b in bits 8k..8k+7.
__device__ __forceinline__ unsigned plot_grey(float I) {
    int c = __float2int_rz(I * 0.9f);
    if (c > 255) c = 255;
    return (unsigned)(unsigned char)c * 0x010101u;
}

// float -> byte of a colour: truncation toward zero, saturated to 0..255, NaN -> 0 (nalo_map_frame_cloud's colours, mode 5 of nalo_map_window_plot)
__device__ __forceinline__ unsigned plot_byte(float x) { return !(x > 0.f) ? 0u : (x >= 255.f ? 255u : (unsigned)(int)x); }

// makeJet3B (globalFuncs.h:350-367): byte k of the Vec3b in bits 8k..8k+7. The branch arithmetic is in double as written; every value lies in [0, 255], so the
// truncation to unsigned char is the one of a non-negative int. NaN fails both comparisons, its (int) conversion is undefined there: DEFINED as white.
__device__ __forceinline__ unsigned plot_jet(float id) {
    if (id <= 0) return 128u;
    if (id >= 1) return 128u << 16;
    if (id != id) return 0xFFFFFFu;
    const int icP = (int)(id * 8);
    const float ifP = (id * 8) - icP;
    auto b = [](double v) { return (unsigned)(int)v; };
    if (icP == 0) return b(255 * (0.5 + 0.5 * ifP));
    if (icP == 1) return 255u | (b(255 * (0.5 * ifP)) << 8);
    if (icP == 2) return 255u | (b(255 * (0.5 + 0.5 * ifP)) << 8);
    if (icP == 3) return b(255 * (1 - 0.5 * ifP)) | (255u << 8) | (b(255 * (0.5 * ifP)) << 16);
    if (icP == 4) return b(255 * (0.5 - 0.5 * ifP)) | (255u << 8) | (b(255 * (0.5 + 0.5 * ifP)) << 16);
    if (icP == 5) return (b(255 * (1 - 0.5 * ifP)) << 8) | (255u << 16);
    if (icP == 6) return (b(255 * (0.5 - 0.5 * ifP)) << 8) | (255u << 16);
    if (icP == 7) return b(255 * (1 - 0.5 * ifP)) << 16;
    return 0xFFFFFFu;
}

// makeRainbow3B (globalFuncs.h:334-348) with freeDebugParam3 = scale. `!(id > 0)` (NaN included) is white. An id that int cannot hold (>= 2^31, +inf) is
// undefined in the reference: DEFINED as the white pixel x86 produces (cvttss2si gives INT_MIN, and INT_MIN % 3 = -2 matches no branch). The bytes are
// 255 * (1 - ifP) and 255 * ifP in float, in [0, 255], truncated.
__device__ __forceinline__ unsigned plot_rainbow(float id, float scale) {
    id *= scale;
    if (!(id > 0)) return 0xFFFFFFu;
    if (id >= 2147483648.f) return 0xFFFFFFu;
    int icP = (int)id;
    const float ifP = id - icP;
    icP = icP % 3;
    const unsigned a = (unsigned)(int)(255 * (1 - ifP)), b = (unsigned)(int)(255 * ifP);
    if (icP == 0) return a | (b << 8);
    if (icP == 1) return (a << 8) | (b << 16);
    return b | (a << 16);
}

// The front end of a resolve pass (256 lanes x 4 pixels, kResolvePix per workgroup; g0: the lane's first pixel, below the plane's padded size): the lane's four keys
// of a KeyPlane<K, FillByte> in 16-byte loads, and the idle value written back only where a key was moved, so that the plane needs no fill before the next call.
template <int FillByte, typename K>
__device__ __forceinline__ void plot_take_keys(K* plane, size_t g0, K key[4]) {
    constexpr K idle = (K)~(K)0 / 0xFF * FillByte;
    constexpr unsigned idle_word = 0x01010101u * FillByte;
    constexpr int NV = sizeof(K) / 4;
    uint4* const kp = reinterpret_cast<uint4*>(plane + g0);
    uint4 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = kp[j];
    __builtin_memcpy(key, v, sizeof(v));
    if ((key[0] ^ idle) | (key[1] ^ idle) | (key[2] ^ idle) | (key[3] ^ idle)) {
#pragma unroll
        for (int j = 0; j < NV; ++j) kp[j] = make_uint4(idle_word, idle_word, idle_word, idle_word);
    }
}

// The four pixels of a lane of a resolve pass (256 lanes x 4 pixels, byte k of a Vec3b in bits 8k..8k+7 of col[]) as 12 bytes {b g r b | g r b g | r b g r}: through
// LDS (stage: 3 x 256 words) they leave the workgroup as 16-byte stores. block: the workgroup's 3 x 1024 bytes of the image. All 256 lanes call.
__device__ __forceinline__ void plot_store4(unsigned* stage, const unsigned col[4], uint8_t* block) {
    const int tid = threadIdx.x;
    stage[3 * tid] = (col[0] & 0xFFFFFFu) | (col[1] << 24);
    stage[3 * tid + 1] = ((col[1] >> 8) & 0xFFFFu) | (col[2] << 16);
    stage[3 * tid + 2] = ((col[2] >> 16) & 0xFFu) | (col[3] << 8);
    __syncthreads();
    if (tid < 192) reinterpret_cast<uint4*>(block)[tid] = reinterpret_cast<const uint4*>(stage)[tid];
}

// allID[(int)(n*0.05)] / allID[(int)(n*0.95)] with n = size - 1: the product in double, truncated. An empty list gives rank 0 (nothing is selected from it).
__device__ __forceinline__ unsigned plot_rank(unsigned total, int which) {
    const int n = (int)total - 1;
    return (unsigned)(int)((double)n * (which == 0 ? 0.05 : 0.95));
}

// the bin of hist[NBINS] whose running count passes k, and k's rank inside that bin (all 256 lanes call; s = 8 shared words). which >= 0: k is that rank of THIS
// histogram's total. An empty histogram gives the last bin.
template <int NBINS>
__device__ __forceinline__ void plot_search(const unsigned* __restrict__ hist, int which, unsigned k_in, unsigned* s, unsigned& total, unsigned& bin, unsigned& kres) {
    constexpr int NB = NBINS / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned cnt[NB], sum = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) { cnt[j] = hist[tid * NB + j]; sum += cnt[j]; }
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    __syncthreads();                                                             // the previous search's words have been read
    if (lane == 63) s[wave] = incl;
    if (tid == 0) { s[4] = (unsigned)(NBINS - 1); s[5] = 0u; }
    __syncthreads();
    unsigned wpre = 0;
    total = s[0] + s[1] + s[2] + s[3];
    for (int i = 0; i < wave; ++i) wpre += s[i];
    const unsigned k = which >= 0 ? plot_rank(total, which) : k_in;
    const unsigned excl = wpre + incl - sum;
    __syncthreads();                                                             // lane 0's defaults stand before the one finder overwrites them
    if (excl <= k && k < excl + sum) {                                           // exactly one lane
        unsigned run = excl; int b = 0; bool found = false;
#pragma unroll
        for (int j = 0; j < NB; ++j) { if (!found && k < run + cnt[j]) { b = j; found = true; } if (!found) run += cnt[j]; }
        s[4] = (unsigned)(tid * NB + b); s[5] = k - run;
    }
    __syncthreads();
    bin = s[4]; kres = s[5];
}

}  // namespace nalo
