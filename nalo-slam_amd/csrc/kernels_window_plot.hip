// FullSystem::debugPlot (FullSystem/FullSystemDebugStuff.cpp:109-358; call site FullSystem.cpp:1412) on the device: one image per window frame, the frame's level-0
// irradiance with a ring (MinimalImage.h:112-126) per point, for nalo_map_window_plot (host_map.hip).
//
//  wp_select_kernel    mode 7 only: allID's two order statistics (:121-136) WITHOUT the sort, then the smoothing of :139-156 in one lane. A three-level radix select
//                      on the float bit patterns made monotone over both signs (negative values: all bits flipped; the others: the sign bit set; -0 < +0, NaN left
//                      out): bits 31..21 (2048 bins), 20..10 (2048 bins), 9..0 (1024 bins). allID is the points of one window (10^3 .. 10^5 values), so ONE
//                      workgroup walks the virtual list three times with its histograms in LDS: no global atomics, no scratch to clear, the count never visits the host.
//  wp_scatter_kernel   one lane per entry of the virtual source list (PlotSeg, nalo_internal.h). A source that is drawn stores its colour in col[] and raises the key
//                      word of the ring's pixels inside the image to (its position in its frame's sublist + 1) with an integer atomicMax. The sublist is laid out in
//                      the reference's painting order, so the largest key IS the last writer; an integer maximum does not depend on arrival order.
//  wp_resolve_kernel   one lane per four pixels of all painted frames: the grey base value (:180-185) or the winner's colour, between the painters' shared front end
//                      and tail (plot_take_keys, plot_store4: plot_device.h). The irradiance in 16-byte loads where a lane's four pixels are one frame's.
//
// No float atomic, no atomic append; the bytes are the same on every run. Built without FMA contraction (build.py: NO_CONTRACT).
#include "nalo_internal.h"
#include "ba_device.h"
#include "imm_ctor_body.h"
#include "plot_device.h"

namespace nalo {

namespace {

struct WpSrc { int kind, widx, fstart, t; float u, v, idepth; };

// entry i of the virtual list: false when it is no source (an invalid slot, an archive record of the other status, an immature point of no window frame)
__device__ __forceinline__ bool wp_fetch(const WindowPlotDev& D, int i, WpSrc& R) {
    if (i >= D.total) return false;
    int lo = 0, hi = D.nseg - 1;                                                // the last segment that starts at or before i (uniform loads)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (D.segs[mid].start <= i) lo = mid; else hi = mid - 1; }
    const PlotSeg sg = D.segs[lo];
    const int t = i - sg.start;
    if (t < 0 || t >= sg.n) return false;
    R.kind = sg.kind; R.widx = sg.widx; R.fstart = sg.fstart; R.t = t;
    if (sg.kind == 0) {                                                         // the resident set (its layout: kernels_imm_carry.hip); the frame is the point's host
        const size_t N = (size_t)D.immN;
        R.widx = ((const int*)(D.imm + 22 * N))[t];
        if (R.widx < 0 || R.widx >= NALO_MAX_WINDOW) return false;
        R.u = D.imm[t]; R.v = D.imm[N + t]; R.idepth = 0.f;
        return true;
    }
    if (sg.kind == 1) {
        const int d = ((const int*)sg.p)[t];
        if (!(D.flags[d] & PT_VALID)) return false;
        const float4 g = D.geo[d];
        R.u = g.x; R.v = g.y; R.idepth = kScaleIdepth * g.z;
        return true;
    }
    const float4* q = reinterpret_cast<const float4*>((const nalo_map_record*)sg.p + t);
    const float4 a = q[0], b = q[1];
    if (__float_as_int(b.y) != sg.kind) return false;
    R.u = a.x; R.v = a.y; R.idepth = a.z;
    return true;
}

// the float's bits as an unsigned that orders like the float (negative < -0 < +0 < positive < +inf)
__device__ __forceinline__ unsigned wp_order_key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float wp_order_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(256) void wp_select_kernel(WindowPlotDev D) {
    __shared__ unsigned hist[2 * 2048];
    __shared__ unsigned s[8];
    const int tid = threadIdx.x;
    unsigned binA[2], kA[2], binB[2], kB[2], val[2], n = 0;
    auto clear = [&](int m) { __syncthreads(); for (int b = tid; b < m; b += 256) hist[b] = 0u; __syncthreads(); };
    // every active, marginalised and out point of every window frame, whatever the mask (:122-132); `if(ph!=0)` has no counterpart
    auto walk = [&](auto&& put) {
        for (int i = tid; i < D.total; i += 256) {
            WpSrc R;
            if (!wp_fetch(D, i, R) || R.idepth != R.idepth) continue;
            put(wp_order_key(R.idepth));
        }
        __syncthreads();
    };
    clear(2048);
    walk([&](unsigned k) { atomicAdd(&hist[k >> 21], 1u); });
#pragma unroll
    for (int r = 0; r < 2; ++r) { unsigned total; plot_search<2048>(hist, r, 0u, s, total, binA[r], kA[r]); n = total; }
    clear(2 * 2048);
    walk([&](unsigned k) {
        if ((k >> 21) == binA[0]) atomicAdd(&hist[(k >> 10) & 2047u], 1u);
        if ((k >> 21) == binA[1]) atomicAdd(&hist[2048 + ((k >> 10) & 2047u)], 1u);
    });
#pragma unroll
    for (int r = 0; r < 2; ++r) { unsigned total; plot_search<2048>(hist + r * 2048, -1, kA[r], s, total, binB[r], kB[r]); }
    clear(2 * 1024);
    walk([&](unsigned k) {
        if ((k >> 10) == ((binA[0] << 11) | binB[0])) atomicAdd(&hist[k & 1023u], 1u);
        if ((k >> 10) == ((binA[1] << 11) | binB[1])) atomicAdd(&hist[1024 + (k & 1023u)], 1u);
    });
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        unsigned total, bin, kres;
        plot_search<1024>(hist + r * 1024, -1, kB[r], s, total, bin, kres);
        val[r] = (binA[r] << 21) | (binB[r] << 10) | bin;
    }
    if (tid != 0) return;
    unsigned* const res = D.res;
    res[0] = n;
    if (n == 0) { for (int i = 1; i < kPlotResWords; ++i) res[i] = 0u; return; } // the reference indexes an empty vector here: refused on the host, nothing painted
    const float minID_new = wp_order_value(val[0]), maxID_new = wp_order_value(val[1]);
    float minID = minID_new, maxID = maxID_new, io_min = D.io_min, io_max = D.io_max;
    if (D.have_io) {                                                             // :139-156
        float maxChange = (float)(0.1 * (double)(io_max - io_min));              // `float maxChange = 0.1*(maxIdJetVisDebug - minIdJetVisDebug);`
        if (io_max < 0 || io_min < 0) maxChange = 1e5f;
        if (minID < io_min - maxChange) minID = io_min - maxChange;
        if (minID > io_min + maxChange) minID = io_min + maxChange;
        if (maxID < io_max - maxChange) maxID = io_max - maxChange;
        if (maxID > io_max + maxChange) maxID = io_max + maxChange;
        io_max = maxID; io_min = minID;
    }
    res[1] = __float_as_uint(minID_new); res[2] = __float_as_uint(maxID_new);
    res[3] = __float_as_uint(minID); res[4] = __float_as_uint(maxID);
    res[5] = __float_as_uint(io_min); res[6] = __float_as_uint(io_max); res[7] = 0u;
}

// the colour of source R under D.mode (:187-312), false when the mode does not draw it
__device__ __forceinline__ bool wp_colour(const WindowPlotDev& D, const WpSrc& R, float minID, float maxID, unsigned& col) {
    constexpr unsigned kWhite = 0xFFFFFFu, kBlack = 0u;
    if (R.kind != 0) {
        if (D.mode == 0) { col = R.kind == 3 ? kWhite : plot_rainbow(R.idepth, D.rainbow_scale); return true; }
        if (D.mode == 1) { col = R.kind == 1 ? plot_rainbow(R.idepth, D.rainbow_scale) : R.kind == 2 ? kBlack : kWhite; return true; }
        if (D.mode == 7 && R.kind != 3) { col = R.kind == 1 ? plot_jet((R.idepth - minID) / ((maxID - minID))) : kBlack; return true; }
        return false;
    }
    const size_t N = (size_t)D.immN;
    const int status = ((const int*)(D.imm + 25 * N))[R.t];
    if (D.mode == 3) {
        if (status != IPS_GOOD && status != IPS_SKIPPED && status != IPS_BADCONDITION) return false;
        const float idmin = D.imm[23 * N + R.t], idmax = D.imm[24 * N + R.t];
        col = !isfinite(idmax) ? kBlack : plot_rainbow((idmin + idmax) * 0.5f, D.rainbow_scale);
        return true;
    }
    if (D.mode == 4) {                                                          // :245-256, byte k of the Vec3b in bits 8k..8k+7
        if (status == IPS_GOOD) col = 0x00FF00u;
        else if (status == IPS_OOB) col = 0x0000FFu;
        else if (status == IPS_OUTLIER) col = 0xFF0000u;
        else if (status == IPS_SKIPPED) col = 0x00FFFFu;
        else if (status == IPS_BADCONDITION) col = kWhite;
        else if (status == IPS_UNINITIALIZED) col = kBlack;
        else return false;
        return true;
    }
    if (D.mode == 5) {
        if (status == IPS_UNINITIALIZED) return false;
        float d = D.quality_scale * (__fsqrt_rn(D.imm[26 * N + R.t]) - 1);
        if (d < 0) d = 0;
        if (d > 1) d = 1;
        col = (plot_byte(d * 255) << 8) | (plot_byte((1 - d) * 255) << 16);
        return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void wp_scatter_kernel(WindowPlotDev D) {
    __shared__ int cnt[4 * NALO_MAX_WINDOW];
    const int tid = threadIdx.x;
    if (tid < 4 * NALO_MAX_WINDOW) cnt[tid] = 0;
    if (blockIdx.x == 0 && tid < 4 * NALO_MAX_WINDOW) D.cnt_next[tid] = 0;       // the NEXT call's counters (two buffers): no fill on the path
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    WpSrc R;
    bool draw = wp_fetch(D, i, R);
    const int out = draw ? D.out_of[R.widx] : -1;
    draw = draw && out >= 0;
    float minID = 0.f, maxID = 0.f;
    if (D.mode == 7) {
        if (D.res[0] == 0u) draw = false;                                       // an empty allID: nothing is painted
        minID = __uint_as_float(D.res[3]); maxID = __uint_as_float(D.res[4]);
    }
    unsigned col = 0u;
    draw = draw && wp_colour(D, R, minID, maxID, col);
    if (draw) {
        atomicAdd(&cnt[4 * out + R.kind], 1);
        D.col[i] = col;
        // setPixelCirc((int)(u + 0.5f), (int)(v + 0.5f)): the conversion saturates with NaN -> 0; a centre whose ring lies outside the image writes nothing
        const int cu = __float2int_rz(R.u + 0.5f), cv = __float2int_rz(R.v + 0.5f);
        if (cu >= -3 && cu <= D.w + 2 && cv >= -3 && cv <= D.h + 2) {
            const unsigned key = (unsigned)(i - R.fstart) + 1u;
            unsigned* const plane = D.key + (size_t)out * D.w * D.h;
            for (int dy = -3; dy <= 3; ++dy) {
                const int y = cv + dy;
                if (y < 0 || y >= D.h) continue;
#pragma unroll
                for (int dx = -3; dx <= 3; ++dx) {
                    const int x = cu + dx;
                    if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) continue;    // the ring leaves the centre and its eight neighbours alone
                    if (x < 0 || x >= D.w) continue;                            // the reference's at() has no bounds check: DEFINED as skipped
                    atomicMax(&plane[(size_t)y * D.w + x], key);
                }
            }
        }
    }
    __syncthreads();
    if (tid < 4 * NALO_MAX_WINDOW && cnt[tid]) atomicAdd(&D.cnt[tid], cnt[tid]);   // integer counts: exact, order independent
}

__global__ __launch_bounds__(256) void wp_resolve_kernel(WindowPlotDev D) {
    __shared__ unsigned stage[3 * 256];
    const size_t npx = (size_t)D.w * D.h, px_total = npx * D.n_frames;
    const size_t g0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned key[4];
    plot_take_keys<0>(D.key, g0, key);
    int f = (int)(g0 / npx);
    size_t q = g0 - (size_t)f * npx;
    float iv[4] = {0.f, 0.f, 0.f, 0.f};
    if (g0 + 4 <= px_total && q + 4 <= npx && (q & 3) == 0) {
        const float4 t = *reinterpret_cast<const float4*>(D.I[f] + q);
        iv[0] = t.x; iv[1] = t.y; iv[2] = t.z; iv[3] = t.w;
    } else {
        int ff = f; size_t qq = q;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (g0 + k < px_total) iv[k] = D.I[ff][qq];
            if (++qq == npx) { qq = 0; ++ff; }
        }
    }
    unsigned col[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        col[k] = g0 + k < px_total ? plot_grey(iv[k]) : 0u;
        if (key[k] && g0 + k < px_total) {
            const int fk = (int)((g0 + k) / npx);
            const long long src = (long long)D.fstart[fk] + (long long)key[k] - 1;
            if (src < D.total) col[k] = D.col[src];
        }
    }
    plot_store4(stage, col, D.bgr + (size_t)blockIdx.x * (3 * kResolvePix));
}

}  // namespace

int window_plot_launch(nalo_ctx* c, const WindowPlotDev& D) {
    if (D.mode == 7) {
        ProfScope ps(c, "window_plot_select");
        wp_select_kernel<<<1, 256, 0, c->stream>>>(D);
    }
    {
        ProfScope ps(c, "window_plot_scatter");
        wp_scatter_kernel<<<std::max(1, (D.total + 255) / 256), 256, 0, c->stream>>>(D);
    }
    {
        ProfScope ps(c, "window_plot_resolve");
        const size_t padded = resolve_padded_pixels((size_t)D.w * D.h * D.n_frames);
        wp_resolve_kernel<<<(unsigned)(padded / kResolvePix), 256, 0, c->stream>>>(D);
    }
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
