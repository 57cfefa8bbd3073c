// CoarseInitializer::debugPlot (FullSystem/CoarseInitializer.cpp:287-335; called at the end of every trackFrame, :280) on the device: the level's irradiance of the
// first frame with a 3x3 square (MinimalImage.h setPixel9) per point, for nalo_init_depth_image (host_init.hip). It reads the initialiser's resident Pnt arrays.
//
//  ip_sum_kernel       :306-316 in ONE wave: n_good (an integer count) and sid, the chain of dependent float adds over the good points in index order
//                      (ordered_sum.h; a point that is not good contributes -0.f, which leaves every float - both zeros and NaN included - as it is), then
//                      fac = (float)n_good / sid in one lane. Nothing visits the host between the sum and the painting.
//  ip_scatter_kernel   one lane per point: its colour (black when it is not good, else makeRainbow3B(iR * fac)) into col[], and the key word of the square's pixels
//                      inside the image raised to index + 1 with an integer atomicMax. Points are painted in ascending index, so the largest key IS the last writer.
//  ip_resolve_kernel   one lane per four pixels: the base value (:300-301) or the winner's colour, between the painters' shared front end and tail
//                      (plot_take_keys, plot_store4: plot_device.h).
//
// No float atomic; the bytes are the same on every run. Built without FMA contraction (build.py: NO_CONTRACT).
#include "nalo_internal.h"
#include "ordered_sum.h"
#include "plot_device.h"

namespace nalo {

namespace {

__global__ __launch_bounds__(64) void ip_sum_kernel(InitPlotDev D) {
    const int lane = threadIdx.x;
    int cnt = 0;
    for (int i = lane; i < D.n; i += 64) cnt += D.good[i] != 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    const float sid = wave_ordered_sum(0.f, D.n, [&](int i) { return D.good[i] ? D.iR[i] : -0.f; });
    if (lane != 0) return;
    D.res[0] = (unsigned)cnt;
    D.res[1] = __float_as_uint(sid);
    D.res[2] = __float_as_uint((float)cnt / sid);                                // `float fac = nid / sid;` nid counts in float, exact below 2^24
    D.res[3] = 0u;
}

__global__ __launch_bounds__(256) void ip_scatter_kernel(InitPlotDev D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D.n) return;
    const float fac = __uint_as_float(D.res[2]);
    D.col[i] = D.good[i] ? plot_rainbow(D.iR[i] * fac, D.rainbow_scale) : 0u;
    // setPixel9((int)(u + 0.5f), (int)(v + 0.5f)): the conversion saturates with NaN -> 0; a centre whose square lies outside the image writes nothing
    const int cu = __float2int_rz(D.u[i] + 0.5f), cv = __float2int_rz(D.v[i] + 0.5f);
    if (cu < -1 || cu > D.w || cv < -1 || cv > D.h) return;
    const unsigned key = (unsigned)i + 1u;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int y = cv + dy;
        if (y < 0 || y >= D.h) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int x = cu + dx;
            if (x < 0 || x >= D.w) continue;                                    // the reference's at() has no bounds check: DEFINED as skipped
            atomicMax(&D.key[(size_t)y * D.w + x], key);
        }
    }
}

__global__ __launch_bounds__(256) void ip_resolve_kernel(InitPlotDev D) {
    __shared__ unsigned stage[3 * 256];
    const size_t npx = (size_t)D.w * D.h;
    const size_t g0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned key[4];
    plot_take_keys<0>(D.key, g0, key);
    float iv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) if (g0 + k < npx) iv[k] = D.dI[g0 + k].x;         // firstFrame->dIp[lvl][i][0]
    unsigned col[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // `Vec3b(I, I, I)`: float -> unsigned char, DEFINED as (unsigned char)__float2int_rz(I) (saturating to int, NaN -> 0, then it wraps)
        col[k] = g0 + k < npx ? (unsigned)(unsigned char)__float2int_rz(iv[k]) * 0x010101u : 0u;
        if (key[k] && g0 + k < npx && key[k] <= (unsigned)D.n) col[k] = D.col[key[k] - 1u];
    }
    plot_store4(stage, col, D.bgr + (size_t)blockIdx.x * (3 * kResolvePix));
}

}  // namespace

int init_plot_launch(nalo_ctx* c, const InitPlotDev& D) {
    {
        ProfScope ps(c, "init_plot_sum");
        ip_sum_kernel<<<1, 64, 0, c->stream>>>(D);
    }
    if (D.n > 0) {
        ProfScope ps(c, "init_plot_scatter");
        ip_scatter_kernel<<<(D.n + 255) / 256, 256, 0, c->stream>>>(D);
    }
    {
        ProfScope ps(c, "init_plot_resolve");
        ip_resolve_kernel<<<(unsigned)(resolve_padded_pixels((size_t)D.w * D.h) / kResolvePix), 256, 0, c->stream>>>(D);
    }
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
