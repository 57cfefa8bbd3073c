// FullSystem::debugPlotTracking (FullSystem/FullSystemDebugStuff.cpp:52-107) with PointFrameResidual::debugPlot (Residuals.cpp:278-302) on the device, for one host
// frame (nalo_ba_residual_plot), and the read-back of PointFrameResidual::projectedTo / state_energy (nalo_ba_get_pattern_projections). Both in host_ba.hip.
//
//  rp_project          the ONE function both use: projectPoint (ResidualProjections.h:47-57) of the eight pattern pixels of a residual slot, from the precalc record
//                      of its (host, target) pair and the point's current inverse depth, in the reference's operation order. ba_linearize's lin_setup
//                      (kernels_ba_lin.hip) holds the same arithmetic but is built WITH FMA contraction inside a kernel tuned to its register budget; it is left alone.
//  rp_get_kernel       one lane per residual slot: the sixteen coordinates and state_energy, or the sentinels of a slot that does not exist or is OOB.
//  rp_scatter_kernel   one lane per (point of the host, window row): row t < W is the residual to that target - its colour into col[] and the key word of every
//                      pattern pixel that passes the guard raised to (the point's position in the host's list + 1) with an integer atomicMax -, row W is the
//                      point's 3x3 square on the host's own image. The list is in painting order, so the largest key IS the last writer.
//  rp_resolve_kernel   one lane per four pixels of all painted images: the brightness-transferred base value (:72-82) or the winner's colour, between the
//                      painters' shared front end and tail (plot_take_keys, plot_store4: plot_device.h).
//
// No float atomic; the bytes are the same on every run. Built without FMA contraction (build.py: NO_CONTRACT).
#include "nalo_internal.h"
#include "ba_device.h"
#include "plot_device.h"

namespace nalo {

namespace {

constexpr uint8_t kRsOOB = 1, kRsOutlier = 2;               // ResState {IN, OOB, OUTLIER} in the state byte's low bits (IN = 0)

// Ku / Kv of the eight pattern pixels: `Vec3f ptp = KRKi * Vec3f(u_pt, v_pt, 1) + Kt * idepth; Ku = ptp[0] / ptp[2]; Kv = ptp[1] / ptp[2];`
__device__ __forceinline__ void rp_project(const float* __restrict__ pc, float pu, float pv, float idepth, float* __restrict__ Ku, float* __restrict__ Kv) {
    constexpr int pdx[8] = NALO_PATTERN_DX, pdy[8] = NALO_PATTERN_DY;                               // util/settings.cpp:297 (ref_constants.h)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float xx = pu + (float)pdx[k], yy = pv + (float)pdy[k];
        const float q0 = ((pc[0] * xx + pc[1] * yy) + pc[2]) + pc[9] * idepth;
        const float q1 = ((pc[3] * xx + pc[4] * yy) + pc[5]) + pc[10] * idepth;
        const float q2 = ((pc[6] * xx + pc[7] * yy) + pc[8]) + pc[11] * idepth;
        Ku[k] = q0 / q2; Kv[k] = q1 / q2;
    }
}

// the slot (row t, device point d) is drawn / read back: its point is valid, the residual exists and is not OOB
__device__ __forceinline__ bool rp_live(const ResidualPlotDev& D, int t, int d, uint8_t& st) {
    st = D.state[(size_t)t * D.Ppad + d];
    return (D.flags[d] & PT_VALID) && (st & RS_EXISTS) && (st & RS_STATE_MASK) != kRsOOB;
}

__global__ __launch_bounds__(256) void rp_get_kernel(ResidualPlotDev D) {
    const int d = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (d >= D.Ppad) return;
    const size_t si = (size_t)t * D.Ppad + d;
    float Ku[8], Kv[8], en = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { Ku[k] = 2.f; Kv[k] = 2.f; }                  // what lin_setup initialises Kus / Kvs with
    uint8_t st;
    if (rp_live(D, t, d, st)) {
        const float4 g = D.geo[d];
        rp_project(D.pre + (size_t)(D.blk_host[d / kBlk] * D.W + t) * kPreStride, g.x, g.y, g.z, Ku, Kv);
        en = D.energy[si].x;
    }
    if (D.proj) {
        float4* const o = reinterpret_cast<float4*>(D.proj + si * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = make_float4(Ku[2 * k], Kv[2 * k], Ku[2 * k + 1], Kv[2 * k + 1]);
    }
    if (D.en_out) D.en_out[si] = en;
}

__global__ __launch_bounds__(256) void rp_scatter_kernel(ResidualPlotDev D) {
    __shared__ int cnt[3];
    const int tid = threadIdx.x, k = blockIdx.x * 256 + tid, t = blockIdx.y;
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();
    const int d = k < D.seg ? D.kmap[k] : -1;
    const bool valid = d >= 0 && (D.flags[d] & PT_VALID);
    const unsigned key = (unsigned)k + 1u;
    if (valid && t == D.W) {                                                    // the point's square on the host's own image (:93)
        atomicAdd(&cnt[0], 1);
        const int out = D.out_of[D.host_row];
        if (out >= 0) {
            const float4 g = D.geo[d];
            D.col[(size_t)out * D.seg + k] = plot_rainbow(kScaleIdepth * g.z, D.rainbow_scale);
            // setPixel9((int)(ph->u + 0.5), (int)(ph->v + 0.5), .): the sums in double; the conversion saturates with NaN -> 0
            const int cu = __double2int_rz((double)g.x + 0.5), cv = __double2int_rz((double)g.y + 0.5);
            if (cu >= -1 && cu <= D.w && cv >= -1 && cv <= D.h) {
                unsigned* const plane = D.key + (size_t)out * D.w * D.h;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    const int y = cv + dy;
                    if (y < 0 || y >= D.h) continue;
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int x = cu + dx;
                        if (x < 0 || x >= D.w) continue;                        // the reference's at() has no bounds check: DEFINED as skipped
                        atomicMax(&plane[(size_t)y * D.w + x], key);
                    }
                }
            }
        }
    }
    uint8_t st;
    if (valid && t < D.W && t != D.host_row && rp_live(D, t, d, st)) {          // r->debugPlot() (Residuals.cpp:278-302); a residual's target is never its host
        const float4 g = D.geo[d];
        float Ku[8], Kv[8];
        rp_project(D.pre + (size_t)(D.host_row * D.W + t) * kPreStride, g.x, g.y, g.z, Ku, Kv);
        const int out = D.out_of[t];
        unsigned cT;
        if (D.energy_mode) {
            // `float rT = 20*sqrt(state_energy/9);` the quotient in float, ::sqrt and the product in double; NaN fails both clamps and gives byte 0 twice
            float rT = (float)(20.0 * __dsqrt_rn((double)(D.energy[(size_t)t * D.Ppad + d].x / 9)));
            if (rT < 0) rT = 0;
            if (rT > 255) rT = 255;
            cT = (plot_byte(255 - rT) << 8) | (plot_byte(rT) << 16);
        } else {
            const uint8_t s = st & RS_STATE_MASK;
            cT = s == 0 ? 0x0000FFu : s == kRsOutlier ? 0xFF0000u : 0xFFFFFFu;  // IN (255, 0, 0), OUTLIER (0, 0, 255), else white; byte k of the Vec3b in bits 8k..8k+7
        }
        if (out >= 0) D.col[(size_t)out * D.seg + k] = cT;
        unsigned* const plane = out >= 0 ? D.key + (size_t)out * D.w * D.h : nullptr;
        const float wM3 = (float)(D.w - 3), hM3 = (float)(D.h - 3);
        int npx = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (!(Ku[i] > 2 && Kv[i] > 2 && Ku[i] < wM3 && Kv[i] < hM3)) continue;
            ++npx;
            const int x = __float2int_rz(Ku[i] + 0.5f), y = __float2int_rz(Kv[i] + 0.5f);   // setPixel1: the guard keeps it inside the image
            if (plane && x >= 0 && x < D.w && y >= 0 && y < D.h) atomicMax(&plane[(size_t)y * D.w + x], key);
        }
        atomicAdd(&cnt[1], 1);
        if (npx) atomicAdd(&cnt[2], npx);
    }
    __syncthreads();
    if (tid < 3 && cnt[tid]) atomicAdd(&D.cnt[tid], cnt[tid]);                  // integer counts: exact, order independent
}

__global__ __launch_bounds__(256) void rp_resolve_kernel(ResidualPlotDev D) {
    __shared__ unsigned stage[3 * 256];
    const size_t npx = (size_t)D.w * D.h, px_total = npx * D.n_frames;
    const size_t g0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned key[4];
    plot_take_keys<0>(D.key, g0, key);
    unsigned col[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        col[k] = 0u;
        if (g0 + k >= px_total) continue;
        const int f = (int)((g0 + k) / npx);
        const size_t q = g0 + k - (size_t)f * npx;
        // `float colL = affL[0] * fd[i][0] + affL[1];` product and sum in double; NaN fails both clamps: DEFINED byte 0
        float colL = (float)(D.aff[f][0] * (double)D.I[f][q] + D.aff[f][1]);
        if (colL < 0) colL = 0;
        if (colL > 255) colL = 255;
        col[k] = plot_byte(colL) * 0x010101u;
        if (key[k] && key[k] <= (unsigned)D.seg) col[k] = D.col[(size_t)f * D.seg + key[k] - 1u];
    }
    plot_store4(stage, col, D.bgr + (size_t)blockIdx.x * (3 * kResolvePix));
}

}  // namespace

int residual_projections_launch(nalo_ctx* c, const ResidualPlotDev& D) {
    ProfScope ps(c, "ba_pattern_projections");
    rp_get_kernel<<<dim3((D.Ppad + 255) / 256, D.W), 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

int residual_plot_launch(nalo_ctx* c, const ResidualPlotDev& D) {
    if (D.seg > 0) {
        ProfScope ps(c, "residual_plot_scatter");
        rp_scatter_kernel<<<dim3((D.seg + 255) / 256, D.W + 1), 256, 0, c->stream>>>(D);
    }
    {
        ProfScope ps(c, "residual_plot_resolve");
        const size_t padded = resolve_padded_pixels((size_t)D.w * D.h * D.n_frames);
        rp_resolve_kernel<<<(unsigned)(padded / kResolvePix), 256, 0, c->stream>>>(D);
    }
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
