// Frame ingest from planes that already live on the device (nalo_frame_ingest_device / nalo_frame_attach, host_api.hip): the sensor frame, the mask and the
// colour image are described by byte strides (nalo_dev_plane), so a pitched region of a larger tensor, an x-strided view, HWC and CHW colour are read where they lie.
//   ingest_dev_kernel   ingest_kernel (kernels_pyramid.hip) with strided addresses: PhotometricUndistorter::processFrame (reference src/util/Undistort.cpp:214-251) +
//                       the remap loop of Undistort::undistort (:435-530), the same operations in the same order (this file: -ffp-contract=off)
//   ingest_f32_kernel   a rectified irradiance image copied to level 0 as 32-bit words (NaN payloads pass)
//   attach_kernel       the INTER_NEAREST resizes of Undistort::undistort_mask (:385-433) for mask and colour, on their own: a slot that already holds a pyramid gets
//                       them without its image being touched (a tracked frame that turned out to be a keyframe, FullSystem.cpp:1113-1132)
// No byte outside a described plane is read: remap entries satisfy x < wOrg - 1, y < hOrg - 1 (nalo_undist_set), so the four taps are pixels of the plane, and the
// 2-pixel load of a row-contiguous plane covers exactly the taps x and x + 1 of one row.
#include "nalo_internal.h"
#include "ingest_device.h"
#include <hip/hip_ext.h>

namespace nalo {

struct IngestDevParams {
    const uint8_t* raw; long long sy, sx;           // the sensor plane: first element, byte strides of a row and of a pixel
    int wOrg, hOrg, w, h;
    const float *G, *vinv; const float2* remapXY;   // as IngestParams: the tables of nalo_undist_set (dense, library-owned)
    float factor;
    float* out_I;
};
template <int DT>
__device__ __forceinline__ unsigned ingest_dev_one(const uint8_t* __restrict__ a) {
    if constexpr (DT == 1) return *a;
    else { uint16_t v; __builtin_memcpy(&v, a, 2); return v; }
}
template <int DT>
__device__ __forceinline__ void ingest_dev_pair(const uint8_t* __restrict__ a, unsigned& lo, unsigned& hi) {      // the elements at a and a + DT with one load
    if constexpr (DT == 1) { uint16_t v; __builtin_memcpy(&v, a, 2); lo = v & 0xFFu; hi = v >> 8; }
    else { uint32_t v; __builtin_memcpy(&v, a, 4); lo = v & 0xFFFFu; hi = v >> 16; }
}
// DT: bytes per pixel (1: NALO_DT_U8, 2: NALO_DT_U16). ROWCONTIG: stride_x == DT, the two taps of a row come with one load as in ingest_kernel; otherwise every
// tap is a load of its own. The order is ingest_kernel's: the response's own load, the remap entries, the taps, the response into LDS, the arithmetic, the stores.
template <int DT, int PHOTO, bool ROWCONTIG>
__global__ __launch_bounds__(256) void ingest_dev_kernel(IngestDevParams P) {
    constexpr int U = kIngestU;
    __shared__ float sG[DT == 1 && PHOTO > 0 ? 256 : 1];
    float g_own = 0.f;
    if constexpr (DT == 1 && PHOTO > 0) g_own = P.G[threadIdx.x];
    auto stage_G = [&]() { if constexpr (DT == 1 && PHOTO > 0) { sG[threadIdx.x] = g_own; __syncthreads(); } };
    const float* __restrict__ Gt = (DT == 1 && PHOTO > 0) ? sG : P.G;
    const int n = P.w * P.h, base = blockIdx.x * (256 * U) + threadIdx.x;
    auto data = [&](unsigned v, float vi) -> float {                       // PhotometricUndistorter::processFrame (Undistort.cpp:224-251) at one original pixel
        if constexpr (PHOTO == 0) return P.factor * (float)v;
        float d = Gt[v];
        if constexpr (PHOTO == 2) d *= vi;
        return d;
    };
    float o[U];
    if (!P.remapXY) {                                                      // passthrough: wOrg x hOrg = w x h
        unsigned v[U]; float vi[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = base + 256 * u, ii = idx < n ? idx : 0;
            const int y = ii / P.w, x = ii - y * P.w;
            v[u] = ingest_dev_one<DT>(P.raw + y * P.sy + x * P.sx);
            vi[u] = PHOTO == 2 ? P.vinv[ii] : 1.f;
        }
        stage_G();
#pragma unroll
        for (int u = 0; u < U; ++u) o[u] = data(v[u], vi[u]);
    } else {
        float2 r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const int idx = base + 256 * u; r[u] = P.remapXY[idx < n ? idx : 0]; }
        unsigned v00[U], v10[U], v01[U], v11[U];
        float2 i0[U], i1[U];
        float xx[U], yy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            xx[u] = r[u].x; yy[u] = r[u].y;
            if (xx[u] < 0) { xx[u] = 0.f; yy[u] = 0.f; }                   // an outside pixel computes on pixel (0, 0) and is zeroed at the end
            const int xxi = (int)xx[u], yyi = (int)yy[u];
            xx[u] -= xxi; yy[u] -= yyi;
            const uint8_t* a = P.raw + yyi * P.sy + xxi * P.sx;
            if constexpr (ROWCONTIG) { ingest_dev_pair<DT>(a, v00[u], v10[u]); ingest_dev_pair<DT>(a + P.sy, v01[u], v11[u]); }
            else {
                v00[u] = ingest_dev_one<DT>(a); v10[u] = ingest_dev_one<DT>(a + P.sx);
                v01[u] = ingest_dev_one<DT>(a + P.sy); v11[u] = ingest_dev_one<DT>(a + P.sy + P.sx);
            }
            const int p = xxi + yyi * P.wOrg;
            i0[u] = make_float2(1.f, 1.f); i1[u] = i0[u];
            if constexpr (PHOTO == 2) { __builtin_memcpy(&i0[u], P.vinv + p, 8); __builtin_memcpy(&i1[u], P.vinv + p + P.wOrg, 8); }
        }
        stage_G();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float xxyy = xx[u] * yy[u];
            o[u] = xxyy * data(v11[u], i1[u].y) + (yy[u] - xxyy) * data(v01[u], i1[u].x) + (xx[u] - xxyy) * data(v10[u], i0[u].y) + (1 - xx[u] - yy[u] + xxyy) * data(v00[u], i0[u].x);
            if (r[u].x < 0) o[u] = 0.f;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int idx = base + 256 * u;
        if (idx >= n) break;
        P.out_I[idx] = o[u];
    }
}

// a rectified w x h irradiance plane -> level 0, word for word (the same four pixels per lane: the loads leave together, then the stores)
__global__ __launch_bounds__(256) void ingest_f32_kernel(const uint8_t* __restrict__ src, long long sy, long long sx, int w, int n, uint32_t* __restrict__ out) {
    constexpr int U = kIngestU;
    const int base = blockIdx.x * (256 * U) + threadIdx.x;
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int idx = base + 256 * u, ii = idx < n ? idx : 0;
        const int y = ii / w, x = ii - y * w;
        __builtin_memcpy(&v[u], src + y * sy + x * sx, 4);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int idx = base + 256 * u;
        if (idx >= n) break;
        out[idx] = v[u];
    }
}

int ingest_dev_launch(nalo_ctx* c, hipStream_t st, const nalo_dev_plane& img, const float* G, const float* vinv, const float2* remapXY, int photometric, float factor, float* out_I) {
    const int n = c->w * c->h, grid = (n + 256 * kIngestU - 1) / (256 * kIngestU);
    ProfScope ps(c, "ingest_dev", true);                                   // dispatch-attached timestamps
    if (img.dtype == NALO_DT_F32) {
        if (ps.a) hipExtLaunchKernelGGL(ingest_f32_kernel, dim3(grid), dim3(256), 0, st, ps.a, ps.b, 0, static_cast<const uint8_t*>(img.ptr), img.stride_y, img.stride_x, c->w, n, reinterpret_cast<uint32_t*>(out_I));
        else ingest_f32_kernel<<<grid, 256, 0, st>>>(static_cast<const uint8_t*>(img.ptr), img.stride_y, img.stride_x, c->w, n, reinterpret_cast<uint32_t*>(out_I));
        NALO_HIP(c, hipGetLastError());
        return NALO_OK;
    }
    IngestDevParams P;
    P.raw = static_cast<const uint8_t*>(img.ptr); P.sy = img.stride_y; P.sx = img.stride_x; P.wOrg = img.w; P.hOrg = img.h; P.w = c->w; P.h = c->h;
    P.G = G; P.vinv = vinv; P.remapXY = remapXY; P.factor = factor; P.out_I = out_I;
    const int dt = img.dtype == NALO_DT_U8 ? 1 : 2;
    const bool rc = img.stride_x == dt;
#define NALO_INGEST_DEV3(D_, P_, R_) do { if (ps.a) hipExtLaunchKernelGGL((ingest_dev_kernel<D_, P_, R_>), dim3(grid), dim3(256), 0, st, ps.a, ps.b, 0, P); else ingest_dev_kernel<D_, P_, R_><<<grid, 256, 0, st>>>(P); } while (0)
#define NALO_INGEST_DEV(D_, P_) do { if (rc) NALO_INGEST_DEV3(D_, P_, true); else NALO_INGEST_DEV3(D_, P_, false); } while (0)
    if (dt == 1) { if (photometric == 0) NALO_INGEST_DEV(1, 0); else if (photometric == 1) NALO_INGEST_DEV(1, 1); else NALO_INGEST_DEV(1, 2); }
    else { if (photometric == 0) NALO_INGEST_DEV(2, 0); else if (photometric == 1) NALO_INGEST_DEV(2, 1); else NALO_INGEST_DEV(2, 2); }
#undef NALO_INGEST_DEV
#undef NALO_INGEST_DEV3
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ mask and colour
struct AttachParams {
    const uint8_t *mask, *col;                      // first elements, or null
    long long msy, msx, csy, csx, cb, cg, cr;       // byte strides; cb / cg / cr: the byte offsets of the B, G and R element inside a source pixel
    int mw, mh, cw, ch, w, h;
    double mifx, mify, cifx, cify;                  // resize_nearest_inv per plane and axis
    uint32_t* out_mask; uint8_t* out_bgr;           // w*h words (float bits), 3*w*h bytes B,G,R
};
template <int MDT>
__device__ __forceinline__ uint32_t attach_mask_word(const uint8_t* __restrict__ a) {
    if constexpr (MDT == NALO_DT_U8) return __float_as_uint((float)*a * 1.0f);                                  // as the ingest pass converts the byte mask
    else if constexpr (MDT == NALO_DT_I32) { int v; __builtin_memcpy(&v, a, 4); return __float_as_uint((float)v); }   // C conversion: round to nearest even
    else { uint32_t v; __builtin_memcpy(&v, a, 4); return v; }                                                 // F32: the word as it is
}
// Every lane owns four consecutive output pixels: the mask leaves as one 16-byte store, the colour as three dwords (12 bytes, 4-byte aligned at 12 * lane). The
// sources are gathers (contiguous at ratio 1). The last lane of an image whose pixel count is no multiple of four stores its 1-3 pixels one by one.
// MDT: the mask's NALO_DT_*, 0 = no mask.
template <int MDT>
__global__ __launch_bounds__(256) void attach_kernel(AttachParams P) {
    const int n = P.w * P.h, i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    int y = i0 / P.w, x = i0 - y * P.w;
    const bool colour = P.col != nullptr;
    uint32_t m[4] = {0, 0, 0, 0};
    unsigned b[4] = {0, 0, 0, 0}, g[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                          // past the end (k >= n - i0) the last pixel is read again and not stored
        if constexpr (MDT != 0) m[k] = attach_mask_word<MDT>(P.mask + resize_nearest_src(y, P.mify, P.mh) * P.msy + resize_nearest_src(x, P.mifx, P.mw) * P.msx);
        if (colour) {
            const uint8_t* a = P.col + resize_nearest_src(y, P.cify, P.ch) * P.csy + resize_nearest_src(x, P.cifx, P.cw) * P.csx;
            b[k] = a[P.cb]; g[k] = a[P.cg]; r[k] = a[P.cr];
        }
        if (i0 + k + 1 < n && ++x == P.w) { x = 0; ++y; }
    }
    if (i0 + 3 < n) {
        if constexpr (MDT != 0) *reinterpret_cast<uint4*>(P.out_mask + i0) = make_uint4(m[0], m[1], m[2], m[3]);
        if (colour) {
            uint32_t* d = reinterpret_cast<uint32_t*>(P.out_bgr + 3 * (size_t)i0);
            d[0] = b[0] | g[0] << 8 | r[0] << 16 | b[1] << 24;
            d[1] = g[1] | r[1] << 8 | b[2] << 16 | g[2] << 24;
            d[2] = r[2] | b[3] << 8 | g[3] << 16 | r[3] << 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (i0 + k >= n) break;
            if constexpr (MDT != 0) P.out_mask[i0 + k] = m[k];
            if (colour) { uint8_t* d = P.out_bgr + 3 * (size_t)(i0 + k); d[0] = (uint8_t)b[k]; d[1] = (uint8_t)g[k]; d[2] = (uint8_t)r[k]; }
        }
    }
}

int attach_launch(nalo_ctx* c, hipStream_t st, const nalo_dev_plane* mask, const nalo_dev_plane* colour, int colour_is_rgb, float* out_mask, uint8_t* out_bgr) {
    if (!mask && !colour) return NALO_OK;
    AttachParams P = {};
    P.w = c->w; P.h = c->h; P.out_mask = reinterpret_cast<uint32_t*>(out_mask); P.out_bgr = out_bgr;
    if (mask) {
        P.mask = static_cast<const uint8_t*>(mask->ptr); P.msy = mask->stride_y; P.msx = mask->stride_x; P.mw = mask->w; P.mh = mask->h;
        P.mifx = resize_nearest_inv(c->w, mask->w); P.mify = resize_nearest_inv(c->h, mask->h);
    }
    if (colour) {
        P.col = static_cast<const uint8_t*>(colour->ptr); P.csy = colour->stride_y; P.csx = colour->stride_x; P.cw = colour->w; P.ch = colour->h;
        P.cg = colour->stride_c; P.cb = colour_is_rgb ? 2 * colour->stride_c : 0; P.cr = colour_is_rgb ? 0 : 2 * colour->stride_c;
        P.cifx = resize_nearest_inv(c->w, colour->w); P.cify = resize_nearest_inv(c->h, colour->h);
    }
    const int n = c->w * c->h, grid = (n + 1023) / 1024;
    ProfScope ps(c, "frame_attach", true);
#define NALO_ATTACH(M_) do { if (ps.a) hipExtLaunchKernelGGL((attach_kernel<M_>), dim3(grid), dim3(256), 0, st, ps.a, ps.b, 0, P); else attach_kernel<M_><<<grid, 256, 0, st>>>(P); } while (0)
    const int mdt = mask ? mask->dtype : 0;
    if (mdt == 0) NALO_ATTACH(0); else if (mdt == NALO_DT_U8) NALO_ATTACH(NALO_DT_U8); else if (mdt == NALO_DT_I32) NALO_ATTACH(NALO_DT_I32); else NALO_ATTACH(NALO_DT_F32);
#undef NALO_ATTACH
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
