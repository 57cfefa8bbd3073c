// nalo_tsdf_raycast's kernel (include/nalo_gpu.h, "The ray-cast"): one lane per pixel marches its ray through the volume at a fixed step and writes depth,
// normal and colour of the first front face. Built WITHOUT FMA contraction: every float expression below is the header's definition, one rounding per
// operation. A wave is an 8 x 8 pixel tile, so its 64 rays stay within a few voxels of each other and the sixteen 4-byte gathers of a sample hit the same
// lines; a workgroup is 16 x 16 pixels. The kernel reads the volume only: no float atomic, no wait between workgroups, the same bytes on every run.
#include <cfloat>

#include "nalo_internal.h"
#include "tsdf_device.h"

namespace nalo {

// the grid coordinate of the point at camera-z `z` on the ray
__device__ __forceinline__ void tsdf_rc_point(const TsdfRaycastDev& P, const float d[3], float z, float q[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = P.t[a] + d[a] * z;
        q[a] = ((p - P.g.origin[a]) / P.g.vs) - 0.5f;
    }
}

// A conservative interval [n0, n1] of sample numbers outside which the index test fails: the slab test of the ray against the cell region
// [origin + vs / 2, origin + (dim - 1 / 2) vs], in double, the region widened by a voxel and by 1e-5 of the magnitudes that enter p and q (the float rounding of
// the definition's p, q and z_n is below 1e-6 of them), the interval by two steps either side, clipped to [0, N). Empty: n0 > n1.
__device__ __forceinline__ void tsdf_rc_interval(const TsdfRaycastDev& P, const float d[3], int& n0, int& n1) {
    n0 = 0; n1 = -1;
    const int dim[3] = {P.g.nx, P.g.ny, P.g.nz};
    const double zl = (double)P.min_depth + (double)(P.N - 1) * (double)P.step;
    double zlo = -1e300, zhi = 1e300;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(fabsf(d[a]) <= FLT_MAX) || dim[a] < 2) return;                     // a direction that is not finite makes every p, hence every sample, invalid
        const double o = (double)P.t[a], g = (double)P.g.origin[a], vs = (double)P.g.vs, da = (double)d[a];
        const double m = vs + 1e-5 * (fabs(o) + fabs(g) + fabs(da) * zl + (double)dim[a] * vs);
        const double lo = g + 0.5 * vs - m, hi = g + ((double)dim[a] - 0.5) * vs + m;
        if (da == 0.0) { if (o < lo || o > hi) return; continue; }
        const double z1 = (lo - o) / da, z2 = (hi - o) / da;
        zlo = fmax(zlo, fmin(z1, z2)); zhi = fmin(zhi, fmax(z1, z2));
    }
    const double st = (double)P.step, md = (double)P.min_depth;
    double a = floor((zlo - md) / st) - 2.0, b = ceil((zhi - md) / st) + 2.0;
    if (!(a >= 0.0)) a = 0.0;
    if (!(b <= (double)(P.N - 1))) b = (double)(P.N - 1);
    if (!(a <= b)) return;                                                     // compared as doubles before the conversion
    n0 = (int)a; n1 = (int)b;
}

template <bool kNormals, bool kColour>
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(TsdfRaycastDev P, int gx) {
    __shared__ int wsum[3][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bx = (int)(blockIdx.x % (unsigned)gx), by = (int)(blockIdx.x / (unsigned)gx);   // a one-dimensional grid: a view of 1 x 2^26 has more tile rows than a grid's y holds
    const int u = bx * 16 + (wv & 1) * 8 + (lane & 7), v = by * 16 + (wv >> 1) * 8 + (lane >> 3);
    const bool in_view = u < P.w && v < P.h;       // a lane outside the view loads nothing; it still takes part in the ballots and the reductions
    float d[3] = {0.0f, 0.0f, 0.0f};
    int n = 0, n_end = -1;
    if (in_view) {
        const float rx = ((float)u - P.cx) / P.fx, ry = ((float)v - P.cy) / P.fy;
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = (P.R[3 * a] * rx + P.R[3 * a + 1] * ry) + P.R[3 * a + 2];
        tsdf_rc_interval(P, d, n, n_end);
    }
    // the march. The sample before a lane's interval is invalid by the index test, so a lane starts without a previous sample.
    bool active = in_view && n <= n_end, pv = false;
    float ps = 0.0f, depth = 0.0f;
    int hit = 0, back = 0, nn = 0;
    for (int it = 0; it < P.N; ++it) {
        if (!__ballot(active)) break;
        if (active) {
            const float z = P.min_depth + (float)n * P.step;
            float q[3], S = 0.0f;
            tsdf_rc_point(P, d, z, q);
            const bool ok = tsdf_rc_field<true>(P.g, P.min_weight, P.g.tsdf, q[0], q[1], q[2], S);
            if (ok && pv && ((ps < 0.0f) != (S < 0.0f))) {
                if (!(ps < 0.0f)) {                                            // outside to inside: the front face (-0.0f is outside)
                    hit = 1;
                    const float s = ps / (ps - S);
                    depth = (P.min_depth + (float)(n - 1) * P.step) + P.step * s;
                } else back = 1;                                               // a back face ends the ray
                active = false;
            }
            pv = ok; ps = S;
            if (++n > n_end) active = false;
        }
    }
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    unsigned rgba = 0;
    if (hit) {
        float q[3];
        tsdf_rc_point(P, d, depth, q);
        if constexpr (kNormals) {
            float G[3];
            bool all = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float qp[3] = {q[0], q[1], q[2]}, qm[3] = {q[0], q[1], q[2]}, sp = 0.0f, sm = 0.0f;
                qp[a] = q[a] + 1.0f; qm[a] = q[a] - 1.0f;
                const bool okp = tsdf_rc_field<true>(P.g, P.min_weight, P.g.tsdf, qp[0], qp[1], qp[2], sp), okm = tsdf_rc_field<true>(P.g, P.min_weight, P.g.tsdf, qm[0], qm[1], qm[2], sm);
                all = all && okp && okm;
                G[a] = sp - sm;
            }
            if (all) {
                // sqrtf is the correctly rounded square root here; __fsqrt_rn is not (without OCML_BASIC_ROUNDED_OPERATIONS the header maps it to the native one)
                const float len = sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
                if (len > 0.0f && len <= FLT_MAX) { nrm[0] = G[0] / len; nrm[1] = G[1] / len; nrm[2] = G[2] / len; nn = 1; }
            }
        }
        if constexpr (kColour) {
            float cb = 0.0f, cg = 0.0f, cr = 0.0f;
            rgba = 0xFF000000u;                                                // the index test fails at q*: 0, 0, 0, 255
            if (tsdf_rc_field<false>(P.g, P.min_weight, P.g.col, q[0], q[1], q[2], cb)) {
                (void)tsdf_rc_field<false>(P.g, P.min_weight, P.g.col + P.g.col_plane, q[0], q[1], q[2], cg);
                (void)tsdf_rc_field<false>(P.g, P.min_weight, P.g.col + 2 * P.g.col_plane, q[0], q[1], q[2], cr);
                rgba = tsdf_colour_byte(cr) | (tsdf_colour_byte(cg) << 8) | (tsdf_colour_byte(cb) << 16) | 0xFF000000u;
            }
        }
    }
    if (in_view) {
        const size_t p = (size_t)v * P.w + u;
        P.depth[p] = depth;
        if constexpr (kNormals) { P.normal[3 * p] = nrm[0]; P.normal[3 * p + 1] = nrm[1]; P.normal[3 * p + 2] = nrm[2]; }
        if constexpr (kColour) P.rgba[p] = rgba;
    }
    // the three counts: wave reductions, the four waves through LDS, one atomic per count and workgroup
    for (int s = 32; s > 0; s >>= 1) { hit += __shfl_down(hit, s, 64); back += __shfl_down(back, s, 64); nn += __shfl_down(nn, s, 64); }
    if (lane == 0) { wsum[0][wv] = hit; wsum[1][wv] = back; wsum[2][wv] = nn; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int s = (wsum[threadIdx.x][0] + wsum[threadIdx.x][1]) + (wsum[threadIdx.x][2] + wsum[threadIdx.x][3]);
        if (s) atomicAdd(P.cnt + threadIdx.x, (unsigned long long)s);
    }
}

int tsdf_raycast_launch(nalo_ctx* c, const TsdfRaycastDev& D) {
    if (D.w < 1 || D.h < 1 || D.N < 1 || !D.depth || !D.cnt) return fail(c, NALO_ERR_ARG, "tsdf_raycast_launch: bad view");
    const int gx = (D.w + 15) / 16;
    const long long blocks = (long long)gx * ((D.h + 15) / 16);               // w h <= 2^26: at most 2^22 + 2^18 tiles
    if (blocks > INT32_MAX) return fail(c, NALO_ERR_ARG, "tsdf_raycast_launch: the view needs more workgroups than a grid has");
    const unsigned grid = (unsigned)blocks;
    ProfScope ps(c, "tsdf_raycast");
    if (D.normal && D.rgba) tsdf_raycast_kernel<true, true><<<grid, 256, 0, c->stream>>>(D, gx);
    else if (D.normal) tsdf_raycast_kernel<true, false><<<grid, 256, 0, c->stream>>>(D, gx);
    else if (D.rgba) tsdf_raycast_kernel<false, true><<<grid, 256, 0, c->stream>>>(D, gx);
    else tsdf_raycast_kernel<false, false><<<grid, 256, 0, c->stream>>>(D, gx);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
