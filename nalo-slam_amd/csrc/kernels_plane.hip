// dense=1 / densemap=1: DenseMapping::makeMaskDistMap + fitPlane (reference src/FullSystem/MapPoint.cpp:445-584; call sites MapPoint.cpp:261,280 and
// CoarseTracker.cpp:559,591) on the device: nalo_trk_fit_planes, nalo_dense_fit_planes, nalo_plane_fit_members. include/nalo_gpu.h has the semantics,
// tests/plane_model.py the same in NumPy. Compiled without FMA contraction: the fp32 arithmetic below is the model's, operation for operation.
//
// One call is a chain of launches on the context's stream, and one wait at its end:
//   plane_key        per input point: (int)u, (int)v, the border test, the GUARDED mask read -> a 32-bit key (-0 folded onto +0; NaN and non-members: no key)
//   radix sort       (key, index) pairs, stable (rocPRIM): every cluster becomes one run of the sorted array, its members in ascending input index
//   plane_heads      one record {key, start, count} per run
//   plane_order      ONE workgroup: the reference's alternating sweeps resolved from (min index, max index) of every run - an odd sweep takes the value under the
//                    LAST remaining point, an even one the value under the FIRST - then the stable order by size; offsets, tiles
//   plane_members    one workgroup per cluster: member list in the reference's vector order, rect, back-projection, the cloud compacted in member order
//   plane_score      one workgroup per (cluster, tile of cloud points), the tile staged in LDS: every candidate triplet's inlier count over the tile
//   plane_refine     one workgroup per cluster: first largest count, fp64 centroid and covariance of the winner's inliers, Jacobi eigenvectors, the record
//   (tracker variant with append: trk_append_clusters_kernel, kernels_tracker.hip)
// nalo_trk_fit_ground enqueues the ground pass of setCoarseTrackingRef (CoarseTracker.cpp:582-625, 669-693) behind the refinement, in the same wait:
//   ground_score     one wave per cluster: fitPlane's mid_z, a sum whose bits depend on the member order (ordered_sum.h), and its score (:332, 363-373)
//   ground_choose    ONE wave: the first strictly smallest score, gp_raw, ground_height (:609-616)
//   ground_paint     the winner's member pixels into a w x h bitmap (integer atomicOr), and out of it again once the marking has read it
//   ground_mark      one lane per window point: the pixel under its centerProjectedTo against the bitmap (:675-690)
#include <algorithm>
#include <climits>
#include <cstring>

#include "nalo_internal.h"
#include "ba_device.h"
#include "ordered_sum.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace nalo {

constexpr unsigned kNoKey = 0xFFFFFFFFu;          // a NaN pattern: no cluster has it
constexpr int kPlaneMaxClusters = 2048;           // plane_order resolves the cluster order in LDS
static_assert(kPlaneMaxClusters == kDenseMaxClusters, "nalo_dense_update_map's tables hold one entry per cluster record");
constexpr int kPlaneTile = 1024;                  // cloud points a scoring workgroup stages (12 KB)
constexpr int kPlaneMaxSamples = 4096;
enum { HDR_RAW = 0, HDR_ERR = 1, HDR_MEMBERS = 2, HDR_TILES = 3, HDR_C = 4, HDR_PCN = 5, HDR_NIN = 6, HDR_WORDS = 16 };
enum { PERR_CLUSTERS = 1, PERR_CLOUD_FULL = 4 };

struct PlaneParams {
    const float *u, *v, *idp, *mask;
    int n, w, h, S, min_fit, nfit;                // min_fit = max(min_points, 3); nfit: rows of counts
    float fxi, cxi, fyi, cyi, threshold;
    unsigned *key, *idx, *skey, *sidx;
    int *cluster_of, *order, *raw, *f_start, *f_cnt, *f_desc, *f_off, *tile_start, *hdr, *counts;
    float *cx, *cy, *cz;
    const unsigned* draws;
    nalo_plane_cluster* rec;
};

__global__ __launch_bounds__(256) void plane_key_kernel(PlaneParams P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    const float u = P.u[i], v = P.v[i];
    unsigned key = kNoKey;
    // xx = (int)u > 2 && xx < w - 2  <=>  3 <= u < w - 2 (truncation), and a NaN fails both: the conversion below is always in range, the read always inside
    if (u >= 3.f && u < (float)(P.w - 2) && v >= 3.f && v < (float)(P.h - 2)) {
        const int xx = (int)u, yy = (int)v;
        const float mv = P.mask[xx + (size_t)yy * P.w];
        if (mv == mv) { key = __float_as_uint(mv); if (key == 0x80000000u) key = 0u; }
    }
    P.key[i] = key; P.idx[i] = (unsigned)i; P.cluster_of[i] = -1;
}

__global__ __launch_bounds__(256) void plane_heads_kernel(PlaneParams P) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P.n) return;
    const unsigned k = P.skey[j];
    if (k == kNoKey || (j > 0 && P.skey[j - 1] == k)) return;
    int lo = j + 1, hi = P.n;                      // first position behind j whose key is larger
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.skey[mid] > k) hi = mid; else lo = mid + 1; }
    const int s = atomicAdd(&P.hdr[HDR_RAW], 1);
    if (s < kPlaneMaxClusters) { P.raw[3 * s] = (int)k; P.raw[3 * s + 1] = j; P.raw[3 * s + 2] = lo - j; }
}

__global__ __launch_bounds__(1024) void plane_order_kernel(PlaneParams P) {
    __shared__ int s_min[kPlaneMaxClusters], s_max[kPlaneMaxClusters], s_cnt[kPlaneMaxClusters], s_start[kPlaneMaxClusters];
    __shared__ unsigned s_key[kPlaneMaxClusters];
    __shared__ unsigned short A[kPlaneMaxClusters], B[kPlaneMaxClusters], disc[kPlaneMaxClusters], fin[kPlaneMaxClusters];
    __shared__ unsigned char taken[kPlaneMaxClusters];
    const int tid = threadIdx.x, C = P.hdr[HDR_RAW];
    if (C > kPlaneMaxClusters) { if (tid == 0) { P.hdr[HDR_ERR] |= PERR_CLUSTERS; P.hdr[HDR_C] = C; } return; }
    for (int s = tid; s < C; s += 1024) {
        const int st = P.raw[3 * s + 1], cn = P.raw[3 * s + 2];
        s_key[s] = (unsigned)P.raw[3 * s]; s_start[s] = st; s_cnt[s] = cn; s_min[s] = (int)P.sidx[st]; s_max[s] = (int)P.sidx[st + cn - 1]; taken[s] = 0;
    }
    __syncthreads();
    // A: the runs by their last member, latest first; B: by their first member, earliest first (every index belongs to one run: no ties)
    for (int s = tid; s < C; s += 1024) {
        int ra = 0, rb = 0;
        const int mx = s_max[s], mn = s_min[s];
        for (int j = 0; j < C; ++j) { ra += s_max[j] > mx; rb += s_min[j] < mn; }
        A[ra] = (unsigned short)s; B[rb] = (unsigned short)s;
    }
    __syncthreads();
    if (tid == 0) {
        // sweep k = 0, 2, ... starts at the back of what is left (and leaves the rest reversed), sweep 1, 3, ... therefore at its front (MapPoint.cpp:482-505)
        int pa = 0, pb = 0;
        for (int k = 0; k < C; ++k) {
            int s;
            if ((k & 1) == 0) { while (taken[A[pa]]) ++pa; s = A[pa]; } else { while (taken[B[pb]]) ++pb; s = B[pb]; }
            taken[s] = 1; disc[k] = (unsigned short)s;
        }
    }
    __syncthreads();
    // by size, descending; ties keep discovery order
    for (int k = tid; k < C; k += 1024) {
        const int cn = s_cnt[disc[k]];
        int r = 0;
        for (int j = 0; j < C; ++j) { const int cj = s_cnt[disc[j]]; r += (cj > cn) || (cj == cn && j < k); }
        fin[r] = (unsigned short)k;
    }
    __syncthreads();
    for (int r = tid; r < C; r += 1024) {
        const int k = fin[r], s = disc[k];
        P.f_start[r] = s_start[s]; P.f_cnt[r] = s_cnt[s]; P.f_desc[r] = (k & 1) == 0;
        nalo_plane_cluster c = {};
        c.mask_value = __uint_as_float(s_key[s]); c.n = s_cnt[s]; c.best_sample = -1;
        c.rect[0] = INT_MAX; c.rect[1] = INT_MIN; c.rect[2] = INT_MAX; c.rect[3] = INT_MIN;
        P.rec[r] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int off = 0, tiles = 0;
        for (int r = 0; r < C; ++r) {
            const int cn = s_cnt[disc[fin[r]]];
            P.f_off[r] = off; P.tile_start[r] = tiles;
            off += cn; tiles += (cn + kPlaneTile - 1) / kPlaneTile;
        }
        P.tile_start[C] = tiles;
        P.hdr[HDR_MEMBERS] = off; P.hdr[HDR_TILES] = tiles; P.hdr[HDR_C] = C;
    }
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

__global__ __launch_bounds__(1024) void plane_members_kernel(PlaneParams P) {
    __shared__ int wave_cnt[16], s_base, s_rect[4];
    if (P.hdr[HDR_ERR]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, C = P.hdr[HDR_C];
    for (int r = blockIdx.x; r < C; r += gridDim.x) {
        const int start = P.f_start[r], cnt = P.f_cnt[r], desc = P.f_desc[r], off = P.f_off[r];
        if (tid == 0) { s_base = 0; s_rect[0] = INT_MAX; s_rect[1] = INT_MIN; s_rect[2] = INT_MAX; s_rect[3] = INT_MIN; }
        __syncthreads();
        int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
        for (int c0 = 0; c0 < cnt; c0 += 1024) {
            const int m = c0 + tid;
            bool fin = false; float X = 0.f, Y = 0.f, Z = 0.f;
            if (m < cnt) {
                const int i = (int)P.sidx[desc ? start + cnt - 1 - m : start + m];
                P.order[off + m] = i; P.cluster_of[i] = r;
                const int xx = (int)P.u[i], yy = (int)P.v[i];           // in range: the point passed plane_key's test
                const float id = P.idp[i];
                X = (P.fxi * (float)xx + P.cxi) / id; Y = (P.fyi * (float)yy + P.cyi) / id; Z = 1.f / id;
                fin = finite3(X, Y, Z);
                mnx = min(mnx, xx); mxx = max(mxx, xx); mny = min(mny, yy); mxy = max(mxy, yy);
            }
            const unsigned long long b = __ballot(fin);
            if (lane == 0) wave_cnt[wv] = __popcll(b);
            __syncthreads();
            int at = s_base;
            for (int k = 0; k < wv; ++k) at += wave_cnt[k];
            if (fin) { at += off + __popcll(b & ((1ull << lane) - 1ull)); P.cx[at] = X; P.cy[at] = Y; P.cz[at] = Z; }
            __syncthreads();
            if (tid == 0) { int s = 0; for (int k = 0; k < 16; ++k) s += wave_cnt[k]; s_base += s; }
            __syncthreads();
        }
        if (mnx != INT_MAX) { atomicMin(&s_rect[0], mnx); atomicMax(&s_rect[1], mxx); atomicMin(&s_rect[2], mny); atomicMax(&s_rect[3], mxy); }
        __syncthreads();
        if (tid == 0) { P.rec[r].n_cloud = s_base; for (int k = 0; k < 4; ++k) P.rec[r].rect[k] = s_rect[k]; }
        __syncthreads();
    }
}

// sample i of a cloud of m points: three distinct indices from three draws
__device__ __forceinline__ void plane_triplet(const unsigned* d, unsigned m, int& i0, int& i1, int& i2) {
    unsigned a = d[0] % m, b = d[1] % (m - 1), c = d[2] % (m - 2);
    if (b >= a) ++b;
    const unsigned lo = min(a, b), hi = max(a, b);
    if (c >= lo) ++c;
    if (c >= hi) ++c;
    i0 = (int)a; i1 = (int)b; i2 = (int)c;
}
// the plane through three points: unit normal of (p1 - p0) x (p2 - p0) and d = -n . p0; false for a zero or non-finite length
__device__ __forceinline__ bool plane_sample_model(const float* cx, const float* cy, const float* cz, int i0, int i1, int i2, float4& mdl) {
    const float x0 = cx[i0], y0 = cy[i0], z0 = cz[i0];
    const float ax = cx[i1] - x0, ay = cy[i1] - y0, az = cz[i1] - z0, bx = cx[i2] - x0, by = cy[i2] - y0, bz = cz[i2] - z0;
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!__builtin_isfinite(len) || len == 0.f) return false;
    const float a = nx / len, b = ny / len, c = nz / len;
    mdl = make_float4(a, b, c, -((a * x0 + b * y0) + c * z0));
    return true;
}
__device__ __forceinline__ bool plane_inlier(const float4& m, float x, float y, float z, float th) { return fabsf(((m.x * x + m.y * y) + m.z * z) + m.w) < th; }

__global__ __launch_bounds__(256) void plane_score_kernel(PlaneParams P) {
    __shared__ float sx[kPlaneTile], sy[kPlaneTile], sz[kPlaneTile];
    __shared__ float4 s_mdl[256];
    __shared__ unsigned char s_ok[256];
    if (P.hdr[HDR_ERR]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, C = P.hdr[HDR_C], T = P.hdr[HDR_TILES];
    for (int k = blockIdx.x; k < T; k += gridDim.x) {
        int lo = 0, hi = C - 1;                    // the cluster r with tile_start[r] <= k < tile_start[r + 1]
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (P.tile_start[mid] <= k) lo = mid; else hi = mid - 1; }
        const int r = lo, m = P.rec[r].n_cloud, p0 = (k - P.tile_start[r]) * kPlaneTile;
        if (m < P.min_fit || p0 >= m || r >= P.nfit) continue;          // uniform over the workgroup
        const int np = min(kPlaneTile, m - p0);
        const float *cx = P.cx + P.f_off[r], *cy = P.cy + P.f_off[r], *cz = P.cz + P.f_off[r];
        __syncthreads();
        for (int i = tid; i < np; i += 256) { sx[i] = cx[p0 + i]; sy[i] = cy[p0 + i]; sz[i] = cz[p0 + i]; }
        for (int c0 = 0; c0 < P.S; c0 += 256) {
            __syncthreads();
            const int s = c0 + tid;
            bool ok = false; float4 mdl = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s < P.S) { int i0, i1, i2; plane_triplet(P.draws + 3 * (size_t)s, (unsigned)m, i0, i1, i2); ok = plane_sample_model(cx, cy, cz, i0, i1, i2, mdl); }
            s_mdl[tid] = mdl; s_ok[tid] = ok;
            __syncthreads();
            const int nc = min(256, P.S - c0), npad = (np + 63) & ~63;
            for (int q = wv; q < nc; q += 4) {
                if (!s_ok[q]) continue;
                const float4 md = s_mdl[q];
                int cnt = 0;
                for (int i = lane; i < npad; i += 64) {       // every lane runs every round: the ballot is the wave's
                    const int ii = min(i, np - 1);
                    cnt += __popcll(__ballot(i < np && plane_inlier(md, sx[ii], sy[ii], sz[ii], P.threshold)));
                }
                if (lane == 0 && cnt) atomicAdd(&P.counts[(size_t)r * P.S + c0 + q], cnt);
            }
        }
    }
}

// fixed-order fp64 column sums of per-thread partials: red[t * NC + j] over t = 0 .. 255 by thread j
template <int NC>
__device__ __forceinline__ void plane_reduce(double (&v)[NC], double* red, double (&out)[NC]) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int j = 0; j < NC; ++j) red[tid * NC + j] = v[j];
    __syncthreads();
    if (tid < NC) { double s = 0.0; for (int t = 0; t < 256; ++t) s += red[t * NC + tid]; red[256 * NC + tid] = s; }
    __syncthreads();
    for (int j = 0; j < NC; ++j) out[j] = red[256 * NC + j];
}

// cyclic Jacobi on a symmetric 3x3: 12 sweeps over (0,1), (0,2), (1,2), as tests/plane_model.py
__device__ void plane_jacobi3(double A[3][3], double V[3][3]) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    const int pq[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int sweep = 0; sweep < 12; ++sweep)
        for (int e = 0; e < 3; ++e) {
            const int p = pq[e][0], q = pq[e][1];
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0.0) t = -t;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
            for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
            for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
        }
}

__global__ __launch_bounds__(256) void plane_refine_kernel(PlaneParams P) {
    __shared__ double red[257 * 6];
    __shared__ unsigned long long s_best[256];
    __shared__ float4 s_win;
    if (P.hdr[HDR_ERR]) return;
    const int tid = threadIdx.x, C = P.hdr[HDR_C];
    for (int r = blockIdx.x; r < C; r += gridDim.x) {
        const int m = P.rec[r].n_cloud;
        if (m < P.min_fit || r >= P.nfit) continue;
        const float *cx = P.cx + P.f_off[r], *cy = P.cy + P.f_off[r], *cz = P.cz + P.f_off[r];
        // the first candidate with the largest count among the non-degenerate ones: max of (count + 1) << 32 | ~s
        unsigned long long best = 0ull;
        for (int s = tid; s < P.S; s += 256) {
            int i0, i1, i2; float4 mdl;
            plane_triplet(P.draws + 3 * (size_t)s, (unsigned)m, i0, i1, i2);
            if (!plane_sample_model(cx, cy, cz, i0, i1, i2, mdl)) continue;
            const unsigned long long key = ((unsigned long long)(unsigned)(P.counts[(size_t)r * P.S + s] + 1) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)s);
            best = max(best, key);
        }
        __syncthreads();
        s_best[tid] = best;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) { if (tid < st) s_best[tid] = max(s_best[tid], s_best[tid + st]); __syncthreads(); }
        best = s_best[0];
        if (best == 0ull) continue;                 // every sample degenerate: not fitted (uniform)
        const int win = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)), inl = (int)(best >> 32) - 1;
        if (tid == 0) { int i0, i1, i2; float4 mdl; plane_triplet(P.draws + 3 * (size_t)win, (unsigned)m, i0, i1, i2); plane_sample_model(cx, cy, cz, i0, i1, i2, mdl); s_win = mdl; }
        __syncthreads();
        const float4 md = s_win;
        double pl[4] = {(double)md.x, (double)md.y, (double)md.z, (double)md.w};
        if (inl > 3) {                              // setOptimizeCoefficients(true): the least-squares plane of the winner's inliers (uniform branch)
            double s3[3] = {0.0, 0.0, 0.0}, sum3[3];
            for (int i = tid; i < m; i += 256) { const float x = cx[i], y = cy[i], z = cz[i]; if (plane_inlier(md, x, y, z, P.threshold)) { s3[0] += (double)x; s3[1] += (double)y; s3[2] += (double)z; } }
            plane_reduce<3>(s3, red, sum3);
            const double kk = (double)inl, mx = sum3[0] / kk, my = sum3[1] / kk, mz = sum3[2] / kk;
            double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, c6[6];
            for (int i = tid; i < m; i += 256) {
                const float x = cx[i], y = cy[i], z = cz[i];
                if (plane_inlier(md, x, y, z, P.threshold)) {
                    const double dx = (double)x - mx, dy = (double)y - my, dz = (double)z - mz;
                    s6[0] += dx * dx; s6[1] += dx * dy; s6[2] += dx * dz; s6[3] += dy * dy; s6[4] += dy * dz; s6[5] += dz * dz;
                }
            }
            plane_reduce<6>(s6, red, c6);
            if (tid == 0) {
                double A[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}}, V[3][3];
                plane_jacobi3(A, V);
                int j = 0;
                if (A[1][1] < A[j][j]) j = 1;
                if (A[2][2] < A[j][j]) j = 2;
                double n0 = V[0][j], n1 = V[1][j], n2 = V[2][j];
                const double ln = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
                n0 /= ln; n1 /= ln; n2 /= ln;
                if ((n0 * pl[0] + n1 * pl[1]) + n2 * pl[2] < 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
                pl[0] = n0; pl[1] = n1; pl[2] = n2; pl[3] = -((n0 * mx + n1 * my) + n2 * mz);
            }
        }
        if (tid == 0) {
            nalo_plane_cluster& c = P.rec[r];
            c.fitted = 1; c.best_sample = win; c.inliers = inl;
            for (int k = 0; k < 4; ++k) c.plane[k] = (float)pl[k];
        }
        __syncthreads();
    }
}

// nalo_dense_fit_planes' input, as DenseMapping::updateMap collects it (MapPoint.cpp:246-259): the valid window points of one host in submission order
// (kmap: their device slots in that order, holes included), then the resident immature points of that host in resident order. ONE workgroup, ordered compaction.
__global__ __launch_bounds__(1024) void plane_dense_gather_kernel(const int* __restrict__ kmap, int seg, const float4* __restrict__ geo, const uint8_t* __restrict__ flags,
                                                                  const float* __restrict__ imm, int N, int host, float* __restrict__ ou, float* __restrict__ ov,
                                                                  float* __restrict__ oid, int cap, int* __restrict__ hdr) {
    __shared__ int wave_cnt[16], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    const int total = seg + N;
    for (int c0 = 0; c0 < total; c0 += 1024) {
        const int k = c0 + tid;
        bool take = false; float u = 0.f, v = 0.f, id = 0.f;
        if (k < seg) { const int d = kmap[k]; if (flags[d] & PT_VALID) { const float4 g = geo[d]; u = g.x; v = g.y; id = g.z; take = true; } }
        else if (k < total) {
            const size_t i = (size_t)(k - seg);
            if (__float_as_int(imm[22 * (size_t)N + i]) == host) { u = imm[i]; v = imm[N + i]; id = (imm[24 * (size_t)N + i] + imm[23 * (size_t)N + i]) * 0.5f; take = true; }
        }
        const unsigned long long b = __ballot(take);
        if (lane == 0) wave_cnt[wv] = __popcll(b);
        __syncthreads();
        int at = s_base;
        for (int q = 0; q < wv; ++q) at += wave_cnt[q];
        at += __popcll(b & ((1ull << lane) - 1ull));
        if (take && at < cap) { ou[at] = u; ov[at] = v; oid[at] = id; }
        __syncthreads();
        if (tid == 0) { int s = 0; for (int q = 0; q < 16; ++q) s += wave_cnt[q]; s_base += s; }
        __syncthreads();
    }
    if (tid == 0) hdr[HDR_NIN] = s_base;
}


// ---- the ground pass (nalo_trk_fit_ground). pick words on the device: {ran, cluster, gp_raw[4], ground_height, n_ground_points}, as nalo_ground_pick
struct GroundParams {
    int mark, P, W;
    nalo_ground_score* gs; nalo_ground_pick* pick; unsigned* bits; uint8_t* on;
    const int* kmap; const uint8_t* st_last; const float4* cpt_last; const uint32_t* pt_last;
};

__global__ __launch_bounds__(64) void ground_score_kernel(PlaneParams P, GroundParams G) {
    if (P.hdr[HDR_ERR]) return;
    const int C = P.hdr[HDR_C];
    for (int r = blockIdx.x; r < C; r += gridDim.x) {
        const nalo_plane_cluster c = P.rec[r];
        nalo_ground_score o = {0.f, 0.f, 0};
        if (c.fitted && c.n_cloud == c.n) {                             // uniform: fitPlane returned true
            const float* cz = P.cz + P.f_off[r];                        // every member is in the cloud: cz is in member order
            const float fn = (float)c.n;
            const float mid_z = wave_ordered_sum(0.f, c.n, [&](int i) { return cz[i] / fn; });           // :332
            o.mid_z = mid_z; o.scored = 1;
            if (c.n < 100 || mid_z < 0.f || c.mask_value < 200.f) o.score = 9999999.0f;                 // :363-368
            else o.score = ((c.plane[0] + c.plane[2]) * 1000.0f + fabsf(c.plane[3]) * 100.0f) + (float)(100 / c.n);   // :370-373
        }
        if (threadIdx.x == 0) G.gs[r] = o;
    }
}

__global__ __launch_bounds__(64) void ground_choose_kernel(PlaneParams P, GroundParams G) {
    if (P.hdr[HDR_ERR]) return;
    const int lane = threadIdx.x, C = P.hdr[HDR_C];
    float bs = 3.402823466e+38f; int br = -1;                           // min_score = FLT_MAX (:574)
    if (C >= 4)
        for (int r = lane; r < C; r += 64) { const nalo_ground_score g = G.gs[r]; if (g.scored && g.score < bs) { bs = g.score; br = r; } }
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(bs, o); const int orr = __shfl_xor(br, o);
        if (orr >= 0 && (br < 0 || os < bs || (os == bs && orr < br))) { bs = os; br = orr; }
    }
    if (lane == 0) {
        nalo_ground_pick k = {};
        k.ran = C >= 4; k.cluster = -1;
        if (br >= 0) {
            const nalo_plane_cluster c = P.rec[br];
            const bool flip = c.plane[1] > 0.f;                         // :611
            for (int j = 0; j < 4; ++j) k.gp_raw[j] = flip ? -c.plane[j] : c.plane[j];
            k.ground_height = fabsf(c.plane[3]); k.cluster = br;
        }
        *G.pick = k;
    }
}

// the winner's members (xx, yy) into the bitmap (set = 1) and out of it (set = 0: every set bit of a touched word is one of this list's)
__global__ __launch_bounds__(256) void ground_paint_kernel(PlaneParams P, GroundParams G, int set) {
    if (P.hdr[HDR_ERR]) return;
    const int r = G.pick->cluster;
    if (r < 0) return;
    const int off = P.f_off[r], cnt = P.f_cnt[r];
    for (int m = blockIdx.x * 256 + threadIdx.x; m < cnt; m += gridDim.x * 256) {
        const int i = P.order[off + m];
        const int xx = (int)P.u[i], yy = (int)P.v[i];                   // in range: the point passed plane_key's test
        const unsigned px = (unsigned)xx + (unsigned)yy * (unsigned)P.w;
        if (set) atomicOr(&G.bits[px >> 5], 1u << (px & 31u)); else G.bits[px >> 5] = 0u;
    }
}

__global__ __launch_bounds__(256) void ground_mark_kernel(PlaneParams P, GroundParams G) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (k < G.P && !P.hdr[HDR_ERR] && G.pick->cluster >= 0) {
        const int d = G.kmap[k];
        const uint8_t s = G.st_last[d];
        const uint32_t last = G.pt_last[d];
        // lastResiduals[0].first != 0 && .second == IN (:675), its target the newest frame (:678), and the residual IN at the last fix pass (its rs_cpt is valid).
        // The last clause guards a history the caller planted: a fix pass removes every residual it finds OOB / OUTLIER and nulls the history's pointer to it
        // (ba_hist_update_kernel), so with a maintained history the first two clauses imply it and no test can reach it with the history still saying IN.
        if ((int)(int8_t)(last & 0xFF) == G.W - 1 && ((last >> 16) & 0xFF) == 0u && (s & RS_EXISTS) && (s & RS_STATE_MASK) == 0) {
            const float4 cp = G.cpt_last[d];
            const int u = __float2int_rz(cp.x + 0.5f), v = __float2int_rz(cp.y + 0.5f);              // :679-680
            if (u >= 0 && u < P.w && v >= 0 && v < P.h) { const unsigned px = (unsigned)u + (unsigned)v * (unsigned)P.w; on = (G.bits[px >> 5] >> (px & 31u)) & 1u; }
        }
    }
    if (k < G.P) G.on[k] = on ? 1 : 0;
    const unsigned long long b = __ballot(on);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&G.pick->n_ground_points, __popcll(b));
}

// what nalo_trk_fit_ground adds to plane_run: the caller's arguments, the window's view, and where the results come up
struct GroundRun {
    const nalo_ground_args* g; nalo_ground_pick* pick; GroundWindowView V; const int* k2p;
};
constexpr size_t kGroundPickWords = sizeof(nalo_ground_pick) / 4, kGroundScoreWords = sizeof(nalo_ground_score) / 4;
static_assert(sizeof(nalo_ground_pick) == 32 && sizeof(nalo_ground_score) == 12, "nalo_ground_pick / nalo_ground_score are packed words");

// The whole chain for n input points (u, v, idp device arrays; in_gather: the dense variant's gather is launched first into the call's own input arrays).
// dense_boxes: nalo_dense_update_map's pass over the mask is enqueued behind the fit, so that its boxes come up in the fit's wait.
struct PlaneGather { const int* kmap; int seg; const float4* geo; const uint8_t* flags; const float* imm; int N, host; };
static int plane_run(nalo_ctx* c, const char* who, const float* u, const float* v, const float* idp, const PlaneGather* g, int n, const float* mask,
                     const nalo_plane_fit_args* a, bool append, int cap, nalo_plane_cluster* out, int* n_clusters, bool dense_boxes = false, const GroundRun* gr = nullptr) {
    const std::string W(who);
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "plane_fit");
    const int S = a->n_samples;
    const size_t N = (size_t)std::max(n, 1);
    const int nfit = (int)std::min<size_t>(kPlaneMaxClusters, N / 3 + 1);
    const int capr = std::min(std::max(cap, 0), kPlaneMaxClusters);
    constexpr size_t RW = sizeof(nalo_plane_cluster) / 4;
    // words: 12 arrays of n | raw | f_start f_cnt f_desc f_off | tile_start | hdr | counts | draws | records
    const size_t o_raw = 12 * N, o_f = o_raw + 3 * kPlaneMaxClusters, o_tile = o_f + 4 * kPlaneMaxClusters, o_hdr = o_tile + kPlaneMaxClusters + 1,
                 o_cnt = o_hdr + HDR_WORDS, o_draws = o_cnt + (size_t)nfit * S, o_rec = o_draws + 3 * (size_t)S, o_gpick = o_rec + RW * kPlaneMaxClusters,
                 o_gs = o_gpick + kGroundPickWords, o_gon = o_gs + kGroundScoreWords * kPlaneMaxClusters;
    const int GP = gr && gr->g->mark_window_points ? gr->V.P : 0;     // window points the ground pass marks
    const size_t gon_words = ((size_t)GP + 3) / 4, total = gr ? o_gon + gon_words : o_gpick;
    NALO_HIP(c, c->plane_w.reserve(total));
    const size_t h_ground = 3 * (size_t)S + HDR_WORDS + RW * kPlaneMaxClusters;      // the ground pass' words in the pinned block: pick | scores | bytes
    NALO_HIP(c, c->plane_host.reserve(h_ground + (gr ? kGroundPickWords + kGroundScoreWords * kPlaneMaxClusters + gon_words : 0)));
    const size_t bit_words = ((size_t)c->w * c->h + 31) / 32;
    if (GP > 0 && c->ground_bits.cap < bit_words) {                    // once per context: every call leaves the bitmap all zero
        NALO_HIP(c, c->ground_bits.reserve(bit_words));
        NALO_HIP(c, hipMemsetAsync(c->ground_bits.p, 0, bit_words * 4, c->stream));
    }
    unsigned* wb = c->plane_w.p;
    PlaneParams P;
    P.n = n; P.w = c->w; P.h = c->h; P.S = S; P.min_fit = std::max(a->min_points, 3); P.nfit = nfit; P.threshold = a->threshold; P.mask = mask;
    P.fxi = 1.0f / c->fx[0]; P.cxi = -c->cx[0] / c->fx[0]; P.fyi = 1.0f / c->fy[0]; P.cyi = -c->cy[0] / c->fy[0];     // Ki[0] as trk_append_plane_launch holds it
    P.key = wb; P.idx = wb + N; P.skey = wb + 2 * N; P.sidx = wb + 3 * N; P.cluster_of = (int*)(wb + 4 * N); P.order = (int*)(wb + 5 * N);
    P.cx = (float*)(wb + 6 * N); P.cy = (float*)(wb + 7 * N); P.cz = (float*)(wb + 8 * N);
    float *iu = (float*)(wb + 9 * N), *iv = (float*)(wb + 10 * N), *iid = (float*)(wb + 11 * N);
    P.u = g ? iu : u; P.v = g ? iv : v; P.idp = g ? iid : idp;
    P.raw = (int*)(wb + o_raw); P.f_start = (int*)(wb + o_f); P.f_cnt = P.f_start + kPlaneMaxClusters; P.f_desc = P.f_cnt + kPlaneMaxClusters; P.f_off = P.f_desc + kPlaneMaxClusters;
    P.tile_start = (int*)(wb + o_tile); P.hdr = (int*)(wb + o_hdr); P.counts = (int*)(wb + o_cnt); P.draws = wb + o_draws; P.rec = (nalo_plane_cluster*)(wb + o_rec);
    int* hst = c->plane_host.p;
    std::memcpy(hst, a->draws, 3 * (size_t)S * 4);
    NALO_HIP(c, hipMemsetAsync(P.hdr, 0, (HDR_WORDS + (size_t)nfit * S) * 4, c->stream));
    NALO_HIP(c, hipMemcpyAsync(wb + o_draws, hst, 3 * (size_t)S * 4, hipMemcpyHostToDevice, c->stream));
    c->plane_last_n = -1;
    if (n > 0) {
        if (g) plane_dense_gather_kernel<<<1, 1024, 0, c->stream>>>(g->kmap, g->seg, g->geo, g->flags, g->imm, g->N, g->host, iu, iv, iid, n, P.hdr);
        const int nb = (n + 255) / 256;
        plane_key_kernel<<<nb, 256, 0, c->stream>>>(P);
        size_t tmp = 0;
        NALO_HIP(c, rocprim::radix_sort_pairs(nullptr, tmp, P.key, P.skey, P.idx, P.sidx, (size_t)n, 0, 32, c->stream));
        NALO_HIP(c, c->plane_sort.reserve(tmp + 256));
        NALO_HIP(c, rocprim::radix_sort_pairs(c->plane_sort.p, tmp, P.key, P.skey, P.idx, P.sidx, (size_t)n, 0, 32, c->stream));
        plane_heads_kernel<<<nb, 256, 0, c->stream>>>(P);
        plane_order_kernel<<<1, 1024, 0, c->stream>>>(P);
        plane_members_kernel<<<256, 1024, 0, c->stream>>>(P);
        plane_score_kernel<<<512, 256, 0, c->stream>>>(P);
        plane_refine_kernel<<<256, 256, 0, c->stream>>>(P);
        NALO_HIP(c, hipGetLastError());
        if (gr) {
            ProfScope ps(c, "ground_pass");
            GroundParams G = {};
            G.mark = GP > 0; G.P = GP; G.W = gr->V.W; G.gs = (nalo_ground_score*)(wb + o_gs); G.pick = (nalo_ground_pick*)(wb + o_gpick); G.bits = c->ground_bits.p;
            G.on = (uint8_t*)(wb + o_gon); G.kmap = gr->V.kmap; G.st_last = gr->V.st_last; G.cpt_last = gr->V.cpt_last; G.pt_last = gr->V.pt_last;
            ground_score_kernel<<<256, 64, 0, c->stream>>>(P, G);
            ground_choose_kernel<<<1, 64, 0, c->stream>>>(P, G);
            if (GP > 0) {
                ground_paint_kernel<<<64, 256, 0, c->stream>>>(P, G, 1);
                ground_mark_kernel<<<(GP + 255) / 256, 256, 0, c->stream>>>(P, G);
                ground_paint_kernel<<<64, 256, 0, c->stream>>>(P, G, 0);
            }
            NALO_HIP(c, hipGetLastError());
        }
        if (append) {
            const FrameSlot& s = c->slots[c->slot_ref];
            const int rc = trk_append_clusters_launch(c, s.mask.p, s.dI[0].p, P.rec, P.hdr, capr); if (rc) return rc;
        }
    }
    if (dense_boxes) { const int rc = dense_boxes_enqueue(c, mask, P.rec, P.hdr + HDR_C, capr); if (rc) return rc; }
    int* h_hdr = hst + 3 * (size_t)S;
    NALO_HIP(c, hipMemcpyAsync(h_hdr, P.hdr, HDR_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    if (capr > 0) NALO_HIP(c, hipMemcpyAsync(h_hdr + HDR_WORDS, P.rec, (size_t)capr * sizeof(nalo_plane_cluster), hipMemcpyDeviceToHost, c->stream));
    int* h_g = hst + h_ground;
    if (gr && n > 0) NALO_HIP(c, hipMemcpyAsync(h_g, wb + o_gpick, (o_gon + gon_words - o_gpick) * 4, hipMemcpyDeviceToHost, c->stream));     // pick | scores | bytes
    NALO_HIP(c, hipStreamSynchronize(c->stream));                       // the call's one wait
    const int C = h_hdr[HDR_C];
    *n_clusters = C;
    if (h_hdr[HDR_ERR] & PERR_CLUSTERS) return fail(c, NALO_ERR_UNSUPPORTED, W + ": more than 2048 distinct mask values under the points (REFUSED, not computed)");
    if (g && n > 0 && h_hdr[HDR_NIN] != n) return fail(c, NALO_ERR_STATE, W + ": the device's point count differs from the host's");
    c->plane_last_n = n; c->plane_last_members = h_hdr[HDR_MEMBERS];
    if (C > cap) return fail(c, NALO_ERR_ARG, W + ": cap too small (*n_clusters holds the need)");
    if (C > 0) std::memcpy(out, h_hdr + HDR_WORDS, (size_t)C * sizeof(nalo_plane_cluster));
    if (gr) {                                                           // fewer than 4 clusters: ran = 0 and nothing else (CoarseTracker.cpp:563-567)
        if (n <= 0 || C < 4) gr->pick->ran = 0;
        else {
            std::memcpy(gr->pick, h_g, sizeof(nalo_ground_pick));
            if (gr->g->scores) std::memcpy(gr->g->scores, h_g + kGroundPickWords, (size_t)C * sizeof(nalo_ground_score));
            if (GP > 0 && gr->g->onground) {
                const uint8_t* on = (const uint8_t*)(h_g + kGroundPickWords + kGroundScoreWords * kPlaneMaxClusters);
                for (int k = 0; k < GP; ++k) gr->g->onground[gr->k2p[k]] = on[k];
            }
        }
    }
    if (append && n > 0) {
        c->pc_n[0] = h_hdr[HDR_PCN];
        if (h_hdr[HDR_ERR] & PERR_CLOUD_FULL) return fail(c, NALO_ERR_STATE, W + ": the level-0 cloud would outgrow its w*h buffer (the clusters before that one were appended)");
    }
    return NALO_OK;
}

static int plane_check_args(nalo_ctx* c, const char* who, const nalo_plane_fit_args* a, int cap, const nalo_plane_cluster* out, const int* n_clusters) {
    const std::string W(who);
    if (!a || !n_clusters || cap < 0 || (cap > 0 && !out)) return fail(c, NALO_ERR_ARG, W + ": bad argument");
    if (a->n_samples < 1 || !a->draws) return fail(c, NALO_ERR_ARG, W + ": n_samples < 1 or no draws");
    if (a->n_samples > kPlaneMaxSamples) return fail(c, NALO_ERR_ARG, W + ": more than 4096 samples");
    if (!(a->threshold >= 0.f)) return fail(c, NALO_ERR_ARG, W + ": threshold negative or not a number");
    return NALO_OK;
}

// what updateMap collects for window frame host_frame, shared by nalo_dense_fit_planes and nalo_dense_update_map: the refusals, the gather's sources, the count
static int dense_fit_inputs(nalo_ctx* c, const char* who, int host_frame, PlaneGather* g, int* slot, int* n) {
    int n_valid = 0;
    int rc = ba_plane_inputs(c, host_frame, slot, &g->kmap, &g->seg, &n_valid, &g->geo, &g->flags); if (rc) return rc;
    const FrameSlot& s = c->slots[*slot];
    if (!s.valid || !s.mask.p) return fail(c, NALO_ERR_STATE, std::string(who) + ": the frame's slot has no mask (nalo_frame_upload with mask)");
    g->imm = c->imm_res.p; g->N = c->imm_res_n; g->host = host_frame;
    int n_imm = 0;
    if (g->N > 0) {
        if (c->imm_host_h.size() != (size_t)g->N) return fail(c, NALO_ERR_STATE, std::string(who) + ": the resident set has no host copy");
        for (int i = 0; i < g->N; ++i) n_imm += c->imm_host_h[i] == host_frame;
    }
    *n = n_valid + n_imm;
    return NALO_OK;
}

}  // namespace nalo

using namespace nalo;

extern "C" {

int nalo_trk_fit_planes(nalo_ctx* c, const nalo_plane_fit_args* a, int cap, nalo_plane_cluster* out, int* n_clusters) {
    if (!c) return NALO_ERR_ARG;
    int rc = plane_check_args(c, "nalo_trk_fit_planes", a, cap, out, n_clusters); if (rc) return rc;
    *n_clusters = 0;
    if (c->slot_ref < 0 || !c->slots[c->slot_ref].valid || !c->pc_u[0].p || c->pc_n[0] <= 0) return fail(c, NALO_ERR_STATE, "nalo_trk_fit_planes: no level-0 cloud (nalo_trk_set_ref / nalo_trk_set_pc)");
    const FrameSlot& s = c->slots[c->slot_ref];
    if (!s.mask.p) return fail(c, NALO_ERR_STATE, "nalo_trk_fit_planes: the reference frame was uploaded without a mask");
    return plane_run(c, "nalo_trk_fit_planes", c->pc_u[0].p, c->pc_v[0].p, c->pc_id[0].p, nullptr, c->pc_n[0], s.mask.p, a, a->append != 0, cap, out, n_clusters);
}

int nalo_trk_fit_ground(nalo_ctx* c, const nalo_plane_fit_args* a, const nalo_ground_args* g, int cap, nalo_plane_cluster* out, int* n_clusters, nalo_ground_pick* pick) {
    if (!c) return NALO_ERR_ARG;
    if (!g || !pick) return fail(c, NALO_ERR_ARG, "nalo_trk_fit_ground: ground arguments and pick are required");
    int rc = plane_check_args(c, "nalo_trk_fit_ground", a, cap, out, n_clusters); if (rc) return rc;
    if (c->slot_ref < 0 || !c->slots[c->slot_ref].valid || !c->pc_u[0].p || c->pc_n[0] <= 0) return fail(c, NALO_ERR_STATE, "nalo_trk_fit_ground: no level-0 cloud (nalo_trk_set_ref / nalo_trk_set_pc)");
    const FrameSlot& s = c->slots[c->slot_ref];
    if (!s.mask.p) return fail(c, NALO_ERR_STATE, "nalo_trk_fit_ground: the reference frame was uploaded without a mask");
    GroundRun gr = {};
    gr.g = g; gr.pick = pick;
    if (g->mark_window_points) {
        rc = ba_ground_inputs(c, &gr.V, &gr.k2p); if (rc) return rc;
        if (g->onground && g->onground_cap < gr.V.P) return fail(c, NALO_ERR_ARG, "nalo_trk_fit_ground: onground_cap is below the window's point count");
    }
    *n_clusters = 0;
    return plane_run(c, "nalo_trk_fit_ground", c->pc_u[0].p, c->pc_v[0].p, c->pc_id[0].p, nullptr, c->pc_n[0], s.mask.p, a, a->append != 0, cap, out, n_clusters, false, &gr);
}

int nalo_dense_fit_planes(nalo_ctx* c, int host_frame, const nalo_plane_fit_args* a, int cap, nalo_plane_cluster* out, int* n_clusters) {
    if (!c) return NALO_ERR_ARG;
    int rc = plane_check_args(c, "nalo_dense_fit_planes", a, cap, out, n_clusters); if (rc) return rc;
    *n_clusters = 0;
    PlaneGather g = {};
    int slot = -1, n = 0;
    rc = dense_fit_inputs(c, "nalo_dense_fit_planes", host_frame, &g, &slot, &n); if (rc) return rc;
    return plane_run(c, "nalo_dense_fit_planes", nullptr, nullptr, nullptr, &g, n, c->slots[slot].mask.p, a, false, cap, out, n_clusters);
}

int nalo_dense_update_map(nalo_ctx* c, int host_frame, const nalo_plane_fit_args* a, const double camToWorld[12], int cap, nalo_plane_cluster* clusters,
                          nalo_dense_run* runs, int* n_clusters, int* n_appended) {
    if (!c) return NALO_ERR_ARG;
    int rc = plane_check_args(c, "nalo_dense_update_map", a, cap, clusters, n_clusters); if (rc) return rc;
    *n_clusters = 0;
    if (!camToWorld || !n_appended || !runs) return fail(c, NALO_ERR_ARG, "nalo_dense_update_map: camToWorld, runs and n_appended are required");
    *n_appended = 0;
    if (!map_dense_on(c)) return fail(c, NALO_ERR_STATE, "nalo_dense_update_map: the dense archive is not enabled (nalo_map_dense_enable)");
    PlaneGather g = {};
    int slot = -1, n = 0;
    rc = dense_fit_inputs(c, "nalo_dense_update_map", host_frame, &g, &slot, &n); if (rc) return rc;
    // room for every point the call can keep, before anything is touched
    DenseArchiveView V;
    rc = map_dense_reserve(c, dense_candidates_bound(c->w, c->h), &V); if (rc) return rc;
    rc = plane_run(c, "nalo_dense_update_map", nullptr, nullptr, nullptr, &g, n, c->slots[slot].mask.p, a, false, cap, clusters, n_clusters, true); if (rc) return rc;
    const int frame_id = ba_frame_id(c, host_frame);
    int n_runs = 0;
    rc = dense_update_finish(c, slot, clusters, *n_clusters, camToWorld, V, map_dense_frame_points(c, frame_id), runs, n_appended, &n_runs);
    if (rc) { *n_appended = 0; return rc; }
    map_dense_commit(c, frame_id, *n_appended, n_runs);
    return NALO_OK;
}

int nalo_plane_fit_members(nalo_ctx* c, int cap, int* cluster_of, int* order) {
    if (!c || cap < 0) return fail(c, NALO_ERR_ARG, "nalo_plane_fit_members: bad argument");
    if (c->plane_last_n < 0) return fail(c, NALO_ERR_STATE, "nalo_plane_fit_members: no completed nalo_trk_fit_planes / nalo_dense_fit_planes");
    const int n = c->plane_last_n;
    if (cap < n) return fail(c, NALO_ERR_ARG, "nalo_plane_fit_members: cap is below the last call's input count");
    if (n == 0) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    const size_t N = (size_t)n;
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    if (cluster_of) NALO_HIP(c, hipMemcpy(cluster_of, c->plane_w.p + 4 * N, N * 4, hipMemcpyDeviceToHost));
    if (order && c->plane_last_members > 0) NALO_HIP(c, hipMemcpy(order, c->plane_w.p + 5 * N, (size_t)c->plane_last_members * 4, hipMemcpyDeviceToHost));
    return NALO_OK;
}

}  // extern "C"
