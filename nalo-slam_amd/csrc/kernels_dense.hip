// a14 — DenseMapping::updateMap bounding-box scan (reference src/FullSystem/MapPoint.cpp:300-310) and
// DenseMapping::makeMap pixel loop (MapPoint.cpp:362-404) on gfx950.
//   bbox     : integer atomicMin/Max over the mask (order independent)
//   make_map : per pixel of the rect with mask == value and (i%3==0 || j%3==0): plane depth, colour, world point;
//              ordered (raster) stream compaction = count / scan / write, same scheme as the tracker point clouds
//   extent   : the accept test of :403 INCLUDING the reference's order-dependent typos:
//              maxy/maxz are "the last point whose y (z) is strictly above the running minimum", maxima are seeded with
//              FLT_MIN. Done with an in-order prefix-min scan in one block, so the decision equals the serial loop's.
#include <cfloat>
#include <climits>
#include "nalo_internal.h"
#include <hip/hip_ext.h>

namespace nalo {

// Three launches, no host round trip between them (round 3; was seven launches and two synchronisations, ~105 us at 1920x1072):
//   dense_rows_kernel   one workgroup per image row: {min x, max x} of the pixels with mask == value, eight loads in flight per lane, NO atomics (thousands of
//                       atomicMin/Max on four words were what the first versions spent their time on)
//   dense_count_kernel  every workgroup folds the row table into the box (block 0 stores it), then the aggregate of its 2048-pixel chunk of the box:
//                       {kept points, min x, min y, min z, max x of their world coordinates}
//   dense_write_kernel  exclusive prefix of the aggregates in front of the chunk (a block-wide fold of <= nb entries: cheaper than a spinning look-back, whose
//                       agent-scope polling of 380 workgroups cost 100 us here), the points written in raster order, and the accept test of MapPoint.cpp:403:
// the reference's loop keeps float extrema but compares the double coordinate against them, and its maxy / maxz are "the last point whose y (z) is strictly
// above the running minimum" (SURVEY App. C.6). The running minimum after point k is min_{i<=k} (float) y_i (rounding is monotone), so point k qualifies iff
// y_k > (double) min(prefix, (float) y_k), prefix = the chunks in front + an in-order scan inside the workgroup; the largest qualifying index wins (one 64-bit
// atomicMax on {index + 1, float bits} per workgroup; the host decodes the two words).
__global__ __launch_bounds__(256) void dense_rows_kernel(const float* __restrict__ mask, int w, int h, float value, int2* __restrict__ rows /* [h]: min x, max x */) {
    const int y = 2 + blockIdx.x;
    int minx = INT_MAX, maxx = INT_MIN;
    const float* row = mask + (size_t)y * w;
    for (int x0 = 2; x0 < w - 2; x0 += 8 * 256) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int x = x0 + k * 256 + threadIdx.x; v[k] = row[x < w - 2 ? x : 2]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int x = x0 + k * 256 + threadIdx.x; if (x < w - 2 && v[k] == value) { minx = min(minx, x); maxx = max(maxx, x); } }
    }
    __shared__ int sm[4][2];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { minx = min(minx, __shfl_down(minx, o)); maxx = max(maxx, __shfl_down(maxx, o)); }
    if ((threadIdx.x & 63) == 0) { const int wv = threadIdx.x >> 6; sm[wv][0] = minx; sm[wv][1] = maxx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { minx = min(minx, sm[k][0]); maxx = max(maxx, sm[k][1]); }
        rows[y] = make_int2(minx, maxx);
    }
}

struct DenseParams {
    const float* mask; const float* I0; const uint8_t* bgr;
    int w, h;
    const int2* rows;                            // dense_rows_kernel
    int* rect;                                   // {minx, maxx, miny, maxy}: written by block 0 of dense_count_kernel, read by dense_write_kernel and the host
    float p0, p1, p2, p3, pcolor, fxi, fyi, cx, cy;
    double c2w[12];
    float* agg;                                  // [nblocks][8]: {count (int bits), min x, min y, min z, max x} of a chunk's kept points
    unsigned long long* last;                    // [2]: packed (index + 1, float bits) of the last point that qualifies for maxy / maxz (decoded by the host)
    float* out6;                                 // {minx, maxx, miny, maxy, minz, maxz} of the serial loop
    int* n_out;
};
constexpr int kDenseChunk = 1024;    // pixels of the box per workgroup. Round 4: 2048 -> 1024 (twice the workgroups for the 256 CUs: 764 instead of 382 on the 460 x 1700 box of the bench)
// e / rw and e % rw for 0 <= e < 2^24 without the ~40-instruction integer division: float quotient, one correction step either way
struct DnDiv { int rw; float rcp; };
__host__ __device__ __forceinline__ void dn_divmod(const DnDiv& d, int e, int& q, int& r) {
    if (d.rcp == 0.f) { q = e / d.rw; r = e - q * d.rw; return; }          // a box of >= 2^24 pixels: (float) e is no longer exact
    q = (int)((float)e * d.rcp); r = e - q * d.rw;
    if (r < 0) { --q; r += d.rw; } else if (r >= d.rw) { ++q; r -= d.rw; }
}

__device__ __forceinline__ void dn_world(const DenseParams& P, int i, int j, float idepth, double (&m)[3]) {
    float c0 = P.fxi * j + (-P.cx * P.fxi), c1 = P.fyi * i + (-P.cy * P.fyi), c2 = 1.f;       // cP = Ki * (j,i,1) / idepth (float), mP = camToWorld * cP (double)  (:390-394)
    c0 /= idepth; c1 /= idepth; c2 /= idepth;
#pragma unroll
    for (int q = 0; q < 3; ++q) m[q] = P.c2w[q * 4] * (double)c0 + P.c2w[q * 4 + 1] * (double)c1 + P.c2w[q * 4 + 2] * (double)c2 + P.c2w[q * 4 + 3];
}
// which pixels of this lane's R rounds are kept (MapPoint.cpp:366-380); the mask loads are issued together, an out-of-range lane reads pixel (rx0, ry0) and drops it
// Round 4: the chunks run over the CANDIDATES of the box in raster order - the pixels with (i % 3 == 0 || j % 3 == 0), MapPoint.cpp:366 -, not over all its pixels:
// both kernels are bound by the number of vector instructions they issue, and 4 of 9 lanes spent theirs on pixels that can never be kept. A band of three rows
// starting at a row i = 0 (mod 3) holds rw candidates (the whole first row) + cj + cj (the columns j = 0 (mod 3) of the other two); the virtual bands start at
// i0 = ry0 - ry0 % 3, `pre` candidates of the first band lie above the box.
struct DnMap {
    int rx0, rw, cj, j0, i0, B, pre, total; DnDiv dv;
    __host__ __device__ __forceinline__ DnMap(int rx0_, int rx1, int ry0, int ry1, bool any) {           // (host: the block-offset table of nalo_dense_update_map)
        rx0 = any ? rx0_ : 0; rw = any ? rx1 - rx0 : 1;
        j0 = rx0 + (3 - rx0 % 3) % 3;
        cj = any && j0 < rx1 ? (rx1 - 1 - j0) / 3 + 1 : 0;
        B = rw + 2 * cj;
        const int m = any ? ry0 % 3 : 0;
        i0 = (any ? ry0 : 0) - m;
        pre = m == 0 ? 0 : (m == 1 ? rw : rw + cj);
        const int nrows = any ? ry1 - i0 : 0, full = nrows / 3, r = nrows - 3 * full;
        total = any ? full * B + (r >= 1 ? rw : 0) + (r >= 2 ? cj : 0) - pre : 0;
        dv = DnDiv{B, total + pre < (1 << 24) ? 1.0f / (float)B : 0.f};
    }
    __host__ __device__ __forceinline__ void at(int e, int& i, int& j) const {         // candidate e (0 <= e < total) -> pixel (i, j)
        int band, rem; dn_divmod(dv, e + pre, band, rem);
        i = i0 + 3 * band;
        if (rem < rw) j = rx0 + rem;
        else if (rem < rw + cj) { i += 1; j = j0 + 3 * (rem - rw); }
        else { i += 2; j = j0 + 3 * (rem - rw - cj); }
    }
};
// which candidates of this lane's R rounds are kept (MapPoint.cpp:366-380); the mask loads are issued together, an out-of-range lane reads candidate 0 and drops it
template <int R>
__device__ __forceinline__ void dn_keep(const DenseParams& P, const DnMap& M, int b, int tid, bool (&keep)[R], float (&idp)[R], int (&pi)[R], int (&pj)[R]) {
    float mv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = b * kDenseChunk + r * 256 + tid;
        M.at(e < M.total ? e : 0, pi[r], pj[r]);
        mv[r] = P.mask[pj[r] + pi[r] * P.w];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = b * kDenseChunk + r * 256 + tid;
        keep[r] = false; idp[r] = 0.f;
        if (e < M.total) {
            const int i = pi[r], j = pj[r];
            if (mv[r] == P.pcolor) {                                                                                  // (i % 3 == 0 || j % 3 == 0) holds for every candidate
                const float ddepth = P.p0 * (j * P.fxi - P.cx * P.fxi) + P.p1 * (i * P.fyi - P.cy * P.fyi) + P.p2;   // MapPoint.cpp:377
                if (ddepth != 0.f) { const float depth = -P.p3 / ddepth; if (depth != 0.f) { idp[r] = 1.f / depth; keep[r] = true; } }
            }
        }
    }
}
// the aggregate of chunk b of a box: {kept points, min x, min y, min z, max x of their world coordinates} -> agg[b]. Shared by dense_count_kernel
// (nalo_dense_make_map) and dense_count_batch_kernel (nalo_dense_update_map). Every lane of the workgroup calls it; the count comes back on lane 0.
__device__ __forceinline__ int dn_count_chunk(const DenseParams& P, const DnMap& M, int b) {
    constexpr int R = kDenseChunk / 256;
    __shared__ float red[4][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool keep[R]; float idp[R]; int pi[R], pj[R];
    dn_keep<R>(P, M, b, tid, keep, idp, pi, pj);
    int cnt = 0;
    float mnx = FLT_MAX, mny = FLT_MAX, mnz = FLT_MAX, mxx = FLT_MIN;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!keep[r]) continue;
        double m[3]; dn_world(P, pi[r], pj[r], idp[r], m);
        const float fx = (float)m[0];
        mnx = fminf(mnx, fx); mxx = fmaxf(mxx, fx); mny = fminf(mny, (float)m[1]); mnz = fminf(mnz, (float)m[2]);
        ++cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); mnx = fminf(mnx, __shfl_xor(mnx, o)); mny = fminf(mny, __shfl_xor(mny, o)); mnz = fminf(mnz, __shfl_xor(mnz, o)); mxx = fmaxf(mxx, __shfl_xor(mxx, o)); }
    if (lane == 0) { red[wave][0] = __int_as_float(cnt); red[wave][1] = mnx; red[wave][2] = mny; red[wave][3] = mnz; red[wave][4] = mxx; }
    __syncthreads();
    int total = 0;
    if (tid == 0) {
        float* o = P.agg + (size_t)b * 8;
        total = __float_as_int(red[0][0]) + __float_as_int(red[1][0]) + __float_as_int(red[2][0]) + __float_as_int(red[3][0]);
        o[0] = __int_as_float(total);
        o[1] = fminf(fminf(red[0][1], red[1][1]), fminf(red[2][1], red[3][1])); o[2] = fminf(fminf(red[0][2], red[1][2]), fminf(red[2][2], red[3][2]));
        o[3] = fminf(fminf(red[0][3], red[1][3]), fminf(red[2][3], red[3][3])); o[4] = fmaxf(fmaxf(red[0][4], red[1][4]), fmaxf(red[2][4], red[3][4]));
    }
    return total;
}
__global__ __launch_bounds__(256) void dense_count_kernel(DenseParams P) {
    __shared__ int sr[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    // ---- the box from the row table (every workgroup on its own: a few hundred entries from L2, all loads in flight; block 0 publishes it and re-arms `last`).
    // No "last workgroup folds it" scheme: an agent-scope fence per workgroup (__threadfence = L2 write-back) cost 20 us in the row kernel and 80 us here.
    int minx = INT_MAX, maxx = INT_MIN, miny = INT_MAX, maxy = INT_MIN;
    {
        int2 rr[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int y = 2 + tid + 256 * k; rr[k] = P.rows[y < P.h - 2 ? y : 2]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int y = 2 + tid + 256 * k; if (y < P.h - 2 && rr[k].x != INT_MAX) { minx = min(minx, rr[k].x); maxx = max(maxx, rr[k].y); miny = min(miny, y); maxy = max(maxy, y); } }
        for (int y = 2 + tid + 2048; y < P.h - 2; y += 256) { const int2 r = P.rows[y]; if (r.x != INT_MAX) { minx = min(minx, r.x); maxx = max(maxx, r.y); miny = min(miny, y); maxy = max(maxy, y); } }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { minx = min(minx, __shfl_xor(minx, o)); maxx = max(maxx, __shfl_xor(maxx, o)); miny = min(miny, __shfl_xor(miny, o)); maxy = max(maxy, __shfl_xor(maxy, o)); }
    if (lane == 0) { sr[wave][0] = minx; sr[wave][1] = maxx; sr[wave][2] = miny; sr[wave][3] = maxy; }
    __syncthreads();
    const int rx0 = min(min(sr[0][0], sr[1][0]), min(sr[2][0], sr[3][0])), rx1 = max(max(sr[0][1], sr[1][1]), max(sr[2][1], sr[3][1]));
    const int ry0 = min(min(sr[0][2], sr[1][2]), min(sr[2][2], sr[3][2])), ry1 = max(max(sr[0][3], sr[1][3]), max(sr[2][3], sr[3][3]));
    if (b == 0 && tid == 0) { P.rect[0] = rx0; P.rect[1] = rx1; P.rect[2] = ry0; P.rect[3] = ry1; P.last[0] = 0ull; P.last[1] = 0ull; P.n_out[0] = 0; }
    const bool any = rx0 != INT_MAX && rx1 > rx0 && ry1 > ry0;
    const DnMap M(rx0, rx1, ry0, ry1, any);
    const int nb = (M.total + kDenseChunk - 1) / kDenseChunk;
    if (b >= nb) return;
    (void)dn_count_chunk(P, M, b);
}
// inclusive prefix minimum over the 64 lanes of a wave, in lane order, without LDS traffic: Hillis-Steele inside the rows of 16 lanes (DPP row_shr), then the row
// tails handed on (row_bcast:15 into the rows 1 and 3, row_bcast:31 into the rows 2 and 3). Lanes without a source keep FLT_MAX, the identity. Round 4: the write
// kernel is bound by the NUMBER of vector instructions (3 waves per SIMD of ~2600 instructions each = 13 us); the ds_bpermute shuffles (150 per wave) and their
// address arithmetic were the largest removable part.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dn_dpp_min(float v) {
    const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(FLT_MAX), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
    return fminf(v, o);
}
__device__ __forceinline__ float dn_wave_prefix_min(float v) {
    v = dn_dpp_min<0x111, 0xF>(v); v = dn_dpp_min<0x112, 0xF>(v); v = dn_dpp_min<0x114, 0xF>(v); v = dn_dpp_min<0x118, 0xF>(v);     // row_shr:1, 2, 4, 8
    v = dn_dpp_min<0x142, 0xA>(v);                                                                                                  // row_bcast:15 -> rows 1, 3
    v = dn_dpp_min<0x143, 0xC>(v);                                                                                                  // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ float dn_lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
// where a kept point goes. nalo_dense_make_map: five arrays the host copies up; nalo_dense_update_map: one 16-byte nalo_dense_point of the call's scratch
// (u | v << 16, idepth, colour, b | g << 8 | r << 16: one dwordx4 store), `base` = the kept points of the clusters in front
struct DnEmitArrays {
    int cap; int* __restrict__ ou; int* __restrict__ ov; float* __restrict__ oid; float* __restrict__ ocol; uint8_t* __restrict__ obgr;
    __device__ __forceinline__ void operator()(const DenseParams& P, int o, int i, int j, float idp) const {
        if (o < cap) {
            const int px = j + i * P.w;
            ou[o] = j; ov[o] = i; oid[o] = idp; ocol[o] = P.I0[px];                             // = dI[px][0] (makeImages keeps level 0's planar image): 4 instead of 64 bytes of sector traffic per point
            if (P.bgr) { obgr[3 * o] = P.bgr[3 * px]; obgr[3 * o + 1] = P.bgr[3 * px + 1]; obgr[3 * o + 2] = P.bgr[3 * px + 2]; }
        }
    }
};
struct DnEmitRecords {
    uint4* __restrict__ out; long long base, cap;
    __device__ __forceinline__ void operator()(const DenseParams& P, int o, int i, int j, float idp) const {
        const long long q = base + o;
        if (q >= cap) return;                                                                   // (the scratch holds every candidate of the scanned range: never)
        const int px = j + i * P.w;
        unsigned c3 = 0u;
        if (P.bgr) c3 = (unsigned)P.bgr[3 * px] | ((unsigned)P.bgr[3 * px + 1] << 8) | ((unsigned)P.bgr[3 * px + 2] << 16);
        out[q] = make_uint4((unsigned)j | ((unsigned)i << 16), __float_as_uint(idp), __float_as_uint(P.I0[px]), c3);
    }
};
// chunk b of the nb chunks of a box: the exclusive prefix of the aggregates in front (P.agg: the box's own chunks), the points in raster order, the totals of the
// serial loop (P.n_out, P.out6, P.last). Shared by dense_write_kernel (nalo_dense_make_map) and dense_write_batch_kernel (nalo_dense_update_map), so the two routes
// run the same arithmetic; every lane of the workgroup calls it.
template <class Emit>
__device__ __forceinline__ void dn_write_chunk(const DenseParams& P, const DnMap& M, int b, int nb, const Emit& emit) {
    constexpr int R = kDenseChunk / 256;
    __shared__ int cnt[R][4];
    __shared__ float gmin[R][4][2];              // min of (float) y, (float) z per (round, wave) group of kept points
    __shared__ float red[4][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        // ---- exclusive prefix of the chunks in front: count, min x / y / z, max x (order-free folds; the in-order part happens inside the workgroup).
        // The first four strides are loaded together (a rolled loop waits for every load: three dependent L2 round trips for the last chunks of the bench's box)
        int ecnt = 0; float e1 = FLT_MAX, e2 = FLT_MAX, e3 = FLT_MAX, e4 = FLT_MIN;
        {
            float4 a[4]; float a4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int p = tid + 256 * k, pp = p < b ? p : 0; a[k] = *reinterpret_cast<const float4*>(P.agg + (size_t)pp * 8); a4[k] = P.agg[(size_t)pp * 8 + 4]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) if (tid + 256 * k < b) { ecnt += __float_as_int(a[k].x); e1 = fminf(e1, a[k].y); e2 = fminf(e2, a[k].z); e3 = fminf(e3, a[k].w); e4 = fmaxf(e4, a4[k]); }
            for (int p = tid + 1024; p < b; p += 256) {
                const float4 q = *reinterpret_cast<const float4*>(P.agg + (size_t)p * 8); const float q4 = P.agg[(size_t)p * 8 + 4];
                ecnt += __float_as_int(q.x); e1 = fminf(e1, q.y); e2 = fminf(e2, q.z); e3 = fminf(e3, q.w); e4 = fmaxf(e4, q4);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { ecnt += __shfl_xor(ecnt, o); e1 = fminf(e1, __shfl_xor(e1, o)); e2 = fminf(e2, __shfl_xor(e2, o)); e3 = fminf(e3, __shfl_xor(e3, o)); e4 = fmaxf(e4, __shfl_xor(e4, o)); }
        if (lane == 0) { red[wave][0] = __int_as_float(ecnt); red[wave][1] = e1; red[wave][2] = e2; red[wave][3] = e3; red[wave][4] = e4; }
        bool keep[R]; float idp[R]; int rank[R], pi[R], pj[R];
        dn_keep<R>(P, M, b, tid, keep, idp, pi, pj);
        double wy[R], wz[R];                     // world y, z of the kept points (compared as doubles against the float running minima)
        float fyv[R], fzv[R], py[R], pz[R];      // their float values (FLT_MAX: no point) and the inclusive prefix minima over the wave in lane order
#pragma unroll
        for (int r = 0; r < R; ++r) {
            fyv[r] = FLT_MAX; fzv[r] = FLT_MAX; wy[r] = 0; wz[r] = 0;
            if (keep[r]) { double m[3]; dn_world(P, pi[r], pj[r], idp[r], m); wy[r] = m[1]; wz[r] = m[2]; fyv[r] = (float)m[1]; fzv[r] = (float)m[2]; }
            const unsigned long long mk = __ballot(keep[r]);
            rank[r] = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
            py[r] = dn_wave_prefix_min(fyv[r]); pz[r] = dn_wave_prefix_min(fzv[r]);
            const float gy = dn_lane63(py[r]), gz = dn_lane63(pz[r]);          // the wave's minima = the last lane's prefix
            if (lane == 0) { cnt[r][wave] = __popcll(mk); gmin[r][wave][0] = gy; gmin[r][wave][1] = gz; }
        }
        __syncthreads();
        ecnt = __float_as_int(red[0][0]) + __float_as_int(red[1][0]) + __float_as_int(red[2][0]) + __float_as_int(red[3][0]);
        e1 = fminf(fminf(red[0][1], red[1][1]), fminf(red[2][1], red[3][1])); e2 = fminf(fminf(red[0][2], red[1][2]), fminf(red[2][2], red[3][2]));
        e3 = fminf(fminf(red[0][3], red[1][3]), fminf(red[2][3], red[3][3])); e4 = fmaxf(fmaxf(red[0][4], red[1][4]), fmaxf(red[2][4], red[3][4]));
        if (b == nb - 1 && tid == 0) {           // the last chunk: prefix + its own aggregate = the totals of the serial loop (maxy / maxz follow from the last workgroup)
            const float* a = P.agg + (size_t)b * 8;
            P.n_out[0] = ecnt + __float_as_int(a[0]);
            P.out6[0] = fminf(e1, a[1]); P.out6[1] = fmaxf(e4, a[4]); P.out6[2] = fminf(e2, a[2]); P.out6[4] = fminf(e3, a[3]);
        }
        // ---- the points in raster order; the in-order prefix minima decide who may be "the last point above the running minimum"
        int off = ecnt;
        float runy = e2, runz = e3;
        // output index o grows with (round, wave, lane): the last qualifying point of a wave is the highest lane of its highest round with one (two ballots per
        // round instead of a 64-bit max reduction over the lanes)
        unsigned long long q1 = 0ull, q2 = 0ull;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int goff = off; float gy = runy, gz = runz;                     // offset / running minima in front of this (round, wave) group
            for (int k = 0; k < wave; ++k) { goff += cnt[r][k]; gy = fminf(gy, gmin[r][k][0]); gz = fminf(gz, gmin[r][k][1]); }
            bool t1 = false, t2 = false;
            const int o = goff + rank[r];
            if (keep[r]) {
                emit(P, o, pi[r], pj[r], idp[r]);
                const float ry_ = fminf(gy, py[r]), rz_ = fminf(gz, pz[r]);       // the running minima AFTER this point's own update
                t1 = wy[r] > (double)ry_; t2 = wz[r] > (double)rz_;
            }
            const unsigned long long m1 = __ballot(t1), m2 = __ballot(t2);
            if (m1) { const int l = 63 - __clzll(m1); q1 = ((unsigned long long)(unsigned)(__builtin_amdgcn_readlane(o, l) + 1) << 32) | (unsigned)__builtin_amdgcn_readlane(__float_as_int(fyv[r]), l); }
            if (m2) { const int l = 63 - __clzll(m2); q2 = ((unsigned long long)(unsigned)(__builtin_amdgcn_readlane(o, l) + 1) << 32) | (unsigned)__builtin_amdgcn_readlane(__float_as_int(fzv[r]), l); }
            for (int k = 0; k < 4; ++k) { off += cnt[r][k]; runy = fminf(runy, gmin[r][k][0]); runz = fminf(runz, gmin[r][k][1]); }   // this round is behind us
        }
        // the largest qualifying index of the workgroup (nearly every point qualifies: one atomic per LANE was 380 k serialised updates of two words, 88 us)
        __shared__ unsigned long long sq[4][2];
        if (lane == 0) { sq[wave][0] = q1; sq[wave][1] = q2; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; ++k) { q1 = sq[k][0] > q1 ? sq[k][0] : q1; q2 = sq[k][1] > q2 ? sq[k][1] : q2; }
            if (q1) atomicMax(&P.last[0], q1);
            if (q2) atomicMax(&P.last[1], q2);
        }
    }
}
__global__ __launch_bounds__(256) void dense_write_kernel(DenseParams P, int cap, int* __restrict__ ou, int* __restrict__ ov, float* __restrict__ oid, float* __restrict__ ocol,
                                                          uint8_t* __restrict__ obgr) {
    const int b = blockIdx.x;
    const int rx0 = P.rect[0], rx1 = P.rect[1], ry0 = P.rect[2], ry1 = P.rect[3];
    const bool any = rx0 != INT_MAX && rx1 > rx0 && ry1 > ry0;
    const DnMap M(rx0, rx1, ry0, ry1, any);
    const int nb = (M.total + kDenseChunk - 1) / kDenseChunk;
    if (b < nb) dn_write_chunk(P, M, b, nb, DnEmitArrays{cap, ou, ov, oid, ocol, obgr});
}

// ------------------------------------------------------------------------------------------------ nalo_dense_update_map: every cluster of a frame in one batch
// The loop of MapPoint.cpp:271-331 without a launch, a wait or a copied point per cluster:
//   dense_boxes_prep_kernel   ONE workgroup: the fitted call's <= 2048 mask values sorted (rank by counting: they are distinct), the boxes seeded
//   dense_boxes_kernel        ONE pass over the mask for all clusters: a workgroup takes eight rows, holds the sorted values and a box per cluster in LDS; only the
//                             first and the last pixel of a run of equal values look their record up (binary search; -0 == +0, NaN equals nothing) and fold
//                             into the LDS box (integer min / max), and the workgroup flushes the boxes it touched with global integer atomicMin / atomicMax:
//                             order independent, every run gives the same bits
//   (the fit's wait: records and boxes come up; the host sizes the grid: per cluster with a plane and a colour the chunks of its own box, DnMap on the host)
//   dense_count_batch_kernel  a workgroup finds its cluster in the block-offset table, then dn_count_chunk on that cluster's box
//   scan_ints_launch          the chunks' kept counts of ALL clusters: a cluster's points start where the clusters in front end (boxes overlap: sizing the scratch
//                             by candidates per box would not be bounded by the image)
//   dense_write_batch_kernel  dn_write_chunk inside the cluster's segment of the aggregates: prefix minima and "last qualifying point" never cross a cluster
//   dense_decide_kernel       ONE workgroup: n, the accept bit of :403 and the exclusive prefix of the accepted run lengths
//   dense_copy_kernel         the accepted runs from the scratch into the archive's chunks, one 16-byte load and store per point
// No float atomic, no atomic append: order comes from the scans.
// NOT done as first sketched: a uint16 cluster-index plane. dn_keep compares the float mask with the cluster's value exactly as nalo_dense_make_map does, so both
// routes share it unchanged, and the plane's 2 bytes per pixel of writes are saved.
static_assert(sizeof(nalo_dense_point) == 16, "one dwordx4 per dense map point");
constexpr int kDnRowsPerBlock = 8;
struct DenseBatchItem { float plane[4]; float pcolor; int rect[4]; int boff; int pad[2]; };      // one per cluster that runs makeMap's loop; boff: its first workgroup
static_assert(sizeof(DenseBatchItem) == 48, "three 16-byte words");
struct DenseBatch {
    DenseParams P;                                // what every cluster shares (mask, image, calibration, camToWorld)
    const DenseBatchItem* items; int A;
    float* aggs; int* cnt;                        // [NB][8] chunk aggregates; [NB + 1] kept counts per chunk, then their exclusive scan
    float* ext; unsigned long long* last;         // per item: {minx, maxx, miny, -, minz, -, n (int)} and the two packed "last qualifying point" words
    uint4* pts; long long pts_cap;                // the call's scratch: every cluster's kept points, cluster after cluster
    int* res;                                     // per item {n, accept, first point in pts, first point among the appended}; res[4 A] = appended in all
};

__global__ __launch_bounds__(1024) void dense_boxes_prep_kernel(const nalo_plane_cluster* __restrict__ rec, const int* __restrict__ n_clusters, float* __restrict__ svals,
                                                                int* __restrict__ sidx, int* __restrict__ gbox, int* __restrict__ cdev) {
    __shared__ float v[kDenseMaxClusters];
    int C = n_clusters[0];
    if (C < 0 || C > kDenseMaxClusters) C = 0;                                  // (more than 2048 clusters: the call is refused after its wait)
    for (int k = threadIdx.x; k < C; k += 1024) v[k] = rec[k].mask_value;
    __syncthreads();
    for (int k = threadIdx.x; k < C; k += 1024) {
        const float x = v[k];
        int r = 0;
        for (int j = 0; j < C; ++j) r += v[j] < x;
        svals[r] = x; sidx[r] = k;
        gbox[4 * k] = INT_MAX; gbox[4 * k + 1] = INT_MIN; gbox[4 * k + 2] = INT_MAX; gbox[4 * k + 3] = INT_MIN;
    }
    if (threadIdx.x == 0) cdev[0] = C;
}

__global__ __launch_bounds__(256) void dense_boxes_kernel(const float* __restrict__ mask, int w, int h, const int* __restrict__ cdev, const float* __restrict__ svals,
                                                          const int* __restrict__ sidx, int* __restrict__ gbox) {
    __shared__ float sv[kDenseMaxClusters];
    __shared__ unsigned short si[kDenseMaxClusters];
    __shared__ int box[kDenseMaxClusters][4];
    const int C = cdev[0], tid = threadIdx.x;
    if (C <= 0) return;
    for (int k = tid; k < C; k += 256) { sv[k] = svals[k]; si[k] = (unsigned short)sidx[k]; box[k][0] = INT_MAX; box[k][1] = INT_MIN; box[k][2] = INT_MAX; box[k][3] = INT_MIN; }
    __syncthreads();
    const int y0 = 2 + blockIdx.x * kDnRowsPerBlock;
    for (int y = y0; y < y0 + kDnRowsPerBlock && y < h - 2; ++y) {
        const float* row = mask + (size_t)y * w;
        for (int x = 2 + tid; x < w - 2; x += 256) {                            // x - 1 >= 1 and x + 1 <= w - 2: the neighbours are inside the row
            const float m = row[x], ml = row[x - 1], mr = row[x + 1];
            const bool first = x == 2 || !(ml == m), last = x == w - 3 || !(mr == m);
            if (!first && !last) continue;                                      // the inside of a run: its ends carry the box
            int lo = 0, hi = C;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (sv[mid] < m) lo = mid + 1; else hi = mid; }
            if (lo >= C || !(sv[lo] == m)) continue;                             // a value no point lies under (or NaN)
            const int k = si[lo];
            if (first) { atomicMin(&box[k][0], x); atomicMin(&box[k][2], y); atomicMax(&box[k][3], y); }
            if (last) atomicMax(&box[k][1], x);
        }
    }
    __syncthreads();
    for (int k = tid; k < C; k += 256) {
        if (box[k][0] == INT_MAX) continue;
        atomicMin(&gbox[4 * k], box[k][0]); atomicMax(&gbox[4 * k + 1], box[k][1]); atomicMin(&gbox[4 * k + 2], box[k][2]); atomicMax(&gbox[4 * k + 3], box[k][3]);
    }
}

// the cluster of this workgroup (the largest a with boff <= blockIdx.x; every item has at least one workgroup) and the parameters of its box
__device__ __forceinline__ DnMap dn_batch_setup(const DenseBatch& B, DenseParams& P, int& a, int& b, int& nb) {
    int lo = 0, hi = B.A;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (B.items[mid].boff <= (int)blockIdx.x) lo = mid; else hi = mid; }
    a = lo;
    const DenseBatchItem it = B.items[a];
    P = B.P;
    P.p0 = it.plane[0]; P.p1 = it.plane[1]; P.p2 = it.plane[2]; P.p3 = it.plane[3]; P.pcolor = it.pcolor;
    P.agg = B.aggs + (size_t)it.boff * 8; P.last = B.last + 2 * a; P.out6 = B.ext + 8 * a; P.n_out = reinterpret_cast<int*>(B.ext + 8 * a + 6);
    b = (int)blockIdx.x - it.boff;
    const DnMap M(it.rect[0], it.rect[1], it.rect[2], it.rect[3], true);
    nb = (M.total + kDenseChunk - 1) / kDenseChunk;
    return M;
}
__global__ __launch_bounds__(256) void dense_count_batch_kernel(DenseBatch B) {
    DenseParams P; int a, b, nb;
    const DnMap M = dn_batch_setup(B, P, a, b, nb);
    if (b == 0 && threadIdx.x == 0) { P.last[0] = 0ull; P.last[1] = 0ull; P.n_out[0] = 0; }
    const int n = b < nb ? dn_count_chunk(P, M, b) : 0;
    if (threadIdx.x == 0) B.cnt[blockIdx.x] = n;
}
__global__ __launch_bounds__(256) void dense_write_batch_kernel(DenseBatch B) {
    DenseParams P; int a, b, nb;
    const DnMap M = dn_batch_setup(B, P, a, b, nb);
    if (b < nb) dn_write_chunk(P, M, b, nb, DnEmitRecords{B.pts, (long long)B.cnt[B.items[a].boff], B.pts_cap});
}
__global__ __launch_bounds__(1024) void dense_decide_kernel(DenseBatch B) {
    __shared__ int len[kDenseMaxClusters], part[1024];
    const int t = threadIdx.x;
    for (int a = t; a < kDenseMaxClusters; a += 1024) {
        int n = 0, acc = 0;
        if (a < B.A) {
            const float* e = B.ext + 8 * a;
            n = reinterpret_cast<const int*>(e)[6];
            if (n > 0) {                                                        // :403 on the serial loop's extrema, as nalo_dense_make_map's host side decides it
                float mx[2];
                for (int k = 0; k < 2; ++k) { const unsigned long long q = B.last[2 * a + k]; mx[k] = (q >> 32) ? __uint_as_float((unsigned)q) : FLT_MIN; }
                acc = (e[1] - e[0] < 30 && mx[0] - e[2] < 30 && mx[1] - e[4] < 30) ? 1 : 0;
            }
            B.res[4 * a] = n; B.res[4 * a + 1] = acc; B.res[4 * a + 2] = B.cnt[B.items[a].boff];
        }
        len[a] = acc ? n : 0;
    }
    __syncthreads();
    const int s0 = len[2 * t], s1 = len[2 * t + 1];
    part[t] = s0 + s1;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int x = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    const int ex = part[t] - (s0 + s1);
    if (2 * t < B.A) B.res[4 * (2 * t) + 3] = ex;
    if (2 * t + 1 < B.A) B.res[4 * (2 * t + 1) + 3] = ex + s0;
    if (t == 1023) B.res[4 * B.A] = part[1023];
}
__global__ __launch_bounds__(256) void dense_copy_kernel(DenseBatch B, int NB, nalo_dense_point* const* __restrict__ chunks, long long base, long long cap, int chunk) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= B.cnt[NB] || p >= B.pts_cap) return;
    int lo = 0, hi = B.A;                                                       // the last item that starts at or before p: the one p belongs to (empty items own nothing)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (B.res[4 * mid + 2] <= p) lo = mid; else hi = mid; }
    const int a = lo, t = p - B.res[4 * a + 2];
    if (!B.res[4 * a + 1] || t >= B.res[4 * a]) return;
    const long long q = base + B.res[4 * a + 3] + t;
    if (q >= cap) return;                                                       // (room for every candidate was reserved: never)
    reinterpret_cast<uint4*>(chunks[q / chunk])[q % chunk] = B.pts[p];
}

long long dense_candidates_bound(int w, int h) {
    if (w < 6 || h < 6) return 0;
    return DnMap(2, w - 2, 2, h - 2, true).total;                                // the scanned range as one box: every pixel a cluster can keep
}

// the tables of a call, carved from c->dn_tab in 16-byte words
namespace {
constexpr size_t K_ = kDenseMaxClusters;
constexpr size_t o_svals = 0, o_sidx = o_svals + K_ / 4, o_gbox = o_sidx + K_ / 4, o_items = o_gbox + K_, o_ext = o_items + 3 * K_, o_last = o_ext + 2 * K_,
                 o_res = o_last + K_, o_cdev = o_res + K_ + 1, dn_tab_words = o_cdev + 1;
}

int dense_boxes_enqueue(nalo_ctx* c, const float* mask, const nalo_plane_cluster* rec, const int* n_clusters_dev, int cap_clusters) {
    NALO_HIP(c, c->dn_tab.reserve(dn_tab_words));
    NALO_HIP(c, c->dn_host.reserve(4 * K_ + 12 * K_ + 4 * K_ + 4));
    uint4* T = c->dn_tab.p;
    float* svals = (float*)(T + o_svals); int* sidx = (int*)(T + o_sidx); int* gbox = (int*)(T + o_gbox); int* cdev = (int*)(T + o_cdev);
    ProfScope ps(c, "dense_boxes");
    dense_boxes_prep_kernel<<<1, 1024, 0, c->stream>>>(rec, n_clusters_dev, svals, sidx, gbox, cdev);
    const int rows = std::max(c->h - 4, 0);
    if (rows > 0 && c->w > 4) dense_boxes_kernel<<<(rows + kDnRowsPerBlock - 1) / kDnRowsPerBlock, 256, 0, c->stream>>>(mask, c->w, c->h, cdev, svals, sidx, gbox);
    NALO_HIP(c, hipGetLastError());
    if (cap_clusters > 0) NALO_HIP(c, hipMemcpyAsync(c->dn_host.p, gbox, (size_t)std::min<int>(cap_clusters, (int)K_) * 16, hipMemcpyDeviceToHost, c->stream));
    return NALO_OK;
}

int dense_update_finish(nalo_ctx* c, int slot, const nalo_plane_cluster* clusters, int C, const double camToWorld[12], const DenseArchiveView& V, long long frame_points,
                        nalo_dense_run* runs, int* n_appended, int* n_runs) {
    *n_appended = 0; *n_runs = 0;
    const FrameSlot& s = c->slots[slot];
    const int* boxes = c->dn_host.p;
    DenseBatchItem* items = reinterpret_cast<DenseBatchItem*>(c->dn_host.p + 4 * K_);
    int* resh = c->dn_host.p + 4 * K_ + 12 * K_;
    std::vector<int> owner;                                                     // item -> cluster record
    long long NB = 0, cand = 0;
    for (int k = 0; k < C; ++k) {
        nalo_dense_run& r = runs[k];
        std::memset(&r, 0, sizeof(r)); r.first = -1;
        const nalo_plane_cluster& cl = clusters[k];
        if (!cl.fitted) continue;                                               // `continue` of :280-281: no box is scanned for it
        std::memcpy(r.rect, boxes + 4 * k, 16);
        if (cl.mask_value == 0.f) continue;                                     // `if(pcolor==0) return;` (:355-357)
        const int rx0 = r.rect[0], rx1 = r.rect[1], ry0 = r.rect[2], ry1 = r.rect[3];
        if (!(rx0 != INT_MAX && rx1 > rx0 && ry1 > ry0)) continue;              // the loops' exclusive upper bounds leave nothing
        const DnMap M(rx0, rx1, ry0, ry1, true);
        const int nb = (M.total + kDenseChunk - 1) / kDenseChunk;
        if (nb == 0) continue;
        DenseBatchItem& it = items[owner.size()];
        std::memcpy(it.plane, cl.plane, 16); it.pcolor = cl.mask_value; std::memcpy(it.rect, r.rect, 16); it.boff = (int)NB; it.pad[0] = it.pad[1] = 0;
        owner.push_back(k);
        NB += nb; cand += M.total;
        if (NB > INT_MAX / 16) return fail(c, NALO_ERR_UNSUPPORTED, "nalo_dense_update_map: the clusters' boxes hold more than 2^37 candidates");
    }
    const int A = (int)owner.size();
    if (A == 0) return NALO_OK;
    HostTimer ht(c, "dense_update_map");
    NALO_HIP(c, c->dn_blk.reserve((size_t)NB * 2 + (size_t)(NB + 1 + 3) / 4));  // aggregates (two 16-byte words per chunk) | counts
    const long long bound = dense_candidates_bound(c->w, c->h);
    NALO_HIP(c, c->dn_pts.reserve((size_t)std::max<long long>(bound, 1)));
    uint4* T = c->dn_tab.p;
    DenseBatch B;
    B.P.mask = s.mask.p; B.P.I0 = s.I[0].p; B.P.bgr = s.bgr.p; B.P.w = c->w; B.P.h = c->h; B.P.rows = nullptr; B.P.rect = nullptr;
    B.P.p0 = B.P.p1 = B.P.p2 = B.P.p3 = B.P.pcolor = 0.f;
    B.P.fxi = 1.0f / c->fx[0]; B.P.fyi = 1.0f / c->fy[0]; B.P.cx = c->cx[0]; B.P.cy = c->cy[0];            // DenseMapping::makeK level 0, as nalo_dense_make_map
    std::memcpy(B.P.c2w, camToWorld, sizeof(B.P.c2w));
    B.P.agg = nullptr; B.P.last = nullptr; B.P.out6 = nullptr; B.P.n_out = nullptr;
    B.items = reinterpret_cast<const DenseBatchItem*>(T + o_items); B.A = A;
    B.aggs = reinterpret_cast<float*>(c->dn_blk.p); B.cnt = reinterpret_cast<int*>(c->dn_blk.p + (size_t)NB * 2);
    B.ext = reinterpret_cast<float*>(T + o_ext); B.last = reinterpret_cast<unsigned long long*>(T + o_last);
    B.pts = c->dn_pts.p; B.pts_cap = bound; B.res = reinterpret_cast<int*>(T + o_res);
    NALO_HIP(c, hipMemcpyAsync(T + o_items, items, (size_t)A * sizeof(DenseBatchItem), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "dense_update_map");
        dense_count_batch_kernel<<<(int)NB, 256, 0, c->stream>>>(B);
        { const int rc = scan_ints_launch(c, B.cnt, (int)NB); if (rc) return rc; }
        dense_write_batch_kernel<<<(int)NB, 256, 0, c->stream>>>(B);
        dense_decide_kernel<<<1, 1024, 0, c->stream>>>(B);
        const long long most = std::min(cand, bound);
        dense_copy_kernel<<<(int)std::max<long long>((most + 255) / 256, 1), 256, 0, c->stream>>>(B, (int)NB, V.chunks, V.base, V.cap, V.chunk);
        NALO_HIP(c, hipGetLastError());
    }
    NALO_HIP(c, hipMemcpyAsync(resh, B.res, ((size_t)4 * A + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));                               // the call's second and last wait
    const int total = resh[4 * A];
    if (total < 0 || total > bound) return fail(c, NALO_ERR_HIP, "nalo_dense_update_map: the device appended more points than the image has candidates");
    for (int a = 0; a < A; ++a) {
        nalo_dense_run& r = runs[owner[a]];
        r.n = resh[4 * a]; r.accept = resh[4 * a + 1];
        if (r.accept && r.n > 0) { r.first = frame_points + resh[4 * a + 3]; ++*n_runs; }
    }
    *n_appended = total;
    return NALO_OK;
}

}  // namespace nalo

using namespace nalo;

extern "C" int nalo_dense_make_map(nalo_ctx* c, int slot, const float plane[4], float mask_value, const double camToWorld[12], int cap,
                                   int rect_out[4], int* out_u, int* out_v, float* out_idepth, float* out_color, uint8_t* out_bgr, int* n_out, int* accept) {
    if (!c || !plane || !camToWorld || !n_out || !accept || cap < 0 || slot < 0 || slot >= (int)c->slots.size())
        return fail(c, NALO_ERR_ARG, "nalo_dense_make_map: bad argument");
    FrameSlot& s = c->slots[slot];
    if (!s.valid || !s.mask.p) return fail(c, NALO_ERR_STATE, "nalo_dense_make_map: slot has no pyramid / mask (nalo_frame_upload with mask)");
    NALO_HIP(c, hipSetDevice(c->device));
    *n_out = 0; *accept = 0;
    // ---- bbox scan (MapPoint.cpp:287-310), makeMap and the accept test: three launches back to back, the box never leaves the device in between
    const int nblk = std::max(1, ((c->w - 4) * (c->h - 4) + kDenseChunk - 1) / kDenseChunk);
    const size_t hrows = ((size_t)c->h + 1) & ~(size_t)1;                  // the aggregates behind the row table stay 16-byte aligned
    const size_t lbw = hrows + (size_t)nblk * 4 + 8;                       // int2 rows[h] | float agg[nblk][8] | last[2] | ticket  (in 8-byte words)
    if (c->dense_lb.cap < lbw) {
        NALO_HIP(c, hipStreamSynchronize(c->stream));
        NALO_HIP(c, c->dense_lb.reserve(lbw));
        NALO_HIP(c, hipMemsetAsync(c->dense_lb.p, 0, lbw * 8, c->stream));   // `last` and the ticket start at zero and are re-armed by the kernel
    }
    int2* rows = reinterpret_cast<int2*>(c->dense_lb.p);
    NALO_HIP(c, c->scan_tmp.reserve(8));
    {   // dispatch-attached timestamps (no barrier packets around the launch: an event pair recorded on the stream adds several microseconds to a 5 us kernel)
        ProfScope ps(c, "dense_bbox", true);
        if (ps.a) hipExtLaunchKernelGGL(dense_rows_kernel, dim3(std::max(1, c->h - 4)), dim3(256), 0, c->stream, ps.a, ps.b, 0, s.mask.p, c->w, c->h, mask_value, rows);
        else dense_rows_kernel<<<std::max(1, c->h - 4), 256, 0, c->stream>>>(s.mask.p, c->w, c->h, mask_value, rows);
    }
    int rect[4];
    float ext[6] = {FLT_MAX, FLT_MIN, FLT_MAX, FLT_MIN, FLT_MAX, FLT_MIN};
    int n = 0;
    const size_t capz = (size_t)std::max(cap, 1);
    const size_t words = capz * 5 + 64;                                      // scratch: u, v (int), idepth, colour (float), bgr carved from upload_tmp
    NALO_HIP(c, c->upload_tmp.reserve(words));
    int* du = (int*)c->upload_tmp.p; int* dv = du + capz; float* did = (float*)(dv + capz); float* dcol = did + capz;
    uint8_t* dbgr = (uint8_t*)(dcol + capz);
    NALO_HIP(c, c->trk_partial.reserve(16));
    DenseParams P;
    P.mask = s.mask.p; P.I0 = s.I[0].p; P.bgr = s.bgr.p; P.w = c->w; P.h = c->h; P.rows = rows; P.rect = c->scan_tmp.p;
    P.p0 = plane[0]; P.p1 = plane[1]; P.p2 = plane[2]; P.p3 = plane[3]; P.pcolor = mask_value;
    P.fxi = 1.0f / c->fx[0]; P.fyi = 1.0f / c->fy[0]; P.cx = c->cx[0]; P.cy = c->cy[0];            // DenseMapping::makeK level 0
    std::memcpy(P.c2w, camToWorld, sizeof(P.c2w));
    P.agg = reinterpret_cast<float*>(c->dense_lb.p + hrows);
    P.last = c->dense_lb.p + hrows + (size_t)nblk * 4;
    P.out6 = c->trk_partial.p; P.n_out = reinterpret_cast<int*>(c->trk_partial.p + 8);
    if (mask_value == 0.f) {                                                 // `if(pcolor==0) return;` (:355-357): only the box is wanted
        dense_count_kernel<<<1, 256, 0, c->stream>>>(P);
        NALO_HIP(c, hipMemcpyAsync(rect, c->scan_tmp.p, 16, hipMemcpyDeviceToHost, c->stream));
        NALO_HIP(c, hipStreamSynchronize(c->stream));
        if (rect_out) std::memcpy(rect_out, rect, 16);
        return NALO_OK;
    }
    {
        ProfScope ps(c, "dense_map", true);                    // start of the first dispatch .. end of the second
        if (ps.a) {
            hipExtLaunchKernelGGL(dense_count_kernel, dim3(nblk), dim3(256), 0, c->stream, ps.a, nullptr, 0, P);
            hipExtLaunchKernelGGL(dense_write_kernel, dim3(nblk), dim3(256), 0, c->stream, nullptr, ps.b, 0, P, cap, du, dv, did, dcol, dbgr);
        } else {
            dense_count_kernel<<<nblk, 256, 0, c->stream>>>(P);
            dense_write_kernel<<<nblk, 256, 0, c->stream>>>(P, cap, du, dv, did, dcol, dbgr);
        }
    }
    float res[9];
    unsigned long long lastq[2] = {0, 0};
    NALO_HIP(c, hipMemcpyAsync(rect, c->scan_tmp.p, 16, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(res, c->trk_partial.p, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(lastq, P.last, 16, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 2; ++k) {                                            // maxy / maxz: the coordinate of the last qualifying point, FLT_MIN if none (the reference's seed)
        const unsigned bits = (unsigned)lastq[k]; float v = FLT_MIN;
        if (lastq[k] >> 32) std::memcpy(&v, &bits, 4);
        res[k == 0 ? 3 : 5] = v;
    }
    if (rect_out) std::memcpy(rect_out, rect, 16);
    std::memcpy(&n, &res[8], 4);
    if (n > cap) return fail(c, NALO_ERR_ARG, "nalo_dense_make_map: cap too small");
    if (n > 0) {
        std::memcpy(ext, res, 24);
        if (out_u) NALO_HIP(c, hipMemcpyAsync(out_u, du, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_v) NALO_HIP(c, hipMemcpyAsync(out_v, dv, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_idepth) NALO_HIP(c, hipMemcpyAsync(out_idepth, did, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_color) NALO_HIP(c, hipMemcpyAsync(out_color, dcol, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_bgr && s.bgr.p) NALO_HIP(c, hipMemcpyAsync(out_bgr, dbgr, (size_t)n * 3, hipMemcpyDeviceToHost, c->stream));
        NALO_HIP(c, hipStreamSynchronize(c->stream));
    }
    NALO_HIP(c, hipGetLastError());
    *n_out = n;
    *accept = (ext[1] - ext[0] < 30 && ext[3] - ext[2] < 30 && ext[5] - ext[4] < 30) ? 1 : 0;       // :403
    return NALO_OK;
}
