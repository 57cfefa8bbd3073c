// The map side of the device chain (nalo_map_*; reference paths relative to src/):
//   (A) the push-backs of FullSystem::flagPointsForRemoval                         FullSystem/FullSystem.cpp:968, 996, 1001, 1008
//       with what marginalizePointsF's addPoint rewrites on a marginalised point   OptimizationBackend/AccumulatedSCHessian.cpp:36-50
//   (B) SampleOutputWrapper::publishKeyframes(final = true)                        IOWrapper/OutputWrapper/SampleOutputWrapper.h:110-118 (map_point_math.h)
//   (C) KeyFrameDisplay::setFromKF + refreshPC                                     IOWrapper/Pangolin/KeyFrameDisplay.cpp:92-177, 297-410
//
// All three are ordered compactions in the count / one-workgroup scan / ballot-rank write idiom of kernels_imm_carry.hip:
//   *_count_kernel      survivors per 256-lane workgroup (and the integer statistics: LDS / global integer atomics count, nothing else)
//   scan_ints_launch    one exclusive scan over the workgroups' counts
//   *_write_kernel      the predicate again, rank = scanned offset + the waves before + ballot rank inside the wave; plain vector stores
// Order never comes from an atomic. Built without FMA contraction: the vertex and world-point arithmetic is the reference's, operation by operation.
#include "nalo_internal.h"
#include "ba_device.h"
#include "map_point_math.h"
#include "plot_device.h"
#include "map_cloud_device.h"

namespace nalo {

static_assert(sizeof(nalo_map_record) == 64, "the archive record is four 16-byte quads");

// rank of this lane among the workgroup's lanes with pred, in lane order. Every lane of the workgroup calls it (one barrier).
__device__ __forceinline__ int map_block_rank(bool pred, int* wsum) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(pred);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int r = __popcll(m & ((1ull << lane) - 1));
    for (int k = 0; k < wave; ++k) r += wsum[k];
    return r;
}

// ------------------------------------------------------------------------------------------------ (A) the archive append
// the decision a slot carries (0: it stays), its slot and its host row
__device__ __forceinline__ int map_append_entry(const MapAppendDev& A, int k, int& d, int& h) {
    d = 0; h = 0;
    if (k >= A.P) return 0;
    d = A.kmap[k];
    h = min(max(A.blk_host[d / kBlk], 0), NALO_MAX_WINDOW - 1);
    return A.flags[d] & (PT_MARG | PT_DROP);
}

__global__ __launch_bounds__(256) void map_append_count_kernel(MapAppendDev A) {
    __shared__ int hc[2 * NALO_MAX_WINDOW];
    if (threadIdx.x < 2 * NALO_MAX_WINDOW) hc[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 2 * NALO_MAX_WINDOW) A.hs_next[threadIdx.x] = 0;      // the NEXT call's counters (two buffers): no fill on the path
    __syncthreads();
    int d, h;
    const int f = map_append_entry(A, blockIdx.x * 256 + threadIdx.x, d, h);
    if (f) atomicAdd(&hc[2 * h + ((f & PT_MARG) ? 0 : 1)], 1);
    __syncthreads();
    if (threadIdx.x < 2 * NALO_MAX_WINDOW && hc[threadIdx.x]) atomicAdd(&A.hs[threadIdx.x], hc[threadIdx.x]);
    if (threadIdx.x == 0) { int s = 0; for (int i = 0; i < 2 * NALO_MAX_WINDOW; ++i) s += hc[i]; A.cnt[blockIdx.x] = s; }
}

// PATCH = false, before the marginalisation pass: the whole record. PATCH = true, behind its accumulation: idepth_hessian of a marginalised point is H of the
// re-accumulated Hdd and the scaled prior (sc_point_finish left both), and a point without an active residual gets idepth_hessian = maxRelBaseline = 0.
template <bool PATCH>
__global__ __launch_bounds__(256) void map_append_write_kernel(MapAppendDev A) {
    __shared__ int wsum[4];
    int d, h;
    const int f = map_append_entry(A, blockIdx.x * 256 + threadIdx.x, d, h);
    const int r = A.cnt[blockIdx.x] + map_block_rank(f != 0, wsum);
    if (!f) return;
    const long long q = A.base + r;
    if (q >= A.cap) return;                                                     // (the host reserved a record for every valid point: never)
    nalo_map_record* rec = A.chunks[q / A.chunk] + (q % A.chunk);
    if (PATCH) {
        if (!(f & PT_MARG)) return;
        if (A.ngood[d] == 0) { rec->idepth_hessian = 0.f; rec->maxRelBaseline = 0.f; return; }
        float H = A.acc[d].x + A.prior[d];
        if (H < 1e-10f) H = 1e-10f;
        rec->idepth_hessian = H;
        return;
    }
    const float4 g = A.geo[d];
    float4* o = reinterpret_cast<float4*>(rec);
    o[0] = make_float4(g.x, g.y, kScaleIdepth * g.z, A.H[d]);
    o[1] = make_float4(A.relbs[d], __int_as_float((f & PT_MARG) ? 2 : 3), __int_as_float((int)A.dec[d]), __int_as_float(A.frame_id[h]));
    o[2] = A.col0[d];
    o[3] = A.col1[d];
}

int map_append_rank_launch(nalo_ctx* c, const MapAppendDev& A) {
    if (A.nb <= 0) return NALO_OK;
    ProfScope ps(c, "map_append");
    map_append_count_kernel<<<A.nb, 256, 0, c->stream>>>(A);
    return scan_ints_launch(c, A.cnt, A.nb);
}
int map_append_write_launch(nalo_ctx* c, const MapAppendDev& A, bool patch) {
    if (A.nb <= 0) return NALO_OK;
    ProfScope ps(c, patch ? "map_append_patch" : "map_append");
    if (patch) map_append_write_kernel<true><<<A.nb, 256, 0, c->stream>>>(A);
    else map_append_write_kernel<false><<<A.nb, 256, 0, c->stream>>>(A);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ (B) the final cloud of a frame that leaves
__global__ __launch_bounds__(256) void map_world_count_kernel(MapWorldDev D) {
    __shared__ int wsum[4];
    MapRec R;
    const bool in = map_fetch<false>(D.S, blockIdx.x * 256 + threadIdx.x, R);
    const int r = map_block_rank(in, wsum);
    if (threadIdx.x == 255) D.S.cnt[blockIdx.x] = r + (in ? 1 : 0);
}
__global__ __launch_bounds__(256) void map_world_write_kernel(MapWorldDev D) {
    __shared__ int wsum[4];
    MapRec R;
    const bool in = map_fetch<false>(D.S, blockIdx.x * 256 + threadIdx.x, R);
    const int r = D.S.cnt[blockIdx.x] + map_block_rank(in, wsum);
    if (!in || r >= D.cap) return;                                              // (the host sized xyz by its own count of the frame's marginalised points: never)
    double wp[3];
    map_world_point(R.u, R.v, R.idepth, D.ci, D.m, wp);
    double* o = D.xyz + 3 * (size_t)r;
    o[0] = wp[0]; o[1] = wp[1]; o[2] = wp[2];
}
int map_world_launch(nalo_ctx* c, const MapWorldDev& D) {
    if (D.S.nb <= 0) return NALO_OK;
    ProfScope ps(c, "map_world_points");
    map_world_count_kernel<<<D.S.nb, 256, 0, c->stream>>>(D);
    int rc = scan_ints_launch(c, D.S.cnt, D.S.nb); if (rc) return rc;
    map_world_write_kernel<<<D.S.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ (C) what the viewer gets per keyframe
// refreshPC's filter, the vertices and the colours: map_cloud_device.h (the 3-D panel shares them)
__global__ __launch_bounds__(256) void map_cloud_count_kernel(MapCloudDev C) {
    __shared__ int wsum[4];
    MapRec R;
    R.status = -1;
    const bool in = map_fetch<false>(C.S, blockIdx.x * 256 + threadIdx.x, R);
    float depth;
    const bool keep = in && map_cloud_keep(C.mode, C.scaledTH, C.absTH, C.minRelBS, R, depth);
    const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const int nr = __popcll(__ballot(in && R.status == st)), ns = __popcll(__ballot(keep && R.status == st));
        if (lead && nr) atomicAdd(&C.stats[st], nr);
        if (lead && ns) atomicAdd(&C.stats[4 + st], ns);
    }
    const int r = map_block_rank(keep, wsum);
    if (threadIdx.x == 255) C.S.cnt[blockIdx.x] = r + (keep ? 1 : 0);
}
__global__ __launch_bounds__(256) void map_cloud_write_kernel(MapCloudDev C) {
    __shared__ int wsum[4];
    MapRec R;
    const bool in = map_fetch<true>(C.S, blockIdx.x * 256 + threadIdx.x, R);
    float depth;
    const bool keep = in && map_cloud_keep(C.mode, C.scaledTH, C.absTH, C.minRelBS, R, depth);
    const int r = C.S.cnt[blockIdx.x] + map_block_rank(keep, wsum);
    if (!keep || r >= C.cap) return;                                            // (survivors <= the frame's records, which the host sized the outputs by)
    const float fxi = C.ci[0];
    constexpr int dx[8] = NALO_PATTERN_DX, dy[8] = NALO_PATTERN_DY;
    const size_t j0 = 8 * (size_t)r;                                            // the first of the record's eight output vertices = its first draw
    float vtx[24];
    unsigned cb[8];
#pragma unroll
    for (int pnt = 0; pnt < 8; ++pnt) {                                         // :334-387
        map_cloud_vertex_xy(C.ci, R, depth, dx[pnt], dy[pnt], vtx[3 * pnt], vtx[3 * pnt + 1]);
        // rand() / (float)RAND_MAX - 0.5f; without draws the library's no-jitter form: the bracket below is exactly 1
        const float jit = C.draws ? ((float)C.draws[j0 + pnt] / (float)2147483647 - 0.5f) : 0.f;
        vtx[3 * pnt + 2] = depth * (1 + 2 * fxi * jit);
        cb[pnt] = plot_byte(R.col[pnt]);
    }
    float4* ov = reinterpret_cast<float4*>(C.xyz + 3 * j0);                      // 96 bytes per record: 16-byte aligned
#pragma unroll
    for (int k = 0; k < 6; ++k) ov[k] = make_float4(vtx[4 * k], vtx[4 * k + 1], vtx[4 * k + 2], vtx[4 * k + 3]);
    unsigned wd[6];
    if (C.mode == 0) {                                                          // :349-372, little-endian bytes {c0 c1 c2} x 8
        unsigned t[3];
        map_cloud_mode0(R.status, t);
#pragma unroll
        for (int k = 0; k < 6; ++k) wd[k] = t[(4 * k) % 3] | (t[(4 * k + 1) % 3] << 8) | (t[(4 * k + 2) % 3] << 16) | (t[(4 * k + 3) % 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) wd[k] = cb[(4 * k) / 3] | (cb[(4 * k + 1) / 3] << 8) | (cb[(4 * k + 2) / 3] << 16) | (cb[(4 * k + 3) / 3] << 24);
    }
    uint2* oc = reinterpret_cast<uint2*>(C.rgb + 3 * j0);                        // 24 bytes per record: 8-byte aligned
    oc[0] = make_uint2(wd[0], wd[1]); oc[1] = make_uint2(wd[2], wd[3]); oc[2] = make_uint2(wd[4], wd[5]);
}
int map_cloud_launch(nalo_ctx* c, const MapCloudDev& C) {
    if (C.S.nb <= 0) return NALO_OK;
    ProfScope ps(c, "map_frame_cloud");
    map_cloud_count_kernel<<<C.S.nb, 256, 0, c->stream>>>(C);
    int rc = scan_ints_launch(c, C.S.cnt, C.S.nb); if (rc) return rc;
    map_cloud_write_kernel<<<C.S.nb, 256, 0, c->stream>>>(C);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ (D) the dense map's two consumers (nalo_map_dense_*)
// point i of the frame's dense list: its archive pieces in append order
__device__ __forceinline__ bool map_dense_fetch(const MapDenseDev& D, int i, uint4& r) {
    MapSeg sg; int t;
    if (!map_find_seg(D.segs, D.nseg, D.total, i, sg, t)) return false;
    r = reinterpret_cast<const uint4*>(sg.p)[t];                                 // {u | v << 16, idepth, colour, b | g << 8 | r << 16}
    return true;
}
// SampleOutputWrapper.h:152-176: one lane per point, no compaction (every point is written)
__global__ __launch_bounds__(256) void map_dense_world_kernel(MapDenseDev D) {
    uint4 r;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (!map_dense_fetch(D, i, r)) return;
    double wp[3];
    map_world_point((float)(r.x & 0xFFFFu), (float)(r.x >> 16), __uint_as_float(r.y), D.ci, D.m, wp);
    double* o = D.wxyz + 3 * (size_t)i;
    o[0] = wp[0]; o[1] = wp[1]; o[2] = wp[2];
}
int map_dense_world_launch(nalo_ctx* c, const MapDenseDev& D) {
    if (D.nb <= 0) return NALO_OK;
    ProfScope ps(c, "map_dense_world_points");
    map_dense_world_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}
// KeyFrameDisplay::refreshPC() :225-248: `if(idpeth < 0) continue;` - a NaN stays
__global__ __launch_bounds__(256) void map_dense_cloud_count_kernel(MapDenseDev D) {
    __shared__ int wsum[4];
    uint4 r = make_uint4(0, 0, 0, 0);
    const bool in = map_dense_fetch(D, blockIdx.x * 256 + threadIdx.x, r);
    const bool keep = in && map_dense_keep(r);
    const int k = map_block_rank(keep, wsum);
    if (threadIdx.x == 255) D.cnt[blockIdx.x] = k + (keep ? 1 : 0);
}
__global__ __launch_bounds__(256) void map_dense_cloud_write_kernel(MapDenseDev D) {
    __shared__ int wsum[4];
    uint4 r = make_uint4(0, 0, 0, 0);
    const bool in = map_dense_fetch(D, blockIdx.x * 256 + threadIdx.x, r);
    const bool keep = in && map_dense_keep(r);
    const int j = D.cnt[blockIdx.x] + map_block_rank(keep, wsum);                // the output vertex = the draw index
    if (!keep || j >= D.total) return;
    const float fxi = D.ci[0];
    float x, y, depth;
    map_dense_vertex(r, D.ci, x, y, depth);
    const float jit = D.draws ? ((float)D.draws[j] / (float)2147483647 - 0.5f) : 0.f;   // as map_cloud_write_kernel: without draws the bracket is exactly 1
    float* o = D.xyz + 3 * (size_t)j;
    o[0] = x; o[1] = y; o[2] = depth * (1 + 2 * fxi * jit);
    uint8_t* q = D.rgb + 3 * (size_t)j;
    q[0] = (uint8_t)(r.w >> 16); q[1] = (uint8_t)(r.w >> 8); q[2] = (uint8_t)r.w;  // {bgr[2], bgr[1], bgr[0]}
}
int map_dense_cloud_launch(nalo_ctx* c, const MapDenseDev& D) {
    if (D.nb <= 0) return NALO_OK;
    ProfScope ps(c, "map_dense_cloud");
    map_dense_cloud_count_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    int rc = scan_ints_launch(c, D.cnt, D.nb); if (rc) return rc;
    map_dense_cloud_write_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
