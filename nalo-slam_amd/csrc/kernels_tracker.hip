// Front-end tracker kernels for gfx950.
//   a2  makeCoarseDepthL0 steps 1-5   (reference src/FullSystem/CoarseTracker.cpp:382-538)
//   a3  calcRes                        (CoarseTracker.cpp:891-1049)      } fused into ONE pass: no buf_warped_*
//   a4  calcGSSSE + Accumulator9       (CoarseTracker.cpp:828-885,       } round trip through memory
//                                       OptimizationBackend/MatrixAccumulators.h:1091-1166)
// Reduction: per-lane fp32 accumulators over a grid-stride loop -> quad DPP adds -> 64 LDS rows per block ->
// column sums -> one fp32 partial per block -> fp64 finish kernel (deterministic: no float atomics on sums).
#include "nalo_internal.h"
#include "reduce.h"
#include "trk_device.h"

namespace nalo {

// ------------------------------------------------------------------------------------------------ a3 + a4
struct TrkEvalParams {
    TrkLevel L;
    int lvl;
    int i0, i1;                     // this rank's share [i0, i1) of the level's points (all of them unless the tracker is sharded, nalo_trk_set_shard)
    float RKi[9], t[3], Ki[9];
    float affa, affb, b0, cutoff, maxEnergy;
};
typedef float trk_f4 __attribute__((ext_vector_type(4)));

constexpr int kTrkEvalNT = 512;                   // lanes per workgroup of the evaluation. 256 -> 512 (round 4, same box): half as many grid-stride rounds at 250 k points and half as many
                                                  // partial rows for the last workgroup: 21.0 -> 19.0 us at 250 k points, 40.0 -> 35.7 us at full density (1920x1072)
constexpr int kTrkEvalNG = kTrkEvalNT / 13;        // lane groups of the last workgroup's sum: 13 lanes x 16 bytes = one block's 52 partials
__global__ __launch_bounds__(kTrkEvalNT) void trk_eval_kernel(TrkEvalParams P, float* __restrict__ partial, unsigned* __restrict__ ticket, double* __restrict__ out, double seq) {
    __shared__ __attribute__((aligned(16))) float smem[(kTrkEvalNT / 4) * (kTrkVals + 1)];
    float acc[kTrkVals];
#pragma unroll
    for (int k = 0; k < kTrkVals; ++k) acc[k] = 0.f;
    const TrkLevel& L = P.L;
    const float wlm3 = (float)(L.wl - 3), hlm3 = (float)(L.hl - 3);
    for (int i = P.i0 + blockIdx.x * blockDim.x + threadIdx.x; i < P.i1; i += gridDim.x * blockDim.x) {
        const float id = L.id[i], x = L.u[i], y = L.v[i];
        float u, v, Ku, Kv, new_idepth;
        trk_project(P.RKi, P.t, L, x, y, id, u, v, Ku, Kv, new_idepth);
        if (P.lvl == 0 && (i & 31) == 0) trk_flow(acc, P.RKi, P.Ki, P.t, L, x, y, id, Ku, Kv);
        if (!(Ku > 2.f && Kv > 2.f && Ku < wlm3 && Kv < hlm3 && new_idepth > 0.f)) continue;      // :981
        const float refColor = L.col[i];
        const float4* bp = L.dI + (int)Ku + (int)Kv * L.wl;                      // the taps are loaded only for points inside the level
        const float3 hit = trk_interp(Ku, Kv, bp[0], bp[1], bp[L.wl], bp[1 + L.wl]);
        if (!isfinite(hit.x)) continue;
        float hw; const float residual = trk_residual(hit.x, refColor, P.affa, P.affb, hw);
        acc[kTrkNE] += 1.f;
        if (fabsf(residual) > P.cutoff) { acc[kTrkE] += P.maxEnergy; acc[kTrkNSat] += 1.f; }
        else {
            acc[kTrkE] += hw * residual * residual * (2.f - hw);
            acc[kTrkNWarped] += 1.f;
            float J[9];
            trk_jacobian(J, hit, refColor, u, v, new_idepth, L.fx, L.fy, P.affa, P.b0, residual);
#pragma unroll
            for (int r = 0; r < 9; ++r) {                    // constant indices after unrolling: acc[] stays in VGPRs (a running `k++` index sent it to scratch)
                const float Jw = J[r] * hw;
#pragma unroll
                for (int c2 = r; c2 < 9; ++c2) acc[trk_ut(r, c2)] += Jw * J[c2];
            }
        }
    }
    // Round 4: the fp64 finish rides in this launch (it was a second, 10 us launch behind a 14 us one). A workgroup's 52 partials leave as
    // agent-scope words, acknowledged before its ticket (the idiom of ba_reduce_kernel's tail); the workgroup that draws the last ticket sums the partials in a fixed order (fp64) and
    // publishes them behind the sequence number the host polls.
    __shared__ float blk[64];
    block_reduce_cols<kTrkVals, kTrkEvalNT>(acc, smem, blk);
    if (threadIdx.x < kTrkVals) __hip_atomic_store(&partial[(size_t)blockIdx.x * 64 + threadIdx.x], blk[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __shared__ bool is_last;
    __syncthreads();
    if (threadIdx.x == 0) is_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
    __syncthreads();
    if (!is_last) return;
    // 13 lanes x 16 bytes cover a block's 52 partials; kTrkEvalNG (19 of a 256-lane workgroup) such lane groups stride over the blocks with fourteen coherent (sc0 sc1: past this XCD's L2, where the
    // other XCDs' write-through stores are not seen) 16-byte loads in flight each - one relaxed atomic word per lane and trip was a chain of ~130 dependent
    // round trips (50 us). Fixed order: rows b = rg, rg + NG, ... in fp64 per group, then the groups in ascending order.
    double (*part)[kTrkVals] = reinterpret_cast<double (*)[kTrkVals]>(smem);       // NG x 52 doubles (7.9 KB of the 13.6 KB reduction buffer at 256 lanes)
    const int cq = threadIdx.x % 13, rg = threadIdx.x / 13, nblocks = (int)gridDim.x;
    static_assert(kTrkEvalNG * kTrkVals * 2 <= (kTrkEvalNT / 4) * (kTrkVals + 1), "the groups' fp64 sums fit the reduction buffer");
    if (rg < kTrkEvalNG) {
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int b0 = rg; b0 < nblocks; b0 += kTrkEvalNG * 14) {
            trk_f4 v[14];
#pragma unroll
            for (int k = 0; k < 14; ++k) {
                const int b2 = b0 + kTrkEvalNG * k;
                const float* q = partial + (size_t)(b2 < nblocks ? b2 : b0) * 64 + cq * 4;
                asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v[k]) : "v"(q) : "memory");
            }
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]) : : "memory");
#pragma unroll
            for (int k = 0; k < 14; ++k) if (b0 + kTrkEvalNG * k < nblocks) { a0 += (double)v[k].x; a1 += (double)v[k].y; a2 += (double)v[k].z; a3 += (double)v[k].w; }
        }
        part[rg][cq * 4] = a0; part[rg][cq * 4 + 1] = a1; part[rg][cq * 4 + 2] = a2; part[rg][cq * 4 + 3] = a3;
    }
    __syncthreads();
    if (threadIdx.x < kTrkVals) { double t = 0; for (int k = 0; k < kTrkEvalNG; ++k) t += part[k][threadIdx.x]; __hip_atomic_store(&out[threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                // re-armed for the next (stream-ordered) launch
        __hip_atomic_store(&out[63], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// out = host-mapped pinned memory; out[63] carries the sequence number of this evaluation, published after the data so the host can poll it instead of paying a
// stream synchronisation per LM iteration
// sharded tracker ("all-reduce of 45 + 6 floats per evaluation"): the evaluation's last workgroup leaves this rank's 52 fp64 sums in DEVICE memory (out = device buffer,
// seq unused), the caller's hook sums them over the ranks in place, and this kernel publishes the result the way the evaluation's tail does
__global__ __launch_bounds__(64) void trk_publish_kernel(const double* __restrict__ src, double* __restrict__ out, double seq) {
    if (threadIdx.x < kTrkVals) __hip_atomic_store(&out[threadIdx.x], src[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    if (threadIdx.x == 0) { __threadfence_system(); __hip_atomic_store(&out[63], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
}

int trk_eval_launch(nalo_ctx* c, int slot_new, int lvl, const float RKi[9], const float t[3], const float Ki[9],
                    float affa, float affb, float b0, float cutoff, float maxEnergy, double out64[64]) {
    TrkEvalParams P;
    P.L = trk_level(c, slot_new, lvl); P.lvl = lvl;
    const bool sharded = c->trk_world > 1 && c->trk_hook;
    P.i0 = sharded ? (int)((long long)P.L.n * c->trk_rank / c->trk_world) : 0;
    P.i1 = sharded ? (int)((long long)P.L.n * (c->trk_rank + 1) / c->trk_world) : P.L.n;
    for (int i = 0; i < 9; ++i) { P.RKi[i] = RKi[i]; P.Ki[i] = Ki[i]; }
    for (int i = 0; i < 3; ++i) P.t[i] = t[i];
    P.affa = affa; P.affb = affb; P.b0 = b0; P.cutoff = cutoff; P.maxEnergy = maxEnergy;
    int nblocks = (P.i1 - P.i0 + kTrkEvalNT - 1) / kTrkEvalNT;
    nblocks = nblocks < 1 ? 1 : (nblocks > 512 ? 512 : nblocks);
    NALO_HIP(c, c->trk_partial.reserve((size_t)2048 * 64));
    if (!c->trk_ticket.p) { NALO_HIP(c, c->trk_ticket.reserve(4)); NALO_HIP(c, hipMemsetAsync(c->trk_ticket.p, 0, 16, c->stream)); }
    double* const dout = c->trk_out_host.dev;
    const double seq = (double)(++c->trk_seq);
    if (sharded) NALO_HIP(c, c->trk_shard_sums.reserve(64));
    {
        ProfScope ps(c, "trk_eval");
        trk_eval_kernel<<<nblocks, kTrkEvalNT, 0, c->stream>>>(P, c->trk_partial.p, c->trk_ticket.p, sharded ? c->trk_shard_sums.p : dout, sharded ? 0.0 : seq);
    }
    if (sharded) {
        // every rank evaluated its share: the 52 sums meet in the hook (in place, device memory), every rank then reads the same totals and runs the same LM step
        if (!c->trk_hook_stream_ordered) NALO_HIP(c, hipStreamSynchronize(c->stream));
        c->trk_hook(c->trk_hook_user, c->trk_shard_sums.p, kTrkVals);
        // the same latch as the BA's call_hook (host_ba.hip): a rank whose collective failed must not take an LM step on rank-local sums - the ranks would take
        // different steps and evaluation counts, and the next collectives would mismatch or hang
        if (c->xchg_failed) return NALO_ERR_HIP;                        // message already in c->err (nalo_ba_exchange_failed / the RCCL hooks)
        trk_publish_kernel<<<1, 64, 0, c->stream>>>(c->trk_shard_sums.p, dout, seq);
    }
    NALO_HIP(c, hipGetLastError());
    if (!poll_flag(c, &c->trk_out_host.p[63], seq)) return NALO_ERR_HIP;
    std::memcpy(out64, c->trk_out_host.p, sizeof(double) * kTrkVals);
    return NALO_OK;
}

// ------------------------------------------------------------------------------------------------ a2
// step 1 (CoarseTracker.cpp:388-405): weighted scatter. Two points on one pixel commute exactly in fp32; three or more (rare) would make the sum depend on
// the arrival order of the atomics while the reference adds them serially, in residual order. The scatter therefore also counts the hits per pixel, and
// the fix pass (trk_scatter_hot_kernel) redoes the pixels with >= 3 hits in ascending residual index: the result is the serial loop's, bit for bit, run to run.
__global__ __launch_bounds__(256) void trk_scatter_kernel(const float* __restrict__ Ku, const float* __restrict__ Kv, const float* __restrict__ nid,
                                                          const float* __restrict__ HdiF, int n, int w0, int h0, float* __restrict__ idepth, float* __restrict__ wsum, int* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int u = (int)(Ku[i] + 0.5f), v = (int)(Kv[i] + 0.5f);
    if (u < 0 || v < 0 || u >= w0 || v >= h0) return;
    const float weight = sqrtf((float)(1e-3 / ((double)HdiF[i] + 1e-12)));
    atomicAdd(idepth + u + w0 * v, nid[i] * weight);
    atomicAdd(wsum + u + w0 * v, weight);
    atomicAdd(cnt + u + w0 * v, 1);
}
// Pass 1 (trk_scatter_hot_kernel, the whole grid) lists the residuals whose pixel took three or more hits - in any order: the rounds below order by INDEX,
// not by list position; pass 2 (trk_scatter_fix_body, ONE workgroup) zeroes those pixels and adds the listed residuals back one per pixel and round, always
// the lowest remaining index first (the pixel's count word is reused as the "next index allowed" gate). Usually the list is empty and pass 2 is one read.
// (The list used to be built by the single workgroup itself, striding all n residuals: 530 us at n = 250 000.)
// The global list has room for all n residuals (a residual is listed at most once), so no count is ever dropped. Up to kScatterFixLds entries the rounds
// run on an LDS copy; a longer list (a full-size window's residuals on the newest frame: tens of thousands) runs them on the global list itself.
constexpr int kScatterFixLds = 4096;
struct ScatterListLds {                              // the LDS copy: written and read by the fixing workgroup only
    int* p;
    __device__ int ld(int k) const { return p[k]; }
    __device__ void st(int k, int v) const { p[k] = v; }
};
struct ScatterListGlobal {                           // the global list: every access at L2 (its entries were stored by other workgroups)
    int* p;
    __device__ int ld(int k) const { return __hip_atomic_load(p + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void st(int k, int v) const { __hip_atomic_store(p + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
template <int NT, class List>
__device__ __forceinline__ void trk_scatter_fix_rounds(List list, int m, const float* __restrict__ Ku, const float* __restrict__ Kv, const float* __restrict__ nid,
                                                       const float* __restrict__ HdiF, int w0, float* __restrict__ idepth, float* __restrict__ wsum, int* __restrict__ cnt) {
    const int tid = threadIdx.x;
    for (int k = tid; k < m; k += NT) {
        const int i = list.ld(k), p = (int)(Ku[i] + 0.5f) + w0 * (int)(Kv[i] + 0.5f);
        // every access to the pixel's words below goes to L2 (atomics / agent-scope loads): the atomics of the scatter and of the gate bypass this CU's L1,
        // a plain load could return a stale line
        atomicExch(idepth + p, 0.f); atomicExch(wsum + p, 0.f); atomicExch(cnt + p, 0x7fffffff);       // gate = lowest listed index of the pixel, found next
    }
    __syncthreads();
    for (int k = tid; k < m; k += NT) { const int i = list.ld(k); atomicMin(cnt + (int)(Ku[i] + 0.5f) + w0 * (int)(Kv[i] + 0.5f), i); }
    __syncthreads();
    // rounds: a listed residual adds itself when the gate of its pixel shows its index, then passes the gate to the next listed index of that pixel
    for (int round = 0; round < m; ++round) {
        bool any = false;
        for (int k = tid; k < m; k += NT) {
            const int i = list.ld(k);
            if (i < 0) continue;
            const int p = (int)(Ku[i] + 0.5f) + w0 * (int)(Kv[i] + 0.5f);
            if (__hip_atomic_load(cnt + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i) {
                const float weight = sqrtf((float)(1e-3 / ((double)HdiF[i] + 1e-12)));
                atomicAdd(idepth + p, __fmul_rn(nid[i], weight)); atomicAdd(wsum + p, weight);         // one adder per pixel and round: the order is the index order
                list.st(k, -1 - i);                                                                 // done (kept negative so that the gate search can skip it)
            } else any = true;
        }
        __syncthreads();
        if (!__syncthreads_or(any)) break;
        // next gate per pixel: the lowest not-yet-added listed index
        for (int k = tid; k < m; k += NT) { const int i = list.ld(k); if (i < 0) { const int j = -1 - i, p = (int)(Ku[j] + 0.5f) + w0 * (int)(Kv[j] + 0.5f); atomicCAS(cnt + p, j, 0x7fffffff); } }
        __syncthreads();
        for (int k = tid; k < m; k += NT) { const int i = list.ld(k); if (i >= 0) atomicMin(cnt + (int)(Ku[i] + 0.5f) + w0 * (int)(Kv[i] + 0.5f), i); }
        __syncthreads();
    }
}
// hot = {counter, ticket, list[n]}
template <int NT>
__device__ __forceinline__ void trk_scatter_fix_body(const float* __restrict__ Ku, const float* __restrict__ Kv, const float* __restrict__ nid, const float* __restrict__ HdiF,
                                                     int w0, float* __restrict__ idepth, float* __restrict__ wsum, int* __restrict__ cnt, int* __restrict__ hot, int* slist) {
    const int tid = threadIdx.x;
    const int m = __hip_atomic_load(hot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (m == 0) return;
    __syncthreads();
    if (tid == 0) __hip_atomic_store(hot, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // re-armed for the next (stream-ordered) call
    if (m > kScatterFixLds) { trk_scatter_fix_rounds<NT>(ScatterListGlobal{hot + 2}, m, Ku, Kv, nid, HdiF, w0, idepth, wsum, cnt); return; }
    for (int k = tid; k < m; k += NT) slist[k] = __hip_atomic_load(hot + 2 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    trk_scatter_fix_rounds<NT>(ScatterListLds{slist}, m, Ku, Kv, nid, HdiF, w0, idepth, wsum, cnt);
}
// Round 4: ONE launch for both passes (the fix pass was a launch of its own, 4.6 us for what is almost always one read): every workgroup lists its residuals on hot pixels
// (agent-scope stores, acknowledged before its ticket), the workgroup that draws the last ticket runs the fix.
__global__ __launch_bounds__(256) void trk_scatter_hot_kernel(const float* __restrict__ Ku, const float* __restrict__ Kv, const float* __restrict__ nid, const float* __restrict__ HdiF,
                                                              int n, int w0, int h0, float* __restrict__ idepth, float* __restrict__ wsum, int* __restrict__ cnt,
                                                              int* __restrict__ hot /* counter, ticket, list[n] */) {
    __shared__ int slist[kScatterFixLds];
    __shared__ int is_last;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int u = (int)(Ku[i] + 0.5f), v = (int)(Kv[i] + 0.5f);
        if (!(u < 0 || v < 0 || u >= w0 || v >= h0) && __hip_atomic_load(cnt + u + w0 * v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 3) {       // written by the scatter's atomics: read at L2
            const int at = atomicAdd(hot, 1);                                                    // < n: every residual is listed at most once
            __hip_atomic_store(hot + 2 + at, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) is_last = __hip_atomic_fetch_add((unsigned*)(hot + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
    __syncthreads();
    if (!is_last) return;
    if (threadIdx.x == 0) __hip_atomic_store(hot + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ticket re-armed for the next (stream-ordered) call
    trk_scatter_fix_body<256>(Ku, Kv, nid, HdiF, w0, idepth, wsum, cnt, hot, slist);
}
// All levels of steps 2-5 go through ONE launch per step (the per-level launches were ~30 dependent kernels of a few microseconds each).
struct TrkLevels {
    float *id[NALO_MAX_LEVELS], *ws[NALO_MAX_LEVELS], *wb[NALO_MAX_LEVELS];      // idepth, weight sums, dilated weight sums (output of step 3/4)
    const float4* dI[NALO_MAX_LEVELS];                                            // reference frame texels
    float *pu[NALO_MAX_LEVELS], *pv[NALO_MAX_LEVELS], *pid[NALO_MAX_LEVELS], *pcol[NALO_MAX_LEVELS];
    int wl[NALO_MAX_LEVELS], hl[NALO_MAX_LEVELS];
    int blk0[NALO_MAX_LEVELS + 1];                                                // first block of each level in a level-partitioned grid
    int scan0[NALO_MAX_LEVELS + 1];                                               // counts/offsets base per level inside scan_tmp ([nb counts | nb+1 offsets])
    int L;
};
__global__ __launch_bounds__(256) void trk_zero2_kernel(float* __restrict__ a, float* __restrict__ b, int* __restrict__ cnt, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a[i] = 0.f; b[i] = 0.f; cnt[i] = 0; }
    if (i == 0) { cnt[n] = 0; cnt[n + 1] = 0; }              // the hot list's counter and the ticket of trk_scatter_hot_kernel
}
// step 2 (:408-433): 2x2 SUM pyramid, every level from one pass over level 0. A block owns a 32x32 level-0 tile = 16x16 level-1 pixels, and
// walks up through LDS (8x8, 4x4, 2x2, 1); each parent is a + b + c + d of its four children in the reference's order, so the values
// are those of the level-by-level loop bit for bit.
// The walk above level 1, shared by trk_sum_down_all_kernel and trk_seed_depth_kernel: lane (tx, ty) of tile (bx, by) hands in its level-1 pair (a, b), zeros where
// the tile leaves the level.
__device__ __forceinline__ void trk_sum_walk_up(const TrkLevels& P, int bx, int by, int tx, int ty, float a, float b, float (*sid)[16 * 16], float (*sws)[16 * 16]) {
    sid[0][ty * 16 + tx] = a; sws[0][ty * 16 + tx] = b;
    int side = 16, cur = 0;
    for (int l = 2; l < P.L; ++l) {
        __syncthreads();
        const int ps = side; side >>= 1;
        if (side == 0) break;                                  // more than 6 levels would need a larger tile (NALO_MAX_LEVELS = 6)
        if (tx < side && ty < side) {
            const int x = bx * side + tx, y = by * side + ty, o = 2 * tx + 2 * ty * ps;
            const float a = sid[cur][o] + sid[cur][o + 1] + sid[cur][o + ps] + sid[cur][o + ps + 1];
            const float b = sws[cur][o] + sws[cur][o + 1] + sws[cur][o + ps] + sws[cur][o + ps + 1];
            if (x < P.wl[l] && y < P.hl[l]) { P.id[l][x + y * P.wl[l]] = a; P.ws[l][x + y * P.wl[l]] = b; }
            sid[cur ^ 1][ty * side + tx] = a; sws[cur ^ 1][ty * side + tx] = b;
        }
        cur ^= 1;
    }
}
__global__ __launch_bounds__(256) void trk_sum_down_all_kernel(TrkLevels P) {
    __shared__ float sid[2][16 * 16], sws[2][16 * 16];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int tiles_x = (P.wl[1] + 15) / 16;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const int x = bx * 16 + tx, y = by * 16 + ty, w0 = P.wl[0];
    float a = 0.f, b = 0.f;
    if (x < P.wl[1] && y < P.hl[1]) {
        const int o = 2 * x + 2 * y * w0;
        a = P.id[0][o] + P.id[0][o + 1] + P.id[0][o + w0] + P.id[0][o + w0 + 1];
        b = P.ws[0][o] + P.ws[0][o + 1] + P.ws[0][o + w0] + P.ws[0][o + w0 + 1];
        P.id[1][x + y * P.wl[1]] = a; P.ws[1][x + y * P.wl[1]] = b;
    }
    trk_sum_walk_up(P, bx, by, tx, ty, a, b, sid, sws);
}
// nalo_trk_set_ref_from_depth: steps 1 and 2 in ONE launch, for a seed in which every level-0 pixel takes at most one hit (no atomics, no hit counts, no hot list).
// A workgroup owns a 32x32 level-0 tile as above, a lane its 2x2 quad: the four depths come through the plane's byte strides (and, with the gradient test on, the
// four absSquaredGrad values of the slot), idepth[0] = (1 / D) * weight and weightSums[0] = weight go out for a passing pixel and 0, 0 for every other one - the
// old path's zero fill plus one atomic add onto 0.0f, which is the addend itself for the values that occur here (a positive quotient times a positive weight).
// The product is rounded on its own (__fmul_rn: it must not contract into the level-1 sums), the quotient is the correctly rounded one, the weight is the
// scatter's expression. Level 1 is a + b + c + d from registers in the reference's order, the levels above are the shared walk. The tiles cover level 0, not
// level 1: the last column / row of an odd w / h and the pixels of partial tiles are written too (the old path zeroes all w*h). VEC: w is even and the plane's
// rows are 8-byte friendly - a quad's row is one 8-byte access, so a wave reads and writes four pairs of contiguous 128-byte rows; otherwise word by word.
// n_seeded: every workgroup adds {1 ticket | its passing pixels} to ONE 64-bit word with one atomic; the one that draws the last ticket publishes the total to
// the host-mapped block (read behind the pc_n flag, which a later kernel of the stream stores) and re-arms the word for the next stream-ordered call. These
// atomics queue at the one address, some 11 ns each: 5 of the kernel's 10 us at 1224x368 (435 workgroups). Two other forms were measured and are slower: one
// atomic a wave issued ahead of the stores (27 us), and plain per-wave stores to a host-mapped array that the host adds up (the kernel's end waits for the
// writes to arrive: 6 to 35 us, and the call 30 us longer).
constexpr int kTrkSeedOut = 96 + NALO_MAX_LEVELS + 2;    // n_seeded in trk_out_host: behind pc_n [96 ..] and its flag [96 + NALO_MAX_LEVELS]
struct TrkDepthSeed {
    const char* depth; long long sy, sx;              // the plane: element (u, v) at depth + v * sy + u * sx
    const float* absg;                                // level-0 absSquaredGrad of the slot (read only with min_grad != 0)
    float min_depth, max_depth, hdi, min_grad;
    int step;
    unsigned long long* ticket;                       // {arrived workgroups << 32 | passing pixels}, zero between calls
    double* n_out;                                    // host-mapped
};
template <bool VEC>
__global__ __launch_bounds__(256) void trk_seed_depth_kernel(TrkLevels P, TrkDepthSeed S) {
    __shared__ float sid[2][16 * 16], sws[2][16 * 16];
    __shared__ int wave_cnt[4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int w0 = P.wl[0], h0 = P.hl[0];
    const int tiles_x = (w0 + 31) / 32;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const int x = bx * 16 + tx, y = by * 16 + ty;     // the lane's level-1 pixel; its quad is (2x .. 2x+1, 2y .. 2y+1)
    const int u0 = 2 * x, v0 = 2 * y;
    const float weight = sqrtf((float)(1e-3 / ((double)S.hdi + 1e-12)));
    const bool grad = S.min_grad != 0.0f;
    // in-image flags of the quad's pixels, row-major: with VEC the two pixels of a row stand or fall together
    const bool in[4] = {u0 < w0 && v0 < h0, u0 + 1 < w0 && v0 < h0, u0 < w0 && v0 + 1 < h0, u0 + 1 < w0 && v0 + 1 < h0};
    float D[4] = {0.f, 0.f, 0.f, 0.f}, G[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const char* row = S.depth + (long long)(v0 + r) * S.sy + (long long)u0 * S.sx;
        const size_t o = (size_t)u0 + (size_t)w0 * (v0 + r);
        if (VEC) {
            if (in[2 * r]) {
                const float2 d = *reinterpret_cast<const float2*>(row); D[2 * r] = d.x; D[2 * r + 1] = d.y;
                if (grad) { const float2 g = *reinterpret_cast<const float2*>(S.absg + o); G[2 * r] = g.x; G[2 * r + 1] = g.y; }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (in[2 * r + k]) {
                    D[2 * r + k] = *reinterpret_cast<const float*>(row + k * S.sx);
                    if (grad) G[2 * r + k] = S.absg[o + k];
                }
        }
    }
    bool on[4] = {true, true, true, true};
    if (S.step != 1) {                                // uniform; x % step == 0 for x = c + 1 iff c % step == step - 1
        const int ru = u0 % S.step, rv = v0 % S.step;
        const bool su0 = ru == 0, su1 = ru + 1 == S.step, sv0 = rv == 0, sv1 = rv + 1 == S.step;
        on[0] = su0 && sv0; on[1] = su1 && sv0; on[2] = su0 && sv1; on[3] = su1 && sv1;
    }
    float pi[4], pw[4];
    int passed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the predicate of include/nalo_gpu.h: float comparisons as they stand (a NaN fails each of them)
        const bool pass = in[k] && on[k] && D[k] >= S.min_depth && D[k] <= S.max_depth && (!grad || G[k] >= S.min_grad);
        pi[k] = pass ? __fmul_rn(__fdiv_rn(1.0f, D[k]), weight) : 0.0f;
        pw[k] = pass ? weight : 0.0f;
        passed += pass ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const size_t o = (size_t)u0 + (size_t)w0 * (v0 + r);
        if (VEC) {
            if (in[2 * r]) {
                *reinterpret_cast<float2*>(P.id[0] + o) = make_float2(pi[2 * r], pi[2 * r + 1]);
                *reinterpret_cast<float2*>(P.ws[0] + o) = make_float2(pw[2 * r], pw[2 * r + 1]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (in[2 * r + k]) { P.id[0][o + k] = pi[2 * r + k]; P.ws[0][o + k] = pw[2 * r + k]; }
        }
    }
    float a = 0.f, b = 0.f;
    if (P.L > 1 && x < P.wl[1] && y < P.hl[1]) {      // all four pixels are inside then
        a = pi[0] + pi[1] + pi[2] + pi[3];
        b = pw[0] + pw[1] + pw[2] + pw[3];
        P.id[1][x + y * P.wl[1]] = a; P.ws[1][x + y * P.wl[1]] = b;
    }
    // the count: the four waves' sums meet in LDS, one atomic a workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) passed += __shfl_xor(passed, o);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = passed;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long mine = (unsigned long long)(wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]);
        const unsigned long long old = __hip_atomic_fetch_add(S.ticket, (1ull << 32) | mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old >> 32) == gridDim.x - 1ull) {        // the last workgroup: every other one's add is in `old`
            __hip_atomic_store(S.n_out, (double)((old & 0xffffffffull) + mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(S.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    trk_sum_walk_up(P, bx, by, tx, ty, a, b, sid, sws);
}
// steps 3/4 (:437-489): 1-px dilation, diagonal (levels 0,1) or axis (levels >= 2), flat-index neighbours. The reference dilates in place
// against a backup copy of the weights; here the undilated weights ws stay read-only and the result goes to wb (the buffers swap roles
// afterwards), so no copy is needed. idepth is written in place: it is read only where ws > 0 and written only where ws <= 0.
__global__ __launch_bounds__(256) void trk_dilate_all_kernel(TrkLevels P) {
    int l = 0;
    while (l + 1 < P.L && (int)blockIdx.x >= P.blk0[l + 1]) ++l;
    const int wl = P.wl[l], npx = wl * P.hl[l];
    const int i = (blockIdx.x - P.blk0[l]) * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    float* __restrict__ id = P.id[l]; const float* __restrict__ bak = P.ws[l]; float* __restrict__ out = P.wb[l];
    const float own = bak[i];
    float res = own;
    if (i >= wl && i < npx - wl && !(own > 0)) {
        const int diag = l < 2;
        const int o0 = diag ? 1 + wl : 1, o1 = diag ? -1 - wl : -1, o2 = diag ? wl - 1 : wl, o3 = diag ? -wl + 1 : -wl;
        // the reference reads one element before/after the array at the first/last pixel of this range
        // (i-1-wl = -1, i+1+wl = w*h): those two taps are outside the image and are skipped here.
        float sum = 0, num = 0, numn = 0;
#define NALO_TAP(o) { const int j = i + (o); if (j >= 0 && j < npx) { const float b = bak[j]; if (b > 0) { sum += id[j]; num += b; numn++; } } }
        NALO_TAP(o0) NALO_TAP(o1) NALO_TAP(o2) NALO_TAP(o3)
#undef NALO_TAP
        if (numn > 0) { id[i] = sum / numn; res = num / numn; }
    }
    out[i] = res;
}
// step 5 (:493-538): normalise + ordered (raster) compaction into pc_*. Pass 0 counts per block, pass 1 writes. (ws = the dilated weights.)
constexpr int kCompactChunk = 2048;          // interior elements per block (8 rounds of 256)
// A block takes its 8 rounds of 256 elements in ONE sweep: all loads of a lane's eight elements are in flight together, the eight ballots give the per-(round,
// wave) counts, one LDS scan of those 32 counts gives every lane its output slot - element order (round, then lane) as in the reference's double loop. (The
// rounds used to be serial, each a dependent load, a ballot and three barriers: 9.5 + 11.6 us for the two passes on a 1224x368 frame.)
template <int WRITE>
__global__ __launch_bounds__(256) void trk_compact_all_kernel(TrkLevels P, int* __restrict__ scan) {
    constexpr int R = kCompactChunk / 256;
    __shared__ int cnt[R * 4 + 1];
    int l = 0;
    while (l + 1 < P.L && (int)blockIdx.x >= P.blk0[l + 1]) ++l;
    const int chunk = blockIdx.x - P.blk0[l], nb = P.blk0[l + 1] - P.blk0[l];
    const int wl = P.wl[l], hl = P.hl[l];
    float* __restrict__ id = P.id[l]; float* __restrict__ ws = P.wb[l]; const float4* __restrict__ dIref = P.dI[l];
    int* counts = scan + P.scan0[l]; const int* offsets = counts + nb;
    const int iw = wl - 4, ih = hl - 4, total = iw * ih;            // interior y in [2,hl-2), x in [2,wl-2)
    const int base = chunk * kCompactChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int idx[R]; float wsv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = base + r * 256 + threadIdx.x;
        idx[r] = -1; wsv[r] = 0.f;
        if (e < total) { const int y = e / iw, x = e - y * iw; idx[r] = (x + 2) + (y + 2) * wl; wsv[r] = ws[idx[r]]; }
    }
    float val[R], col[R]; bool keep[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        val[r] = 0.f; col[r] = 0.f; keep[r] = false;
        if (idx[r] >= 0 && wsv[r] > 0) { val[r] = id[idx[r]]; col[r] = dIref[idx[r]].x; }
    }
    int rank[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (idx[r] >= 0 && wsv[r] > 0) { val[r] = val[r] / wsv[r]; keep[r] = isfinite(col[r]) && (val[r] > 0); }
        const unsigned long long m = __ballot(keep[r]);
        rank[r] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) cnt[r * 4 + wave] = __popcll(m);
    }
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < R * 4; ++k) t += cnt[k]; counts[chunk] = t; }
        return;
    }
    if (threadIdx.x < 64) {                                         // exclusive scan of the R x 4 counts (round-major), one wave
        const int v = lane < R * 4 ? cnt[lane] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        if (lane < R * 4) cnt[lane] = inc - v;
    }
    __syncthreads();
    const int first = offsets[chunk];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = idx[r];
        if (i < 0) continue;
        if (wsv[r] > 0) {
            id[i] = keep[r] ? val[r] : -1.f; if (keep[r]) ws[i] = 1.f;                 // `continue` skips weightSums=1 (:524-528)
            if (keep[r]) {
                const int o = first + cnt[r * 4 + wave] + rank[r];
                const int y = i / wl, x = i - y * wl;
                P.pu[l][o] = (float)x; P.pv[l][o] = (float)y; P.pid[l][o] = val[r]; P.pcol[l][o] = col[r];
            }
        } else { id[i] = -1.f; ws[i] = 1.f; }
    }
}
// exclusive scan of the block counts of every level by one block (a few hundred counts); the per-level totals go to host-mapped memory
// followed by the sequence number the host polls on: pc_n reaches the host without a stream synchronisation
__global__ __launch_bounds__(1024) void trk_scan_all_kernel(TrkLevels P, int* __restrict__ scan, double* __restrict__ out, double seq) {
    __shared__ int part[4][4];
    // four levels at a time, 256 lanes each (the levels used to be scanned one after the other by the whole block)
    const int grp = threadIdx.x >> 8, t = threadIdx.x & 255, lane = threadIdx.x & 63, wave = t >> 6;
    for (int l0 = 0; l0 < P.L; l0 += 4) {
        const int l = l0 + grp;
        const bool on = l < P.L;
        const int nb = on ? P.blk0[l + 1] - P.blk0[l] : 0;
        const int* counts = scan + (on ? P.scan0[l] : 0); int* offsets = scan + (on ? P.scan0[l] : 0) + nb;
        const int per = (nb + 255) / 256, lo = min(t * per, nb), hi = min(lo + per, nb);
        int s = 0;
        for (int i = lo; i < hi; ++i) s += counts[i];
        int v = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int nbv = __shfl_up(v, off); if (lane >= off) v += nbv; }
        if (lane == 63) part[grp][wave] = v;
        __syncthreads();
        int wpre = 0, tot = 0;
        for (int k = 0; k < 4; ++k) { const int pv = part[grp][k]; if (k < wave) wpre += pv; tot += pv; }
        int run = wpre + v - s;
        for (int i = lo; i < hi; ++i) { offsets[i] = run; run += counts[i]; }
        if (on && t == 0) { offsets[nb] = tot; out[l] = (double)tot; }
        __syncthreads();
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&out[NALO_MAX_LEVELS], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// dense=1: the plane-sampled points CoarseTracker::makeCoarseDepthL0 appends to the level-0 cloud (reference src/FullSystem/CoarseTracker.cpp:628-655). For one
// mask cluster with fitted plane (dir, dis): every pixel of its bounding box [minx,maxx) x [miny,maxy) with x % 5 == 0, y % 5 == 0 and mask == refMaskColor
// becomes a point with new_idepth = (dir^T Ki (x, y, 1)) / -dis, colour = I_ref(x, y), in the reference's loop order (x outer, y inner). The reference stores
// point k at index pc_n + 1 + k and then counts pc_n += 1 per point (:646-650): slot [old pc_n] is never written (stale heap there, ZERO here) and the last
// sampled point falls just outside the count. Reproduced. ONE workgroup: the candidates (multiples of 5: <= w h / 25) are compacted in order, chunk by
// chunk, with ballot counts and an LDS scan over the 16 waves.
// One cluster's points, by all 1024 lanes of the workgroup (wave_cnt[16] and base_s in LDS); returns the growth of pc_n.
__device__ __forceinline__ int trk_append_plane_body(int* wave_cnt, int* base_s, const float* __restrict__ mask, const float4* __restrict__ dIref, int w, float d0, float d1, float d2,
                                                     float dis, float Ki00, float Ki02, float Ki11, float Ki12, float refColor, int x0, int nx, int y0, int ny, int n0,
                                                     float* __restrict__ pu, float* __restrict__ pv, float* __restrict__ pid, float* __restrict__ pcol) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __syncthreads();
    if (tid == 0) { *base_s = 0; pu[n0] = 0.f; pv[n0] = 0.f; pid[n0] = 0.f; pcol[n0] = 0.f; }
    __syncthreads();
    // dir^T * Ki as Eigen evaluates it (row vector times matrix, then times the point): t = dir^T Ki
    const float t0 = d0 * Ki00 + d1 * 0.f + d2 * 0.f, t1 = d0 * 0.f + d1 * Ki11 + d2 * 0.f, t2 = d0 * Ki02 + d1 * Ki12 + d2 * 1.f;
    const int total = nx * ny;
    for (int c0 = 0; c0 < total; c0 += 1024) {
        const int j = c0 + tid;
        bool take = false; int x = 0, y = 0;
        if (j < total) { x = x0 + 5 * (j / ny); y = y0 + 5 * (j % ny); take = mask[x + y * w] == refColor; }
        const unsigned long long b = __ballot(take);
        if (lane == 0) wave_cnt[wv] = __popcll(b);
        __syncthreads();
        int off = *base_s;
        for (int k = 0; k < wv; ++k) off += wave_cnt[k];
        if (take) {
            const int at = n0 + 1 + off + __popcll(b & ((1ull << lane) - 1ull));
            float nid = t0 * (float)x + t1 * (float)y + t2 * 1.f;
            nid /= -dis;
            pu[at] = (float)x; pv[at] = (float)y; pid[at] = nid; pcol[at] = dIref[x + y * w].x;
        }
        __syncthreads();
        if (tid == 0) { int s = 0; for (int k = 0; k < 16; ++k) s += wave_cnt[k]; *base_s += s; }
        __syncthreads();
    }
    return *base_s;
}
__global__ __launch_bounds__(1024) void trk_append_plane_kernel(const float* __restrict__ mask, const float4* __restrict__ dIref, int w, float d0, float d1, float d2, float dis,
                                                                float Ki00, float Ki02, float Ki11, float Ki12, float refColor, int x0, int nx, int y0, int ny, int n0,
                                                                float* __restrict__ pu, float* __restrict__ pv, float* __restrict__ pid, float* __restrict__ pcol, int* __restrict__ n_out) {
    __shared__ int wave_cnt[16];
    __shared__ int base_s;
    const int added = trk_append_plane_body(wave_cnt, &base_s, mask, dIref, w, d0, d1, d2, dis, Ki00, Ki02, Ki11, Ki12, refColor, x0, nx, y0, ny, n0, pu, pv, pid, pcol);
    if (threadIdx.x == 0) *n_out = added;
}
// nalo_trk_fit_planes(append = 1): the loop of CoarseTracker.cpp:582-666 over the cluster records the fit has just written, in their order, each cluster with the
// checks and the arithmetic of nalo_trk_append_plane_points on that record (the same body). hdr[1] != 0: the fit refused; hdr[4]: clusters; nothing is appended
// with fewer than 4 (:563) or when the caller's array cannot take every record. hdr[5] receives pc_n[0]; a cluster the buffer cannot hold sets bit 4 of hdr[1] and ends the loop.
__global__ __launch_bounds__(1024) void trk_append_clusters_kernel(const float* __restrict__ mask, const float4* __restrict__ dIref, int w, int h, float Ki00, float Ki02, float Ki11,
                                                                   float Ki12, nalo_plane_cluster* __restrict__ rec, int* __restrict__ hdr, int cap_clusters, int n0, int pc_cap,
                                                                   float* __restrict__ pu, float* __restrict__ pv, float* __restrict__ pid, float* __restrict__ pcol) {
    __shared__ int wave_cnt[16];
    __shared__ int base_s;
    const int C = hdr[4];
    int n_cur = n0;
    if (hdr[1] == 0 && C >= 4 && C <= cap_clusters) {
        for (int r = 0; r < C; ++r) {                                   // every condition below is uniform over the workgroup
            const int fitted = rec[r].fitted, minx = rec[r].rect[0], maxx = rec[r].rect[1], miny = rec[r].rect[2], maxy = rec[r].rect[3];
            const float mv = rec[r].mask_value, dis = rec[r].plane[3];
            const int refMaskColor = (int)fminf(fmaxf(mv, -2.0e9f), 2.0e9f);                      // `int refMaskColor = clusters[i][0][3]` (:632)
            if (!fitted || maxx > w - 1 || minx < 1 || maxy > h - 1 || miny < 1 || refMaskColor == 0 || dis == 0.f) continue;
            const int x0 = ((minx + 4) / 5) * 5, y0 = ((miny + 4) / 5) * 5;
            const int nx = x0 < maxx ? (maxx - 1 - x0) / 5 + 1 : 0, ny = y0 < maxy ? (maxy - 1 - y0) / 5 + 1 : 0;
            if ((long long)n_cur + 2 + (long long)nx * ny > (long long)pc_cap) { if (threadIdx.x == 0) hdr[1] |= 4; break; }
            if (nx == 0 || ny == 0) continue;
            const int added = trk_append_plane_body(wave_cnt, &base_s, mask, dIref, w, rec[r].plane[0], rec[r].plane[1], rec[r].plane[2], dis, Ki00, Ki02, Ki11, Ki12,
                                                    (float)refMaskColor, x0, nx, y0, ny, n_cur, pu, pv, pid, pcol);
            if (threadIdx.x == 0) rec[r].appended = added;
            n_cur += added;
        }
    }
    if (threadIdx.x == 0) hdr[5] = n_cur;
}
int trk_append_clusters_launch(nalo_ctx* c, const float* mask, const float4* dIref, nalo_plane_cluster* rec, int* hdr, int cap_clusters) {
    const float fx = c->fx[0], fy = c->fy[0], cx = c->cx[0], cy = c->cy[0];
    trk_append_clusters_kernel<<<1, 1024, 0, c->stream>>>(mask, dIref, c->w, c->h, 1.0f / fx, -cx / fx, 1.0f / fy, -cy / fy, rec, hdr, cap_clusters, c->pc_n[0], (int)c->pc_u[0].cap,
                                                          c->pc_u[0].p, c->pc_v[0].p, c->pc_id[0].p, c->pc_col[0].p);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}
int trk_append_plane_launch(nalo_ctx* c, const float* mask, const float4* dIref, const float dir[3], float dis, float refColor, int x0, int nx, int y0, int ny, int n0, int* n_dev) {
    const float fx = c->fx[0], fy = c->fy[0], cx = c->cx[0], cy = c->cy[0];
    trk_append_plane_kernel<<<1, 1024, 0, c->stream>>>(mask, dIref, c->w, dir[0], dir[1], dir[2], dis, 1.0f / fx, -cx / fx, 1.0f / fy, -cy / fy, refColor, x0, nx, y0, ny, n0,
                                                       c->pc_u[0].p, c->pc_v[0].p, c->pc_id[0].p, c->pc_col[0].p, n_dev);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

// makeCoarseDepthL0 on the host side, in three parts: the level table and the buffers (trk_ref_prepare), a seed that leaves idepth[] / weightSums[] of every
// level as steps 1 and 2 do (the scatter of trk_build_ref, the depth plane of trk_build_ref_from_depth), and steps 3-5 with the pc_n poll (trk_ref_finish).
struct TrkRefPlan {
    TrkLevels P;
    int dil_blocks, cmp_blocks;
    int dil0[NALO_MAX_LEVELS + 1], cmp0[NALO_MAX_LEVELS + 1];
};
static int trk_ref_prepare(nalo_ctx* c, TrkRefPlan& R) {
    const int L = c->levels;
    std::memset(&R, 0, sizeof(R));
    TrkLevels& P = R.P;
    P.L = L;
    int dil_blocks = 0, cmp_blocks = 0, scan_total = 0;
    for (int l = 0; l < L; ++l) {
        const size_t npx = (size_t)c->wl[l] * c->hl[l];
        NALO_HIP(c, c->trk_idepth[l].reserve(npx)); NALO_HIP(c, c->trk_wsum[l].reserve(npx)); NALO_HIP(c, c->trk_wbak[l].reserve(npx));
        NALO_HIP(c, c->pc_u[l].reserve(npx)); NALO_HIP(c, c->pc_v[l].reserve(npx)); NALO_HIP(c, c->pc_id[l].reserve(npx)); NALO_HIP(c, c->pc_col[l].reserve(npx));
        P.id[l] = c->trk_idepth[l].p; P.ws[l] = c->trk_wsum[l].p; P.wb[l] = c->trk_wbak[l].p; P.dI[l] = c->slots[c->slot_ref].dI[l].p;
        P.pu[l] = c->pc_u[l].p; P.pv[l] = c->pc_v[l].p; P.pid[l] = c->pc_id[l].p; P.pcol[l] = c->pc_col[l].p;
        P.wl[l] = c->wl[l]; P.hl[l] = c->hl[l];
        R.dil0[l] = dil_blocks; dil_blocks += (int)((npx + 255) / 256);
        const int total = (c->wl[l] - 4) * (c->hl[l] - 4);
        const int nb = total > 0 ? (total + kCompactChunk - 1) / kCompactChunk : 0;
        R.cmp0[l] = cmp_blocks; cmp_blocks += nb;
        P.scan0[l] = scan_total; scan_total += 2 * nb + 2;
    }
    R.dil0[L] = dil_blocks; R.cmp0[L] = cmp_blocks; P.scan0[L] = scan_total;
    R.dil_blocks = dil_blocks; R.cmp_blocks = cmp_blocks;
    NALO_HIP(c, c->scan_tmp.reserve((size_t)scan_total));
    return NALO_OK;
}
static int trk_ref_finish(nalo_ctx* c, TrkRefPlan& R) {
    TrkLevels& P = R.P;
    const int L = P.L;
    for (int l = 0; l <= L; ++l) P.blk0[l] = R.dil0[l];
    trk_dilate_all_kernel<<<R.dil_blocks, 256, 0, c->stream>>>(P);
    for (int l = 0; l <= L; ++l) P.blk0[l] = R.cmp0[l];
    double* const dout = c->trk_out_host.dev;
    const double seq = (double)(++c->trk_seq);
    if (R.cmp_blocks > 0) trk_compact_all_kernel<0><<<R.cmp_blocks, 256, 0, c->stream>>>(P, c->scan_tmp.p);
    trk_scan_all_kernel<<<1, 1024, 0, c->stream>>>(P, c->scan_tmp.p, dout + 96, seq);
    if (R.cmp_blocks > 0) trk_compact_all_kernel<1><<<R.cmp_blocks, 256, 0, c->stream>>>(P, c->scan_tmp.p);
    NALO_HIP(c, hipGetLastError());
    for (int l = 0; l < L; ++l) std::swap(c->trk_wsum[l], c->trk_wbak[l]);      // the dilated (then normalised) weights are the level's weightSums now
    if (!poll_flag(c, &c->trk_out_host.p[96 + NALO_MAX_LEVELS], seq)) return NALO_ERR_HIP;   // pc_n for the host; the point clouds follow in stream order
    for (int l = 0; l < L; ++l) c->pc_n[l] = (int)c->trk_out_host.p[96 + l];
    return NALO_OK;
}

int trk_build_ref(nalo_ctx* c, int n, const float* dKu, const float* dKv, const float* dId, const float* dHdi) {
    TrkRefPlan R;
    { const int rc = trk_ref_prepare(c, R); if (rc) return rc; }
    const TrkLevels& P = R.P;
    const int n0 = c->wl[0] * c->hl[0];
    NALO_HIP(c, c->trk_cnt.reserve((size_t)n0 + 2 + std::max(n, 0)));        // hits per level-0 pixel, then the hot list's counter, its ticket and room for every residual
    trk_zero2_kernel<<<(n0 + 255) / 256, 256, 0, c->stream>>>(P.id[0], P.ws[0], c->trk_cnt.p, n0);
    if (n > 0) {
        trk_scatter_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(dKu, dKv, dId, dHdi, n, c->wl[0], c->hl[0], P.id[0], P.ws[0], c->trk_cnt.p);
        trk_scatter_hot_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(dKu, dKv, dId, dHdi, n, c->wl[0], c->hl[0], P.id[0], P.ws[0], c->trk_cnt.p, c->trk_cnt.p + n0);
    }
    if (P.L > 1) trk_sum_down_all_kernel<<<((c->wl[1] + 15) / 16) * ((c->hl[1] + 15) / 16), 256, 0, c->stream>>>(P);
    return trk_ref_finish(c, R);
}

// nalo_trk_set_ref_from_depth behind its checks (host_api.hip): c->slot_ref is the new reference slot and the main stream already waits for the producer
int trk_build_ref_from_depth(nalo_ctx* c, const nalo_dev_plane& d, float min_depth, float max_depth, float hdi, int step, float min_grad, int* n_seeded) {
    TrkRefPlan R;
    { const int rc = trk_ref_prepare(c, R); if (rc) return rc; }
    TrkDepthSeed S;
    S.depth = static_cast<const char*>(d.ptr); S.sy = d.stride_y; S.sx = d.stride_x;
    S.absg = c->slots[c->slot_ref].absg[0].p;
    S.min_depth = min_depth; S.max_depth = max_depth; S.hdi = hdi; S.min_grad = min_grad; S.step = step;
    const int w0 = c->wl[0], h0 = c->hl[0];
    const int blocks = ((w0 + 31) / 32) * ((h0 + 31) / 32);
    if (!c->trk_seed_ticket.p) { NALO_HIP(c, c->trk_seed_ticket.reserve(1)); NALO_HIP(c, hipMemsetAsync(c->trk_seed_ticket.p, 0, 8, c->stream)); }
    S.ticket = c->trk_seed_ticket.p; S.n_out = c->trk_out_host.dev + kTrkSeedOut;
    const bool vec = w0 % 2 == 0 && d.stride_x == 4 && d.stride_y % 8 == 0 && (uintptr_t)d.ptr % 8 == 0;
    if (vec) trk_seed_depth_kernel<true><<<blocks, 256, 0, c->stream>>>(R.P, S);
    else trk_seed_depth_kernel<false><<<blocks, 256, 0, c->stream>>>(R.P, S);
    { const int rc = trk_ref_finish(c, R); if (rc) return rc; }
    *n_seeded = (int)c->trk_out_host.p[kTrkSeedOut];            // stored by the seed kernel, in stream order before the flag the poll has just seen
    return NALO_OK;
}

}  // namespace nalo
