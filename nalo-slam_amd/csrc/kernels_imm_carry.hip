// The resident immature-point set across a keyframe, on the device (nalo_imm_resident_carry; reference paths relative to src/FullSystem/):
//   (A) FullSystem::activatePointsMT, steps 2-4 as they end for the immature set     FullSystem.cpp:805-876, :893-917, and the compaction :920-931
//   (C) a frame leaves: its ImmaturePoints go with it (FrameHessian dtor)             HessianBlocks.cpp:117
//   (B) FullSystem::makeNewTraces                                                     FullSystem.cpp:1677-1687 with the constructor of imm_ctor_body.h
//
// The compaction :920-931 fills every hole of a host's vector with the vector's back and re-examines the slot, so null backs are consumed one by one.
// In closed form, with p a point's rank in its host's vector, kb(p) the kept points of that host before p and m the host's kept points: a kept point
// with p < m stays at p; the holes below m, in ascending order, take the kept points at p >= m from the back, i.e. the kept point at p >= m goes to the
// hole with hole index m - 1 - kb(p), and the hole at q has hole index q - kb(q). (A kept point below m is never the back when a hole is filled: the
// vector would then be shorter than its kept points.) tests/imm_carry_model.py runs the loop as written; tests/test_imm_carry_gpu.py compares.
//
// Hosts interleave in storage, so p and kb are segmented ranks:
//   immc_count_kernel   per workgroup and OLD host: points, kept points; per workgroup: points (A) deletes; per workgroup of the append list: live
//                       entries and entries that become points (inside makeNewTraces' bounds, finite energyTH: the constructor runs for the verdict, kept in arank[])
//   scan_ints_launch    one exclusive scan over all of those counts (a few thousand words, one workgroup)
//   immc_place_kernel   ballot ranks inside the workgroup + the scanned offsets give p, kb, m: src[new slot] = old index for the points that stay, an
//                       indirection through mover[] for the holes below m, the list entry for appended points
//   immc_gather_kernel  one thread per NEW slot moves the 30 resident rows and my_type, or runs the constructor for an appended point
// Order never comes from an atomic: LDS integer atomics count, everything else is a ballot rank or a scanned offset. Stores are plain vector stores.
// Built without FMA contraction (the constructor's arithmetic is the reference's).
#include "nalo_internal.h"
#include "imm_ctor_body.h"

namespace nalo {

constexpr int kCarryAppendBit = 0x40000000;

__device__ __forceinline__ int immc_wave_count(bool b) { return __popcll(__ballot(b)); }

// 0: the point stays, 1: (A) deletes it, 2: it leaves with its host (C). host: its OLD host index.
__device__ __forceinline__ int immc_class(const ImmCarryParams& P, int i, int& host) {
    const size_t N = (size_t)P.n;
    host = min(max(((const int*)(P.res + 22 * N))[i], 0), P.H - 1);           // the host checked the range (its copy of host_idx): a clamp, never an index outside
    const int code = P.code ? P.code[i] : 0;
    if (code == 1 || (code == 2 && ((const int*)(P.res + 25 * N))[i] == IPS_OOB)) return 1;     // :908: result 0 deletes only what the trace left OOB
    return P.host_map[host] < 0 ? 2 : 0;
}
// an entry of the append list: live = the map is non-zero there (:1681); true when makeNewTraces' loop bounds reach it (:1677-1678)
__device__ __forceinline__ bool immc_entry(const ImmCarryParams& P, int k, bool& live, int& x, int& y, int& st) {
    const int e = P.list[k];
    st = (int)((unsigned)e >> 28);
    const int idx = e & 0x0FFFFFFF;
    x = idx % P.w; y = idx / P.w;
    live = st != 0;
    return live && x >= kPatternPadding + 1 && x < P.w - kPatternPadding - 2 && y >= kPatternPadding + 1 && y < P.h - kPatternPadding - 2;
}

// cnt: [T: H x nb][K: H x nb][A: mb][L: mb][D: nb], then the total
__global__ __launch_bounds__(256) void immc_count_kernel(ImmCarryParams P) {
    __shared__ int hc[2][NALO_MAX_WINDOW];
    __shared__ int ac[3];
    if (threadIdx.x < NALO_MAX_WINDOW) { hc[0][threadIdx.x] = 0; hc[1][threadIdx.x] = 0; }
    if (threadIdx.x < 3) ac[threadIdx.x] = 0;
    __syncthreads();
    const int K0 = P.H * P.nb, A0 = 2 * K0, L0 = A0 + P.mb, D0 = L0 + P.mb;
    if ((int)blockIdx.x < P.nb) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        bool del = false;
        if (i < P.n) {
            int host;
            const int cl = immc_class(P, i, host);
            atomicAdd(&hc[0][host], 1);
            if (cl == 0) atomicAdd(&hc[1][host], 1);
            del = cl == 1;
        }
        const int nd = immc_wave_count(del);
        if (nd && (threadIdx.x & 63) == 0) atomicAdd(&ac[2], nd);
        __syncthreads();
        if ((int)threadIdx.x < P.H) { P.cnt[threadIdx.x * P.nb + blockIdx.x] = hc[0][threadIdx.x]; P.cnt[K0 + threadIdx.x * P.nb + blockIdx.x] = hc[1][threadIdx.x]; }
        if (threadIdx.x == 0) P.cnt[D0 + blockIdx.x] = ac[2];
    } else {
        const int b = blockIdx.x - P.nb, k = b * 256 + threadIdx.x;
        bool live = false, acc = false;
        if (k < P.m) {
            int x, y, st;
            if (immc_entry(P, k, live, x, y, st)) acc = isfinite(imm_ctor(P.dI, P.w, x, y).energyTH);     // :1684
            P.arank[k] = acc;                                                   // the verdict, for immc_place_kernel (which puts the entry's name there)
        }
        const int na = immc_wave_count(acc), nl = immc_wave_count(live);
        if ((threadIdx.x & 63) == 0) { if (na) atomicAdd(&ac[0], na); if (nl) atomicAdd(&ac[1], nl); }
        __syncthreads();
        if (threadIdx.x == 0) { P.cnt[A0 + b] = ac[0]; P.cnt[L0 + b] = ac[1]; }
    }
}

__global__ __launch_bounds__(256) void immc_place_kernel(ImmCarryParams P) {
    __shared__ int wc[4][2][NALO_MAX_WINDOW];
    __shared__ int wa[4][2];
    __shared__ int app_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const int K0 = P.H * P.nb, A0 = 2 * K0, L0 = A0 + P.mb, D0 = L0 + P.mb;
    const int* cnt = P.cnt;
    const int n_app = cnt[L0] - cnt[A0];
    if ((int)blockIdx.x < P.nb) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        int host = -1, cl = 1;
        if (i < P.n) cl = immc_class(P, i, host);
        int rT = 0, rK = 0;
        for (int h = 0; h < P.H; ++h) {
            const unsigned long long mT = __ballot(host == h), mK = __ballot(host == h && cl == 0);
            if (host == h) { rT = __popcll(mT & below); rK = __popcll(mK & below); }
            if (lane == 0) { wc[wave][0][h] = __popcll(mT); wc[wave][1][h] = __popcll(mK); }
        }
        __syncthreads();
        if (host < 0) return;
        const int hb = cnt[host * P.nb];                                        // the host's first rank among all old points in (host, index) order
        int p = cnt[host * P.nb + blockIdx.x] - hb + rT, kb = cnt[K0 + host * P.nb + blockIdx.x] - cnt[K0 + host * P.nb] + rK;
        for (int k = 0; k < wave; ++k) { p += wc[k][0][host]; kb += wc[k][1][host]; }
        const int m = cnt[K0 + (host + 1) * P.nb] - cnt[K0 + host * P.nb];
        const int hn = P.host_map[host];
        const int base = cnt[K0 + host * P.nb] - cnt[K0] + ((P.append_host >= 0 && hn > P.append_host) ? n_app : 0);
        if (cl == 0) {
            if (p < m) P.src[base + p] = i;
            else P.mover[hb + (m - 1 - kb)] = i;                                // the (m - 1 - kb)-th hole of this host takes it
        } else if (p < m) P.src[base + p] = ~(hb + (p - kb));                   // a hole below m: its hole index is p - kb
    } else {
        const int b = blockIdx.x - P.nb, k = b * 256 + threadIdx.x;
        bool live = false, acc = false;
        int x = 0, y = 0, st = 0;
        if (k < P.m) { immc_entry(P, k, live, x, y, st); acc = P.arank[k] != 0; }      // immc_count_kernel's verdict: the constructor is not run again here
        const unsigned long long mA = __ballot(acc), mL = __ballot(live);
        if (lane == 0) { wa[wave][0] = __popcll(mA); wa[wave][1] = __popcll(mL); }
        if (threadIdx.x == 0) {                                                 // the kept points of the new hosts up to and including append_host stand before
            int s = 0;
            for (int h = 0; h < P.H; ++h) if (P.host_map[h] >= 0 && P.host_map[h] <= P.append_host) s += cnt[K0 + (h + 1) * P.nb] - cnt[K0 + h * P.nb];
            app_base = s;
        }
        __syncthreads();
        if (!acc) return;
        int r = cnt[A0 + b] - cnt[A0] + __popcll(mA & below), rl = cnt[L0 + b] - cnt[L0] + __popcll(mL & below);
        for (int q = 0; q < wave; ++q) { r += wa[q][0]; rl += wa[q][1]; }
        P.src[app_base + r] = ~(kCarryAppendBit | k);
        P.arank[k] = P.rank_live ? rl : k;                                      // what nalo_imm_resident_carry_map names: the entry of the list the caller sees
    }
    (void)D0;
}

__global__ __launch_bounds__(256) void immc_gather_kernel(ImmCarryParams P) {
    const int K0 = P.H * P.nb, A0 = 2 * K0, L0 = A0 + P.mb, D0 = L0 + P.mb, M = D0 + P.nb;
    const int* cnt = P.cnt;
    const int n_app = cnt[L0] - cnt[A0], n_kept = cnt[A0] - cnt[K0], n_new = n_kept + n_app;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) {                                                               // {n_new, deleted by (A), dropped with their host, appended, per new host}
        const int n_del = cnt[M] - cnt[D0];
        P.out[0] = n_new; P.out[1] = n_del; P.out[2] = P.n - n_del - n_kept; P.out[3] = n_app;
        for (int h = 0; h < NALO_MAX_WINDOW; ++h) P.out[4 + h] = 0;
        for (int h = 0; h < P.H; ++h) if (P.host_map[h] >= 0) P.out[4 + P.host_map[h]] = cnt[K0 + (h + 1) * P.nb] - cnt[K0 + h * P.nb];
        if (P.append_host >= 0) P.out[4 + P.append_host] += n_app;
    }
    if (j >= n_new) return;
    const size_t N = (size_t)P.n, Nn = (size_t)n_new;
    int s = P.src[j];
    if (s < 0 && !(~s & kCarryAppendBit)) s = P.mover[~s];
    // the set's layout (nalo_imm_resident_set): u | v | color[8] | weights[8] | gradH[3] | energyTH | host | idmin | idmax | status | quality | lastTraceUV[2] | interval,
    // one block of N entries each, the entries of a block point by point
    float* o = P.res2;
    if (s >= 0) {
        const float* in = P.res;
        const size_t t = (size_t)s;
        o[j] = in[t]; o[Nn + j] = in[N + t];
#pragma unroll
        for (int q = 0; q < 8; ++q) { o[2 * Nn + 8 * j + q] = in[2 * N + 8 * t + q]; o[10 * Nn + 8 * j + q] = in[10 * N + 8 * t + q]; }
#pragma unroll
        for (int q = 0; q < 3; ++q) o[18 * Nn + 3 * j + q] = in[18 * N + 3 * t + q];
        o[21 * Nn + j] = in[21 * N + t];
        ((int*)o)[22 * Nn + j] = P.host_map[min(max(((const int*)in)[22 * N + t], 0), P.H - 1)];
#pragma unroll
        for (int r = 23; r < 27; ++r) o[r * Nn + j] = in[r * N + t];            // idmin idmax status quality
        o[27 * Nn + 2 * j] = in[27 * N + 2 * t]; o[27 * Nn + 2 * j + 1] = in[27 * N + 2 * t + 1];
        o[29 * Nn + j] = in[29 * N + t];
        P.type2[j] = P.type ? P.type[t] : 0.f;
        P.src[j] = s;
        return;
    }
    const int k = ~s & (kCarryAppendBit - 1);
    bool live; int x, y, st;
    immc_entry(P, k, live, x, y, st);
    const ImmCtor c = imm_ctor(P.dI, P.w, x, y);
    o[j] = (float)x; o[Nn + j] = (float)y;                                      // ImmaturePoint.cpp:32-60
#pragma unroll
    for (int q = 0; q < 8; ++q) { o[2 * Nn + 8 * j + q] = c.color[q]; o[10 * Nn + 8 * j + q] = c.weights[q]; }
    o[18 * Nn + 3 * j] = c.gxx; o[18 * Nn + 3 * j + 1] = c.gxy; o[18 * Nn + 3 * j + 2] = c.gyy;
    o[21 * Nn + j] = c.energyTH;
    ((int*)o)[22 * Nn + j] = P.append_host;
    o[23 * Nn + j] = 0.f; o[24 * Nn + j] = __int_as_float(0x7FC00000);          // idepth_min = 0, idepth_max = NAN
    ((int*)o)[25 * Nn + j] = IPS_UNINITIALIZED; o[26 * Nn + j] = 10000.f;
    o[27 * Nn + 2 * j] = -1.f; o[27 * Nn + 2 * j + 1] = -1.f; o[29 * Nn + j] = 0.f;
    P.type2[j] = (float)st;                                                    // my_type = the selector's status (:1683)
    P.src[j] = -(P.arank[k] + 2);
}

int imm_carry_launch(nalo_ctx* c, const ImmCarryParams& P) {
    const int slots = P.n + P.m;
    if (slots <= 0) return NALO_OK;
    {
        ProfScope ps(c, "imm_carry_rank");
        immc_count_kernel<<<P.nb + P.mb, 256, 0, c->stream>>>(P);
        int rc = scan_ints_launch(c, P.cnt, 2 * P.H * P.nb + 2 * P.mb + P.nb); if (rc) return rc;
        immc_place_kernel<<<P.nb + P.mb, 256, 0, c->stream>>>(P);
    }
    {
        ProfScope ps(c, "imm_carry_gather");
        immc_gather_kernel<<<(slots + 255) / 256, 256, 0, c->stream>>>(P);
    }
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
