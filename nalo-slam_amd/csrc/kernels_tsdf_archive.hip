// nalo_tsdf_archive_mesh's kernels (include/nalo_gpu.h, "The mesh archive"): the device mesh behind a mesh call is welded onto the archive by vertex identity.
// A vertex's key is (gx, gy, gz, m): the global voxel that owns its edge and the edge number, one int4. Integers and whole words only - no float arithmetic, no
// float atomic - so the file does not depend on the contraction policy.
//   keys       per lane four voxels of the sub-box, as the mesh's passes: the keys of the vertices a voxel owns, at the indices its vbase / vmask give
//   lookup     one lane per piece vertex, read-only: the archived index of its key, or -1 (new); per workgroup the number of new ones
//   scan       of those counts (scan_ints_launch)
//   insert     a new vertex takes index nv + its rank among the new ones, in piece order; xyz, rgba and key are copied as words and the index is put into the table
//   triangles  one lane per piece triangle: three mapped indices behind the archive's triangles
// The table: open addressing, linear probing, a power of two of 32-bit slots, each an archived index or kTsdfArchiveEmpty; a key is compared through the archive's
// key array with one 16-byte load. Within a piece all keys are distinct (an edge carries at most one vertex) and the lookup ran to its end before the insert
// starts, so every inserted key is absent: an insert is an atomicCAS on the first empty slot of its probe sequence, and no lane ever waits for another. Which
// slot a key lands in depends on the order the hardware runs the lanes in and is not observable: indices, positions, colours, keys and triangles are fixed by
// piece order alone. Every probe loop is bounded by the slot count; the host keeps the load at or below one half, so the bound is never met on a sound table,
// and a lane that does meet it (or reads an index the archive does not hold) raises *err and stops: the call fails, nothing spins.
#include "nalo_internal.h"

namespace nalo {

__device__ __forceinline__ unsigned tsdf_archive_hash(const int4& k) {
    unsigned h = (unsigned)k.x * 0x9E3779B1u ^ (unsigned)k.y * 0x85EBCA77u ^ (unsigned)k.z * 0xC2B2AE3Du ^ (unsigned)k.w * 0x27D4EB2Fu;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}
__device__ __forceinline__ bool tsdf_archive_same(const int4& a, const int4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// `index` into the first empty slot of key's probe sequence; false when every slot was taken
__device__ __forceinline__ bool tsdf_archive_insert(int* table, unsigned mask, const int4& key, int index) {
    unsigned h = tsdf_archive_hash(key) & mask;
    for (unsigned p = 0; p <= mask; ++p, h = (h + 1u) & mask)
        if (atomicCAS(&table[h], kTsdfArchiveEmpty, index) == kTsdfArchiveEmpty) return true;
    return false;
}

__global__ __launch_bounds__(256) void tsdf_archive_keys_kernel(TsdfArchiveDev P) {
    const long long q0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (q0 >= P.total) return;
    const unsigned four = *reinterpret_cast<const unsigned*>(P.vmask + q0);       // vmask and vbase are padded to whole lanes; the bytes behind `total` are 0
    if (!four) return;
    const int4 b = *reinterpret_cast<const int4*>(P.vbase + q0);
    const int first[4] = {b.x, b.y, b.z, b.w};
    int x = (int)(q0 % P.size[0]), y = (int)((q0 / P.size[0]) % P.size[1]), z = (int)(q0 / ((long long)P.size[0] * P.size[1]));
    for (int e = 0; e < 4; ++e) {
        const unsigned m = (four >> (8 * e)) & 0x7Fu;
        int at = first[e];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!((m >> (d - 1)) & 1u)) continue;
            if (at >= 0 && at < P.p_nv) P.p_key[at] = make_int4(P.base[0] + P.lo[0] + x, P.base[1] + P.lo[1] + y, P.base[2] + P.lo[2] + z, d);
            ++at;
        }
        if (++x == P.size[0]) { x = 0; if (++y == P.size[1]) { y = 0; ++z; } }
    }
}

__global__ __launch_bounds__(256) void tsdf_archive_lookup_kernel(TsdfArchiveDev P) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    int is_new = 0;
    if (v < P.p_nv) {
        const int4 key = P.p_key[v];
        unsigned h = tsdf_archive_hash(key) & P.mask;
        int found = -1; bool done = false;
        for (unsigned p = 0; p <= P.mask; ++p, h = (h + 1u) & P.mask) {
            const int s = P.table[h];
            if (s == kTsdfArchiveEmpty) { done = true; break; }
            if ((unsigned)s >= (unsigned)P.nv) break;                             // not an index of this archive: the table is not sound
            if (tsdf_archive_same(P.key[s], key)) { found = s; done = true; break; }
        }
        if (!done) *P.err = 1;
        P.p_map[v] = found;
        is_new = found < 0;
    }
    const int n = __syncthreads_count(is_new);
    if (threadIdx.x == 0) P.cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(256) void tsdf_archive_insert_kernel(TsdfArchiveDev P) {
    __shared__ int ws[4];
    const int v = blockIdx.x * 256 + threadIdx.x;
    const bool is_new = v < P.p_nv && P.p_map[v] < 0;
    const unsigned long long b = __ballot(is_new);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) ws[wv] = __popcll(b);
    __syncthreads();
    if (!is_new) return;
    int rank = __popcll(b & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; ++q) rank += ws[q];
    const long long at = (long long)P.nv + P.cnt[blockIdx.x] + rank;             // the host made room for nv + p_nv vertices
    if (at >= (long long)P.nv + P.p_nv) { *P.err = 1; return; }
    const unsigned* src = reinterpret_cast<const unsigned*>(P.p_xyz) + 3 * (size_t)v;
    unsigned* dst = reinterpret_cast<unsigned*>(P.xyz) + 3 * (size_t)at;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];                            // words: a NaN position passes with its payload
    if (P.rgba) P.rgba[at] = P.p_rgba[v];
    const int4 key = P.p_key[v];
    P.key[at] = key;
    P.p_map[v] = (int)at;
    if (!tsdf_archive_insert(P.table, P.mask, key, (int)at)) *P.err = 1;
}

__global__ __launch_bounds__(256) void tsdf_archive_triangle_kernel(TsdfArchiveDev P) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;              // p_nt may be close to 2^31
    if (t >= P.p_nt) return;
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = P.p_tri[3 * (size_t)t + k];
        idx[k] = (unsigned)i < (unsigned)P.p_nv ? P.p_map[i] : -1;
        if (idx[k] < 0) *P.err = 1;
    }
    int* dst = P.tri + 3 * ((size_t)P.nt + t);
    dst[0] = idx[0]; dst[1] = idx[1]; dst[2] = idx[2];
}

__global__ __launch_bounds__(256) void tsdf_archive_rebuild_kernel(const int4* __restrict__ key, int nv, int* table, unsigned mask, int* err) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;              // nv may be 2^31 - 1
    if (v >= nv) return;
    if (!tsdf_archive_insert(table, mask, key[v], (int)v)) *err = 1;
}

int tsdf_archive_keys_launch(nalo_ctx* c, const TsdfArchiveDev& D) {
    tsdf_archive_keys_kernel<<<(D.total + kTsdfVoxPerBlock - 1) / kTsdfVoxPerBlock, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

int tsdf_archive_append_launch(nalo_ctx* c, const TsdfArchiveDev& D) {
    tsdf_archive_lookup_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    { const int rc = scan_ints_launch(c, D.cnt, D.nb); if (rc) return rc; }
    tsdf_archive_insert_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    if (D.p_nt > 0) {
        tsdf_archive_triangle_kernel<<<(unsigned)(((long long)D.p_nt + 255) / 256), 256, 0, c->stream>>>(D);
        NALO_HIP(c, hipGetLastError());
    }
    return NALO_OK;
}

int tsdf_archive_rebuild_launch(nalo_ctx* c, const int4* key, int nv, int* table, unsigned mask, int* err) {
    if (nv <= 0) return NALO_OK;
    tsdf_archive_rebuild_kernel<<<(unsigned)(((long long)nv + 255) / 256), 256, 0, c->stream>>>(key, nv, table, mask, err);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
