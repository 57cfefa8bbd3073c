// nalo_tsdf_mesh's kernels (include/nalo_gpu.h, "the mesh"): marching tetrahedra on the Kuhn split of every cell of a sub-box, as an ordered compaction in the
// surface points' scheme. A lane takes four consecutive voxels of the sub-box, so lane order is output order; counts are scanned inside a workgroup and across
// workgroups (scan_ints_launch); nothing is appended atomically, so the same bytes come out on every run. Built WITHOUT FMA contraction: a vertex is
// centre(v) + voxel_size * (t0 / (t0 - t1)), one rounding per operation, the surface points' own expression.
//   classify   per voxel the 7-bit mask of the edges it owns that carry a vertex (one byte of scratch) and its cell's triangle count; per workgroup both sums
//   scan       both count arrays
//   vertices   per voxel the index of its first vertex (an int of scratch), and the positions; nalo_tsdf_mesh_color's instantiation also the colours
//   triangles  per live cell the six tetrahedra through the table in __constant__ memory; a vertex's index is its owner's first index plus the set bits below its edge
// The two write kernels store nothing into xyz / tri when the scanned totals exceed the buffers (the host grows them and runs the two again).
// What is skipped: a voxel that is not valid owns no vertex and its cell is not live, so its seven neighbours are not read; a cell that yields a triangle has a
// corner on the other side of corner 0, so the triangle pass reads the volume only where the voxel's mask byte is not zero.
#include "nalo_internal.h"
#include "tsdf_mesh_table.h"

namespace nalo {

__constant__ TsdfMeshTable kTsdfMeshTable = tsdf_mesh_make_table();

// a lane's first voxel as sub-box coordinates, and the step to the next voxel in (k, j, i) order
struct TsdfMeshAt { int x, y, z; };
__device__ __forceinline__ TsdfMeshAt tsdf_mesh_at(const TsdfMeshDev& P, int q) {
    return {q % P.size[0], (q / P.size[0]) % P.size[1], q / (P.size[0] * P.size[1])};
}
__device__ __forceinline__ void tsdf_mesh_next(const TsdfMeshDev& P, TsdfMeshAt& a) {
    if (++a.x == P.size[0]) { a.x = 0; if (++a.y == P.size[1]) { a.y = 0; ++a.z; } }
}
// the cell of sub-box voxel a: bit b of `valid` / `inside` for corner b = dx + 2 dy + 4 dz. A corner outside the sub-box is not valid. A voxel that is not
// valid itself owns no vertex and its cell is not live: the other seven corners are not read then (most of a fused volume was never observed), valid = 0.
// Returns the voxel's linear index in the grid.
__device__ __forceinline__ size_t tsdf_mesh_cell(const TsdfMeshDev& P, const TsdfMeshAt& a, unsigned& valid, unsigned& inside) {
    const size_t at = ((size_t)(P.lo[2] + a.z) * P.ny + (P.lo[1] + a.y)) * P.nx + (P.lo[0] + a.x);
    valid = 0; inside = 0;
    {
        const float t = P.tsdf[at], w = P.weight[at];
        if (!(w >= P.min_weight && t == t)) return at;
        valid = 1u; inside = t < 0.0f ? 1u : 0u;
    }
    const bool in[3] = {a.x + 1 < P.size[0], a.y + 1 < P.size[1], a.z + 1 < P.size[2]};
#pragma unroll
    for (int b = 1; b < 8; ++b) {
        if (((b & 1) && !in[0]) || ((b & 2) && !in[1]) || ((b & 4) && !in[2])) continue;
        const size_t o = at + (b & 1) + (size_t)((b >> 1) & 1) * P.nx + (size_t)((b >> 2) & 1) * P.nx * P.ny;
        const float t = P.tsdf[o], w = P.weight[o];
        if (w >= P.min_weight && t == t) valid |= 1u << b;
        if (t < 0.0f) inside |= 1u << b;
    }
    return at;
}
// bit m - 1: edge m of the voxel carries a vertex
__device__ __forceinline__ unsigned tsdf_mesh_vertex_mask(unsigned valid, unsigned inside) {
    if (!(valid & 1u)) return 0;
    const unsigned differs = (inside & 1u) ? ~inside : inside;                    // corners on the other side of the sign than corner 0
    return ((valid & differs) >> 1) & 0x7Fu;
}
__device__ __forceinline__ int tsdf_mesh_tet_mask(unsigned inside, int t) {
    return (int)((inside & 1u) | (((inside >> kTsdfTetCorner[t][1]) & 1u) << 1) | (((inside >> kTsdfTetCorner[t][2]) & 1u) << 2) | (((inside >> 7) & 1u) << 3));
}
__device__ __forceinline__ int tsdf_mesh_triangles(unsigned valid, unsigned inside) {
    if (valid != 0xFFu || inside == 0 || inside == 0xFFu) return 0;
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) { const int k = __popc((unsigned)tsdf_mesh_tet_mask(inside, t)); n += k == 2 ? 2 : (k == 1 || k == 3) ? 1 : 0; }
    return n;
}

// exclusive prefixes of a and b over the workgroup's 256 lanes, and the workgroup's totals
__device__ __forceinline__ void tsdf_mesh_block_scan2(int a, int b, int& pa, int& pb, int& sa, int& sb) {
    __shared__ int ws[2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int ia = a, ib = b;
    for (int d = 1; d < 64; d <<= 1) {
        const int oa = __shfl_up(ia, d, 64), ob = __shfl_up(ib, d, 64);
        if (lane >= d) { ia += oa; ib += ob; }
    }
    if (lane == 63) { ws[0][wv] = ia; ws[1][wv] = ib; }
    __syncthreads();
    int fa = 0, fb = 0;
    for (int q = 0; q < wv; ++q) { fa += ws[0][q]; fb += ws[1][q]; }
    sa = (ws[0][0] + ws[0][1]) + (ws[0][2] + ws[0][3]);
    sb = (ws[1][0] + ws[1][1]) + (ws[1][2] + ws[1][3]);
    pa = fa + ia - a; pb = fb + ib - b;
}

__global__ __launch_bounds__(256) void tsdf_mesh_classify_kernel(TsdfMeshDev P) {
    const long long q0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    int nv = 0, nt = 0;
    if (q0 < P.total) {
        TsdfMeshAt a = tsdf_mesh_at(P, (int)q0);
        unsigned four = 0;
        for (int e = 0; e < 4 && q0 + e < P.total; ++e, tsdf_mesh_next(P, a)) {
            unsigned valid, inside;
            (void)tsdf_mesh_cell(P, a, valid, inside);
            const unsigned m = tsdf_mesh_vertex_mask(valid, inside);
            four |= m << (8 * e);
            nv += __popc(m); nt += tsdf_mesh_triangles(valid, inside);
        }
        *reinterpret_cast<unsigned*>(P.vmask + q0) = four;                       // vmask and vbase are padded to whole lanes
    }
    int pa, pb, sa, sb;
    tsdf_mesh_block_scan2(nv, nt, pa, pb, sa, sb);
    if (threadIdx.x == 0) { P.cntv[blockIdx.x] = sa; P.cntt[blockIdx.x] = sb; }
}

// both scanned sums fit the device mesh's buffers: xyz and tri are written together or not at all, so that a mesh too large for them leaves the previous one whole
__device__ __forceinline__ bool tsdf_mesh_fits(const TsdfMeshDev& P) {
    return (long long)P.cntv[P.nb] <= P.capv && (long long)(unsigned)P.cntt[P.nb] <= P.capt;
}

// nalo_tsdf_mesh_color: plane X of the vertex on (v, n) is X(v) + s * (X(n) - X(v)), its byte (uint8)(int)(fminf(fmaxf(cX, 0.0f), 255.0f) + 0.5f); a NaN is 0
__device__ __forceinline__ unsigned tsdf_mesh_colour_byte(float xv, float xn, float s) {
    const float cx = xv + s * (xn - xv);
    return (unsigned)(int)(fminf(fmaxf(cx, 0.0f), 255.0f) + 0.5f);
}

// kColour: the vertex pass also writes one colour per vertex, R, G, B, 255 as one aligned word
template <bool kColour>
__global__ __launch_bounds__(256) void tsdf_mesh_vertex_kernel(TsdfMeshDev P) {
    const long long q0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned m[4] = {0, 0, 0, 0};
    int n = 0;
    if (q0 < P.total) {
        const unsigned four = *reinterpret_cast<const unsigned*>(P.vmask + q0);
        for (int e = 0; e < 4; ++e) if (q0 + e < P.total) { m[e] = (four >> (8 * e)) & 0xFFu; n += __popc(m[e]); }
    }
    int pa, pb, sa, sb;
    tsdf_mesh_block_scan2(n, 0, pa, pb, sa, sb);
    if (q0 >= P.total) return;
    long long at = (long long)P.cntv[blockIdx.x] + pa;                            // below 7 * 2^28
    {
        int4 b;
        b.x = (int)at; b.y = b.x + __popc(m[0]); b.z = b.y + __popc(m[1]); b.w = b.z + __popc(m[2]);
        *reinterpret_cast<int4*>(P.vbase + q0) = b;
    }
    if (!n || !tsdf_mesh_fits(P)) return;
    TsdfMeshAt a = tsdf_mesh_at(P, (int)q0);
    for (int e = 0; e < 4; ++e, tsdf_mesh_next(P, a)) {
        if (!m[e]) continue;
        const int i = P.lo[0] + a.x, j = P.lo[1] + a.y, k = P.lo[2] + a.z;
        const size_t v = ((size_t)k * P.ny + j) * P.nx + i;
        const float c[3] = {P.origin[0] + ((float)i + 0.5f) * P.vs, P.origin[1] + ((float)j + 0.5f) * P.vs, P.origin[2] + ((float)k + 0.5f) * P.vs};
        const float t0 = P.tsdf[v];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!((m[e] >> (d - 1)) & 1u)) continue;
            const size_t nb = v + (d & 1) + (size_t)((d >> 1) & 1) * P.nx + (size_t)((d >> 2) & 1) * P.nx * P.ny;
            const float t1 = P.tsdf[nb];
            const float s = t0 / (t0 - t1);
            const float prod = P.vs * s;
            P.xyz[3 * at] = (d & 1) ? c[0] + prod : c[0];
            P.xyz[3 * at + 1] = (d & 2) ? c[1] + prod : c[1];
            P.xyz[3 * at + 2] = (d & 4) ? c[2] + prod : c[2];
            if constexpr (kColour) {
                const unsigned b = tsdf_mesh_colour_byte(P.col[v], P.col[nb], s);
                const unsigned g = tsdf_mesh_colour_byte(P.col[P.col_plane + v], P.col[P.col_plane + nb], s);
                const unsigned r = tsdf_mesh_colour_byte(P.col[2 * P.col_plane + v], P.col[2 * P.col_plane + nb], s);
                P.rgba[at] = r | (g << 8) | (b << 16) | 0xFF000000u;
            }
            ++at;
        }
    }
}

__global__ __launch_bounds__(256) void tsdf_mesh_triangle_kernel(TsdfMeshDev P) {
    const long long q0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned ins[4] = {0, 0, 0, 0};
    int nt[4] = {0, 0, 0, 0}, n = 0;
    const bool fits = tsdf_mesh_fits(P);
    if (fits && q0 < P.total) {
        // a live cell whose corners differ in sign has a corner that differs from corner 0: its voxel owns a vertex. Only those cells read the volume again.
        const unsigned four = *reinterpret_cast<const unsigned*>(P.vmask + q0);
        TsdfMeshAt a = tsdf_mesh_at(P, (int)q0);
        for (int e = 0; e < 4 && q0 + e < P.total; ++e, tsdf_mesh_next(P, a)) {
            if (!((four >> (8 * e)) & 0xFFu)) continue;
            unsigned valid;
            (void)tsdf_mesh_cell(P, a, valid, ins[e]);
            nt[e] = tsdf_mesh_triangles(valid, ins[e]);
            n += nt[e];
        }
    }
    int pa, pb, sa, sb;
    tsdf_mesh_block_scan2(n, 0, pa, pb, sa, sb);
    long long at = (long long)(unsigned)P.cntt[blockIdx.x] + pa;                  // the scan wraps as unsigned: 12 triangles a cell of 2^28 pass 2^31, not 2^32
    const int sx = P.size[0], sxy = P.size[0] * P.size[1];
    for (int e = 0; e < 4; ++e) {
        if (!nt[e]) continue;
        const long long q = q0 + e;
        int base[7]; unsigned vm[7];                                              // the owners: corners 0..6 (corner 7 owns no edge of this cell)
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            const long long o = q + (b & 1) + ((b >> 1) & 1) * sx + (long long)((b >> 2) & 1) * sxy;
            base[b] = P.vbase[o]; vm[b] = P.vmask[o];
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const signed char* row = kTsdfMeshTable.e[t][tsdf_mesh_tet_mask(ins[e], t)];
#pragma unroll
            for (int k3 = 0; k3 < 6; k3 += 3) {
                if (row[k3] < 0) break;
                int idx[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int code = row[k3 + k], p = code >> 3, mm = code & 7;
                    int bp = base[0]; unsigned mp = vm[0];
#pragma unroll
                    for (int b = 1; b < 7; ++b) if (p == b) { bp = base[b]; mp = vm[b]; }      // selects, so that base / vm stay in registers
                    idx[k] = bp + __popc(mp & ((1u << (mm - 1)) - 1u));
                }
                P.tri[3 * at] = idx[0]; P.tri[3 * at + 1] = idx[1]; P.tri[3 * at + 2] = idx[2];
                ++at;
            }
        }
    }
}

int tsdf_mesh_classify_launch(nalo_ctx* c, const TsdfMeshDev& D) {
    tsdf_mesh_classify_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    { const int rc = scan_ints_launch(c, D.cntv, D.nb); if (rc) return rc; }
    return scan_ints_launch(c, D.cntt, D.nb);
}
int tsdf_mesh_write_launch(nalo_ctx* c, const TsdfMeshDev& D) {
    if (D.col) tsdf_mesh_vertex_kernel<true><<<D.nb, 256, 0, c->stream>>>(D);
    else tsdf_mesh_vertex_kernel<false><<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    tsdf_mesh_triangle_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
