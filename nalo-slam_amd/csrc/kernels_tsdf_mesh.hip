// nalo_tsdf_mesh's and nalo_tsdf_surface_points' kernels (include/nalo_gpu.h, "the mesh"): marching tetrahedra on the Kuhn split of every cell of a sub-box, as
// an ordered compaction. A lane takes four consecutive voxels of the sub-box, so lane order is output order; counts are scanned inside a workgroup and across
// workgroups (scan_ints_launch); nothing is appended atomically, so the same bytes come out on every run. Built WITHOUT FMA contraction: a vertex is
// centre(v) + voxel_size * (t0 / (t0 - t1)), one rounding per operation.
//   classify   per voxel the 7-bit mask of the edges it owns that carry a vertex (one byte of scratch) and its cell's triangle count; per workgroup both sums
//   scan       both count arrays
//   vertices   per voxel the index of its first vertex (an int of scratch), and the positions; nalo_tsdf_mesh_color's instantiation also the colours
//   triangles  per live cell the six tetrahedra through the table in __constant__ memory; a vertex's index is its owner's first index plus the set bits below its edge
// The two write kernels store nothing into xyz / tri when the scanned totals exceed the buffers (the host grows them and runs the two again).
// What is skipped: a voxel that is not valid owns no vertex and its cell is not live, so its seven neighbours are not read; a cell that yields a triangle has a
// corner on the other side of corner 0, so the triangle pass reads the volume only where the voxel's mask byte is not zero.
// The surface points are the vertices on the axis edges m = 1, 2, 4, in the same order: the kAxisOnly instantiations of classify and vertices load corners
// 0, 1, 2 and 4 only, keep those three bits of the mask, and neither count triangles nor store first indices; no triangle pass follows them.
#include "nalo_internal.h"
#include "tsdf_device.h"
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
constexpr unsigned kTsdfAllCorners = 0xFFu, kTsdfAxisCorners = 0x17u;             // axis: corners 0, 1, 2, 4, the ends of edges 1, 2, 4

// the cell of sub-box voxel a: bit b of `valid` / `inside` for corner b = dx + 2 dy + 4 dz. A corner outside the sub-box is not valid. A voxel that is not
// valid itself owns no vertex and its cell is not live: the other seven corners are not read then (most of a fused volume was never observed), valid = 0.
// A corner outside kCorners is not loaded: its bits stay 0. Returns the voxel's linear index in the grid.
template <unsigned kCorners>
__device__ __forceinline__ size_t tsdf_mesh_cell(const TsdfMeshDev& P, const TsdfMeshAt& a, unsigned& valid, unsigned& inside) {
    // tsdf_index of the voxel, written out: each sum sits where the product takes it up, and the compiler's order of these kernels' instructions follows that
    const size_t at = ((size_t)(P.lo[2] + a.z) * P.g.ny + (P.lo[1] + a.y)) * P.g.nx + (P.lo[0] + a.x);
    valid = 0; inside = 0;
    {
        const float t = P.g.tsdf[at], w = P.g.weight[at];
        if (!(w >= P.min_weight && t == t)) return at;
        valid = 1u; inside = t < 0.0f ? 1u : 0u;
    }
    const bool in[3] = {a.x + 1 < P.size[0], a.y + 1 < P.size[1], a.z + 1 < P.size[2]};
#pragma unroll
    for (int b = 1; b < 8; ++b) {
        if (!((kCorners >> b) & 1u)) continue;
        if (((b & 1) && !in[0]) || ((b & 2) && !in[1]) || ((b & 4) && !in[2])) continue;
        const size_t o = at + (b & 1) + (size_t)((b >> 1) & 1) * P.g.nx + (size_t)((b >> 2) & 1) * P.g.nx * P.g.ny;
        const float t = P.g.tsdf[o], w = P.g.weight[o];
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

template <bool kAxisOnly>
__global__ __launch_bounds__(256) void tsdf_mesh_classify_kernel(TsdfMeshDev P) {
    constexpr unsigned kCorners = kAxisOnly ? kTsdfAxisCorners : kTsdfAllCorners;
    const long long q0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    int nv = 0, nt = 0;
    if (q0 < P.total) {
        TsdfMeshAt a = tsdf_mesh_at(P, (int)q0);
        unsigned four = 0;
        for (int e = 0; e < 4 && q0 + e < P.total; ++e, tsdf_mesh_next(P, a)) {
            unsigned valid, inside;
            (void)tsdf_mesh_cell<kCorners>(P, a, valid, inside);
            const unsigned m = tsdf_mesh_vertex_mask(valid, inside) & (kCorners >> 1);
            four |= m << (8 * e);
            nv += __popc(m);
            if constexpr (!kAxisOnly) nt += tsdf_mesh_triangles(valid, inside);
        }
        *reinterpret_cast<unsigned*>(P.vmask + q0) = four;                       // vmask and vbase are padded to whole lanes
    }
    int pa, pb, sa, sb;
    tsdf_mesh_block_scan2(nv, nt, pa, pb, sa, sb);
    if (threadIdx.x == 0) { P.cntv[blockIdx.x] = sa; if constexpr (!kAxisOnly) P.cntt[blockIdx.x] = sb; }
}

// the scanned sums fit the buffers: the mesh's xyz and tri are written together or not at all, so that a mesh too large for them leaves the previous one whole
template <bool kAxisOnly>
__device__ __forceinline__ bool tsdf_mesh_fits(const TsdfMeshDev& P) {
    return (long long)P.cntv[P.nb] <= P.capv && (kAxisOnly || (long long)(unsigned)P.cntt[P.nb] <= P.capt);
}

// nalo_tsdf_mesh_color: plane X of the vertex on (v, n) is the byte of X(v) + s * (X(n) - X(v))
__device__ __forceinline__ unsigned tsdf_mesh_colour_byte(float xv, float xn, float s) { return tsdf_colour_byte(xv + s * (xn - xv)); }

// kColour: the vertex pass also writes one colour per vertex, R, G, B, 255 as one aligned word
template <bool kColour, bool kAxisOnly>
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
    if constexpr (!kAxisOnly) {
        int4 b;
        b.x = (int)at; b.y = b.x + __popc(m[0]); b.z = b.y + __popc(m[1]); b.w = b.z + __popc(m[2]);
        *reinterpret_cast<int4*>(P.vbase + q0) = b;
    }
    if (!n || !tsdf_mesh_fits<kAxisOnly>(P)) return;
    TsdfMeshAt a = tsdf_mesh_at(P, (int)q0);
    for (int e = 0; e < 4; ++e, tsdf_mesh_next(P, a)) {
        if (!m[e]) continue;
        const int i = P.lo[0] + a.x, j = P.lo[1] + a.y, k = P.lo[2] + a.z;
        const size_t v = tsdf_index(P.g, k, j, i);
        const float c[3] = {tsdf_centre(P.g, 0, i), tsdf_centre(P.g, 1, j), tsdf_centre(P.g, 2, k)};
        const float t0 = P.g.tsdf[v];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (kAxisOnly && !((kTsdfAxisCorners >> d) & 1u)) continue;          // classify left the other bits 0
            if (!((m[e] >> (d - 1)) & 1u)) continue;
            const size_t nb = v + (d & 1) + (size_t)((d >> 1) & 1) * P.g.nx + (size_t)((d >> 2) & 1) * P.g.nx * P.g.ny;
            const float t1 = P.g.tsdf[nb];
            const float s = t0 / (t0 - t1);
            const float prod = P.g.vs * s;
            P.xyz[3 * at] = (d & 1) ? c[0] + prod : c[0];
            P.xyz[3 * at + 1] = (d & 2) ? c[1] + prod : c[1];
            P.xyz[3 * at + 2] = (d & 4) ? c[2] + prod : c[2];
            if constexpr (kColour) {
                const unsigned b = tsdf_mesh_colour_byte(P.g.col[v], P.g.col[nb], s);
                const unsigned g = tsdf_mesh_colour_byte(P.g.col[P.g.col_plane + v], P.g.col[P.g.col_plane + nb], s);
                const unsigned r = tsdf_mesh_colour_byte(P.g.col[2 * P.g.col_plane + v], P.g.col[2 * P.g.col_plane + nb], s);
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
    const bool fits = tsdf_mesh_fits<false>(P);
    if (fits && q0 < P.total) {
        // a live cell whose corners differ in sign has a corner that differs from corner 0: its voxel owns a vertex. Only those cells read the volume again.
        const unsigned four = *reinterpret_cast<const unsigned*>(P.vmask + q0);
        TsdfMeshAt a = tsdf_mesh_at(P, (int)q0);
        for (int e = 0; e < 4 && q0 + e < P.total; ++e, tsdf_mesh_next(P, a)) {
            if (!((four >> (8 * e)) & 0xFFu)) continue;
            unsigned valid;
            (void)tsdf_mesh_cell<kTsdfAllCorners>(P, a, valid, ins[e]);
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

int tsdf_mesh_classify_launch(nalo_ctx* c, const TsdfMeshDev& D, bool axis_only) {
    if (axis_only) tsdf_mesh_classify_kernel<true><<<D.nb, 256, 0, c->stream>>>(D);
    else tsdf_mesh_classify_kernel<false><<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    { const int rc = scan_ints_launch(c, D.cntv, D.nb); if (rc) return rc; }
    return axis_only ? NALO_OK : scan_ints_launch(c, D.cntt, D.nb);
}
int tsdf_mesh_write_launch(nalo_ctx* c, const TsdfMeshDev& D, bool axis_only) {
    if (axis_only) tsdf_mesh_vertex_kernel<false, true><<<D.nb, 256, 0, c->stream>>>(D);
    else if (D.g.col) tsdf_mesh_vertex_kernel<true, false><<<D.nb, 256, 0, c->stream>>>(D);
    else tsdf_mesh_vertex_kernel<false, false><<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    if (axis_only) return NALO_OK;
    tsdf_mesh_triangle_kernel<<<D.nb, 256, 0, c->stream>>>(D);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
