// The triangle table of nalo_tsdf_mesh (include/nalo_gpu.h, "the mesh"): marching tetrahedra on the Kuhn split of a cell. Nothing here is typed in: the table is
// BUILT from the header's rules (the lone corner / the quad, then the winding test at doubled unit-cube coordinates) by a constexpr function that the device file
// evaluates into __constant__ memory and host_tsdf.cpp hands out through nalo_tsdf_mesh_table. Plain C++17, integers only.
#pragma once

namespace nalo {

struct TsdfMeshTable { signed char e[6][16][6]; };                             // [tetrahedron][mask][up to two triangles], a vertex coded 8 p + (q ^ p), -1 padding

// the corners of T0..T5 as cell corners b = dx + 2 dy + 4 dz: every one a chain 0 ⊂ c1 ⊂ c2 ⊂ 7
constexpr int kTsdfTetCorner[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};

constexpr TsdfMeshTable tsdf_mesh_make_table() {
    TsdfMeshTable T{};
    for (int t = 0; t < 6; ++t)
        for (int mask = 0; mask < 16; ++mask) {
            for (int k = 0; k < 6; ++k) T.e[t][mask][k] = -1;
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;    // positions r, ascending
            for (int r = 0; r < 4; ++r) { if ((mask >> r) & 1) in[ni++] = r; else out[no++] = r; }
            if (ni == 0 || no == 0) continue;
            int ea[4] = {0, 0, 0, 0}, eb[4] = {0, 0, 0, 0}, nq = 0;              // the polygon's vertices as edges (r, r') of the tetrahedron
            if (ni == 1 || no == 1) {
                const int L = ni == 1 ? in[0] : out[0];
                const int* O = ni == 1 ? out : in;
                for (int k = 0; k < 3; ++k) { ea[k] = L; eb[k] = O[k]; }
                nq = 3;
            } else {
                ea[0] = in[0]; eb[0] = out[0];
                ea[1] = in[0]; eb[1] = out[1];
                ea[2] = in[1]; eb[2] = out[1];
                ea[3] = in[1]; eb[3] = out[0];
                nq = 4;
            }
            // mean of the outside corners minus mean of the inside corners, times ni no > 0
            int dir[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                int so = 0, si = 0;
                for (int k = 0; k < no; ++k) so += (kTsdfTetCorner[t][out[k]] >> a) & 1;
                for (int k = 0; k < ni; ++k) si += (kTsdfTetCorner[t][in[k]] >> a) & 1;
                dir[a] = ni * so - no * si;
            }
            for (int tri = 0; tri + 2 < nq; ++tri) {
                const int idx[3] = {0, tri + 1, tri + 2};
                int code[3] = {0, 0, 0}, pos[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
                for (int k = 0; k < 3; ++k) {
                    const int ca = kTsdfTetCorner[t][ea[idx[k]]], cb = kTsdfTetCorner[t][eb[idx[k]]];
                    const int p = ca < cb ? ca : cb, q = ca < cb ? cb : ca;     // p ⊂ q along the chain
                    code[k] = 8 * p + (q ^ p);
                    for (int a = 0; a < 3; ++a) pos[k][a] = ((p >> a) & 1) + ((q >> a) & 1);      // the edge's midpoint, doubled
                }
                int u[3] = {0, 0, 0}, v[3] = {0, 0, 0};
                for (int a = 0; a < 3; ++a) { u[a] = pos[1][a] - pos[0][a]; v[a] = pos[2][a] - pos[0][a]; }
                const int dot = (u[1] * v[2] - u[2] * v[1]) * dir[0] + (u[2] * v[0] - u[0] * v[2]) * dir[1] + (u[0] * v[1] - u[1] * v[0]) * dir[2];
                const bool keep = dot > 0;
                T.e[t][mask][3 * tri] = (signed char)code[0];
                T.e[t][mask][3 * tri + 1] = (signed char)(keep ? code[1] : code[2]);
                T.e[t][mask][3 * tri + 2] = (signed char)(keep ? code[2] : code[1]);
            }
        }
    return T;
}

}  // namespace nalo
