// The TSDF grid as the device sees it (include/nalo_gpu.h, "tsdf=1"): where a voxel lies in memory, where its centre lies in the world, and how a colour becomes
// a byte, and the ray-cast's field S(q). The header's definitions are stated here once; kernels_tsdf.hip, kernels_tsdf_replace.hip, kernels_tsdf_replace_n.hip,
// kernels_tsdf_mesh.hip, kernels_tsdf_raycast.hip and kernels_tsdf_align.hip use them, and all six are built
// WITHOUT FMA contraction (build.py: NO_CONTRACT): one rounding per operation. Nothing else belongs here.
// nalo_internal.h includes this file too, for the struct its kernel-argument structs embed, so every file of the library sees the functions below. Only the
// six files above may call them: tsdf_centre compiled with contraction would round differently from the header's definition.
#pragma once
#include <hip/hip_runtime.h>

namespace nalo {

// tsdf, weight: [nz][ny][nx], x fastest. col: NULL without colour, else [3][nz][ny][nx], planes B, G, R, col_plane floats apart. The pointers are not const:
// the integration writes through them, and what a kernel may write is said at its own argument struct (nalo_internal.h).
struct TsdfGridDev {
    float *tsdf, *weight;
    int nx, ny, nz;
    float origin[3], vs;
    float* col; size_t col_plane;
};

// the linear index of voxel (i, j, k), subscripts in the arrays' order [k][j][i]: below 2^29, but its byte offset is not. Three kernels write this sum out
// where its terms are computed on the way (tsdf_block_kernel, tsdf_mesh_cell, tsdf_rc_field): the order of their instructions is held to what it was.
__device__ __forceinline__ long long tsdf_index(const TsdfGridDev& G, int k, int j, int i) { return ((long long)k * G.ny + j) * G.nx + i; }

// px, py, pz: coordinate a of the centre of the voxel with index i along that axis
__device__ __forceinline__ float tsdf_centre(const TsdfGridDev& G, int a, int i) { return G.origin[a] + ((float)i + 0.5f) * G.vs; }

// (uint8)(int)(fminf(fmaxf(c, 0.0f), 255.0f) + 0.5f); a NaN is 0
__device__ __forceinline__ unsigned tsdf_colour_byte(float c) { return (unsigned)(int)(fminf(fmaxf(c, 0.0f), 255.0f) + 0.5f); }

// S(q) of "The ray-cast" on `vol`, for nalo_tsdf_raycast and nalo_tsdf_align_eval alike. kWeights: the field of the march and of the normal, VALID only with eight valid corners; without it the colour planes' plain index test.
// Every conversion to int sits behind the float comparisons (a NaN or an infinity fails them), and the linear index is 64-bit: 2^29 voxels of 4 B.
template <bool kWeights>
__device__ __forceinline__ bool tsdf_rc_field(const TsdfGridDev& G, float min_weight, const float* __restrict__ vol, float qx, float qy, float qz, float& S) {
    const float ix = floorf(qx), iy = floorf(qy), iz = floorf(qz);
    if (!(ix >= 0.0f && ix <= (float)(G.nx - 2) && iy >= 0.0f && iy <= (float)(G.ny - 2) && iz >= 0.0f && iz <= (float)(G.nz - 2))) return false;
    const float fx = qx - ix, fy = qy - iy, fz = qz - iz;
    const long long sy = G.nx, sz = (long long)G.nx * G.ny;
    // tsdf_index of the cell, written out: each conversion sits where the sum takes it up, and the compiler's order of this kernel's instructions follows that
    const long long at = ((long long)(int)iz * G.ny + (long long)(int)iy) * G.nx + (long long)(int)ix;   // corner (1, 1, 1) is at most voxel (nx - 1, ny - 1, nz - 1)
    if constexpr (kWeights) {
        const float* w = G.weight + at;
        const float mw = min_weight;
        const bool ok = (w[0] >= mw) & (w[1] >= mw) & (w[sy] >= mw) & (w[sy + 1] >= mw) & (w[sz] >= mw) & (w[sz + 1] >= mw) & (w[sz + sy] >= mw) & (w[sz + sy + 1] >= mw);
        if (!ok) return false;
    }
    const float* t = vol + at;
    const float t000 = t[0], t001 = t[1], t010 = t[sy], t011 = t[sy + 1], t100 = t[sz], t101 = t[sz + 1], t110 = t[sz + sy], t111 = t[sz + sy + 1];   // t_zyx
    const float a00 = t000 + fx * (t001 - t000), a10 = t010 + fx * (t011 - t010), a01 = t100 + fx * (t101 - t100), a11 = t110 + fx * (t111 - t110);   // a_yz
    const float b0 = a00 + fy * (a10 - a00), b1 = a01 + fy * (a11 - a01);
    S = b0 + fz * (b1 - b0);
    if constexpr (kWeights) return S == S;            // a NaN corner reaches S through every path (0 * NaN is NaN), and so does inf - inf
    return true;
}

}  // namespace nalo
