// The TSDF grid as the device sees it (include/nalo_gpu.h, "tsdf=1"): where a voxel lies in memory, where its centre lies in the world, and how a colour becomes
// a byte. The header's definitions are stated here once; kernels_tsdf.hip, kernels_tsdf_mesh.hip and kernels_tsdf_raycast.hip use them, and all three are built
// WITHOUT FMA contraction (build.py: NO_CONTRACT): one rounding per operation. Nothing else belongs here.
// nalo_internal.h includes this file too, for the struct its kernel-argument structs embed, so every file of the library sees the functions below. Only the
// three files above may call them: tsdf_centre compiled with contraction would round differently from the header's definition.
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

}  // namespace nalo
