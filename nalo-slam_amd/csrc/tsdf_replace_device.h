// The per-voxel steps of "The replacement" (include/nalo_gpu.h), stated ONCE: what a removal and an add do to a voxel's tsdf, weight and colour words, and the
// flags of what fired. kernels_tsdf_replace.hip (one pair) and kernels_tsdf_replace_n.hip (the window's pairs in one launch) call them, and both are built
// WITHOUT FMA contraction (build.py: NO_CONTRACT): one rounding per operation. The predicate and d are tsdf_voxel_device.h's. Nothing else belongs here.
#pragma once
#include "tsdf_voxel_device.h"

namespace nalo {

enum : unsigned { kTsdfRemoved = 1u, kTsdfReset = 2u, kTsdfAdded = 4u };

// the removal of d at a voxel the side's predicate accepted: the flags. w0 <= 1, a NaN, a voxel never seen: the initial values ("reset")
__device__ __forceinline__ unsigned tsdf_remove_step(float& t, float& w, float d) {
    const float t0 = t, w0 = w, w1 = w0 - 1.0f;
    if (!(w1 > 0.0f)) { t = 1.0f; w = 0.0f; return kTsdfRemoved | kTsdfReset; }
    t = (t0 * w0 - d) / w1; w = w1;
    return kTsdfRemoved;
}
// the add of d: the integration's running mean
__device__ __forceinline__ unsigned tsdf_add_step(float& t, float& w, float d, float max_weight) {
    const float t0 = t, w0 = w;
    t = (t0 * w0 + d) / (w0 + 1.0f);
    w = fminf(w0 + 1.0f, max_weight);
    return kTsdfAdded;
}
// plane X of a voxel a coloured removal took, w0 the weight BEFORE the removal: X = (X0 * w0 - (float)x) / (w0 - 1.0f), or 0.0f where the voxel was reset.
// The add's is tsdf_colour (tsdf_voxel_device.h)
__device__ __forceinline__ float tsdf_remove_colour(float x0, float w0, unsigned bgr, int plane, bool reset) {
    return reset ? 0.0f : (x0 * w0 - (float)((bgr >> (8 * plane)) & 0xFFu)) / (w0 - 1.0f);
}

}  // namespace nalo
