// A float sum whose bits depend on the order of its terms, run in index order by ONE wave: s += term(0); s += term(1); ... s += term(n - 1).
// Every lane loads one term of a 64-term run (four runs are in flight), then all lanes add the 64 lanes' terms one after the other (v_readlane, a uniform
// operand): no tree, no atomic, no partial sums. Every lane ends with the sum. term(i) is evaluated by one lane, for 0 <= i < n only; n is uniform over the wave.
// Users: iw_sum_kernel (kernels_init_window.hip, initializeFromInitializer's sumID) and ground_score_kernel (kernels_plane.hip, fitPlane's mid_z).
#pragma once
#include <hip/hip_runtime.h>

namespace nalo {

__device__ __forceinline__ float wave_lane_value(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

template <class Term>
__device__ __forceinline__ float wave_ordered_sum(float s, int n, Term term) {
    const int lane = threadIdx.x & 63;
    int i = 0;
    for (; i + 256 <= n; i += 256) {                                    // four full runs: the loads of all four are issued before the first add
        const float a = term(i + lane), b = term(i + 64 + lane), c = term(i + 128 + lane), d = term(i + 192 + lane);
#pragma unroll
        for (int k = 0; k < 64; ++k) s += wave_lane_value(a, k);
#pragma unroll
        for (int k = 0; k < 64; ++k) s += wave_lane_value(b, k);
#pragma unroll
        for (int k = 0; k < 64; ++k) s += wave_lane_value(c, k);
#pragma unroll
        for (int k = 0; k < 64; ++k) s += wave_lane_value(d, k);
    }
    for (; i < n; i += 64) {                                            // the tail: only the terms that exist are added
        const float a = i + lane < n ? term(i + lane) : 0.f;
        const int m = min(64, n - i);
        for (int k = 0; k < m; ++k) s += wave_lane_value(a, k);
    }
    return s;
}

}  // namespace nalo
