// The back-projection of SampleOutputWrapper::publishKeyframes (IOWrapper/OutputWrapper/SampleOutputWrapper.h:110-118), once: the PCD writer of host_io.cpp
// (nalo_io_write_pcd_points), its host form nalo_map_world_points_host and the device cloud of kernels_map.hip (nalo_map_world_points) both compile this function, so the two
// cannot drift apart. Every operation is written out in the reference's order and precision; the device side is built without FMA contraction.
#pragma once

#if defined(__HIPCC__)
#define NALO_MAP_HD __host__ __device__ inline
#else
#define NALO_MAP_HD inline
#endif

namespace nalo {

// ci = {fxi, fyi, cxi, cyi}; m = camToWorld, 3x4 row major; wp = m * (x, y, z, 1)
NALO_MAP_HD void map_world_point(float u, float v, float idepth, const float ci[4], const double m[12], double wp[3]) {
    const float fxi = ci[0], fyi = ci[1], cxi = ci[2], cyi = ci[3];
    const float depth = 1.0f / idepth;
    const float x = (u * fxi + cxi) * depth, y = (v * fyi + cyi) * depth, z = depth * (1 + 2 * fxi);       // SampleOutputWrapper.h:113-116
    const double c[4] = {x, y, z, 1.0};
    for (int r = 0; r < 3; ++r) wp[r] = ((m[4 * r] * c[0] + m[4 * r + 1] * c[1]) + m[4 * r + 2] * c[2]) + m[4 * r + 3] * c[3];
}

}  // namespace nalo
