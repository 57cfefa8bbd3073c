// What the two ingest passes share on the device (kernels_pyramid.hip: ingest_kernel, from host memory; kernels_ingest_dev.hip: ingest_dev_kernel / attach_kernel,
// from planes that already live on the device): the pixels per lane and the source index of cv::resize(.., INTER_NEAREST).
#pragma once
#include <hip/hip_runtime.h>

namespace nalo {

constexpr int kIngestU = 4;                   // pixels per lane of the ingest passes (kernels_pyramid.hip, Round 4)

// cv::resize(src, dst, dsize, 0, 0, INTER_NEAREST) as Undistort::undistort_mask calls it (util/Undistort.cpp:385-433): the source column (row) of destination
// column (row) x is min(floor(x * inv), nOrg - 1) with inv = 1 / ((double)n / nOrg), evaluated in double. At nOrg == n inv is 1 and the index is x itself.
__device__ __forceinline__ int resize_nearest_src(int x, double inv, int nOrg) {
    const int s = (int)floor(x * inv);
    return s < nOrg - 1 ? s : nOrg - 1;
}
inline double resize_nearest_inv(int n, int nOrg) { return 1.0 / ((double)n / nOrg); }

}  // namespace nalo
