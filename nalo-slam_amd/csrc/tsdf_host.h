// The host arithmetic of the TSDF section (include/nalo_gpu.h) that needs no device: host_tsdf.cpp, plain C++ built without FMA contraction, so that a CPU
// program can exercise it. host_tsdf.hip calls it before it enqueues anything.
#pragma once
#include "../../include/nalo_gpu.h"

namespace nalo {

// nalo_tsdf_create's refusals; NULL when the descriptor is good, else the reason (a static string)
const char* tsdf_desc_refusal(const nalo_tsdf_desc* d);
// M = worldToCam in float from camToWorld in double (R^T and -(R^T t), each row summed left to right in double); false: an entry is not finite
bool tsdf_world_to_cam(const double camToWorld[12], float M[12]);

}  // namespace nalo
