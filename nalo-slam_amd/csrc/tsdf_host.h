// The host arithmetic of the TSDF section (include/nalo_gpu.h) that needs no device: host_tsdf.cpp, plain C++ built without FMA contraction, so that a CPU
// program can exercise it. host_tsdf.hip calls it before it enqueues anything.
#pragma once
#include "../../include/nalo_gpu.h"

namespace nalo {

// nalo_tsdf_create's refusals; NULL when the descriptor is good, else the reason (a static string)
const char* tsdf_desc_refusal(const nalo_tsdf_desc* d);
// M = worldToCam in float from camToWorld in double (R^T and -(R^T t), each row summed left to right in double); false: an entry is not finite
bool tsdf_world_to_cam(const double camToWorld[12], float M[12]);
// nalo_tsdf_shift's host half: new_base = base + shift (refused beyond 2^24 in magnitude, the sum taken in 64 bits) and origin[a] = origin0[a] +
// (float)new_base[a] * voxel_size, the product rounded, then the sum. NULL when good, else the reason (a static string); the outputs are written only when good
const char* tsdf_shift_geometry(const float origin0[3], float voxel_size, const int base[3], const int shift[3], int new_base[3], float origin[3]);
// nalo_tsdf_replace_frames' host half (the header's nalo_tsdf_replace_frames_plan): NULL when the list is good, else the reason (a static string). skip[k] = 1
// for the frames skip_unchanged leaves out, written for every k < n when good. list_len[k]: the length of frame k's dense list now (NULL: nothing is skipped)
const char* tsdf_replace_frames_plan(const nalo_tsdf_replace_frames_args* a, const nalo_tsdf_log_entry* log, int n_log, const int* list_len, unsigned char* skip);

}  // namespace nalo
