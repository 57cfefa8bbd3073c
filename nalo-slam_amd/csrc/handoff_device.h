// The segment table of handoff_copy_kernel (kernels_handoff.hip), filled by nalo_trk_ref_import (host_api.hip) and passed in the kernel arguments.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/nalo_gpu.h"

struct nalo_ctx;

namespace nalo {

constexpr int kHandoffMaxSegs = 6 * NALO_MAX_LEVELS;     // per level: u, v, idepth, color of the cloud, the idepth and weightSums maps
constexpr int kHandoffChunk = 4096;                      // words per workgroup: 256 lanes x four 16-byte elements; a multiple of 4, so a chunk keeps its segment's alignment
struct HandoffSeg { const uint32_t* src; uint32_t* dst; size_t words; int blk0, pad; };   // src NULL: zero fill; blk0: the segment's first workgroup (handoff_copy_launch)
struct HandoffTable { int nseg, pad; HandoffSeg seg[kHandoffMaxSegs]; };
int handoff_copy_launch(nalo_ctx* c, HandoffTable& T);

}  // namespace nalo
