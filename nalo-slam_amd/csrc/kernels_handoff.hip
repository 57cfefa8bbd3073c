// The hand-off of a tracking reference between two contexts (nalo_trk_ref_import, host_api.hip): every level's cloud {u, v, idepth, color} and its
// idepth / weightSums maps copied from device memory in ONE launch, where 24 copy packets would each cost a launch's latency on the tracker's stream.
//   handoff_copy_kernel   a segmented copy: a table of at most kHandoffMaxSegs segments {src, dst, words} in the kernel arguments, src NULL = zero fill. A
//                         workgroup owns kHandoffChunk consecutive words of ONE segment (consecutive workgroups cover consecutive memory); a lane moves one 16-byte
//                         element where source and destination are both 16-byte aligned - a chunk starts a multiple of 16 bytes into its segment, so the segment's
//                         first addresses decide for all its chunks -, 4-byte words otherwise (a torch slice is only 4-byte aligned), and the chunk's last
//                         words % 4 words go word by word. Words are moved as 32-bit integers: NaN payloads and -0.0 pass.
// No lane touches a word outside [0, words) of its segment: every index is tested against the chunk's count, which is cut at the segment's end.
#include "nalo_internal.h"
#include "handoff_device.h"
#include <hip/hip_ext.h>

namespace nalo {

__global__ __launch_bounds__(256) void handoff_copy_kernel(HandoffTable T) {
    int s = 0;
    while (s + 1 < T.nseg && (int)blockIdx.x >= T.seg[s + 1].blk0) ++s;           // uniform: at most kHandoffMaxSegs - 1 scalar compares
    const HandoffSeg& S = T.seg[s];
    const size_t base = (size_t)((int)blockIdx.x - S.blk0) * kHandoffChunk;
    if (base >= S.words) return;
    const unsigned count = (unsigned)(S.words - base < (size_t)kHandoffChunk ? S.words - base : (size_t)kHandoffChunk);
    const uint32_t* __restrict__ src = S.src ? S.src + base : nullptr;
    uint32_t* __restrict__ dst = S.dst + base;
    const bool wide = (((uintptr_t)dst | (uintptr_t)src) & 15u) == 0;             // a NULL source (zero fill) leaves the destination to decide
    if (wide) {
        const unsigned nvec = count >> 2;
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);
        uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
        for (unsigned i = threadIdx.x; i < nvec; i += 256) d4[i] = s4 ? s4[i] : make_uint4(0u, 0u, 0u, 0u);
        const unsigned t = (nvec << 2) + threadIdx.x;                              // the tail: count % 4 words
        if (t < count) dst[t] = src ? src[t] : 0u;
    } else {
        for (unsigned i = threadIdx.x; i < count; i += 256) dst[i] = src ? src[i] : 0u;
    }
}

// fills blk0 per segment (segments of zero words are dropped) and launches behind whatever the stream holds; an empty table launches nothing
int handoff_copy_launch(nalo_ctx* c, HandoffTable& T) {
    int nseg = 0, blocks = 0;
    for (int i = 0; i < T.nseg; ++i) {
        if (!T.seg[i].words) continue;
        T.seg[nseg] = T.seg[i];
        T.seg[nseg].blk0 = blocks;
        blocks += (int)((T.seg[i].words + kHandoffChunk - 1) / kHandoffChunk);
        ++nseg;
    }
    T.nseg = nseg;
    if (!blocks) return NALO_OK;
    ProfScope ps(c, "trk_ref_import", true);                                       // dispatch-attached timestamps
    if (ps.a) hipExtLaunchKernelGGL(handoff_copy_kernel, dim3(blocks), dim3(256), 0, c->stream, ps.a, ps.b, 0, T);
    else handoff_copy_kernel<<<blocks, 256, 0, c->stream>>>(T);
    NALO_HIP(c, hipGetLastError());
    return NALO_OK;
}

}  // namespace nalo
