// The TSDF volume of a context (include/nalo_gpu.h, "tsdf=1"): its memory and scratch, the checks of every call, the stream order of an integration. The
// arithmetic lives in kernels_tsdf.hip, kernels_tsdf_replace.hip, kernels_tsdf_replace_n.hip, kernels_tsdf_mesh.hip, kernels_tsdf_raycast.hip and kernels_tsdf_align.hip (device; the grid's own definitions in tsdf_device.h) and host_tsdf.cpp (worldToCam, the culling box, the mesh's triangle table, the alignment's step).
#include <algorithm>
#include <cmath>

#include "nalo_internal.h"
#include "tsdf_host.h"

namespace nalo {

struct TsdfVolume {
    nalo_tsdf_desc d{};                              // d.origin: the CURRENT origin, origin0 + (float)base * voxel_size (tsdf_shift_geometry)
    float origin0[3] = {0, 0, 0}; int base[3] = {0, 0, 0};   // nalo_tsdf_shift: the origin of nalo_tsdf_create and the whole voxels shifted since
    size_t n = 0;
    DevBuf<float> tsdf, weight;
    DevBuf<float> tsdf2, weight2, colour2;           // nalo_tsdf_shift's spares, empty until the first non-zero shift (colour2: of a coloured volume); each shift swaps them in
    Event ev_read;                                   // behind the last kernel that read a caller's depth plane (nalo_tsdf_release)
    bool read_pending = false;
    DevBuf<unsigned long long> updated; HostBuf<unsigned long long> updated_h;
    nalo_tsdf_stats last{}; bool have_last = false, last_replace = false;   // updated: the integration's count in [0]; a replacement's written, removed, reset, added in [0..4)
    int last_n = 0;                                  // > 0: the last operation was a window replacement of last_n pairs: updated holds [4 last_n + 1], per pair removed, reset, added, written, then written_total
    // nalo_tsdf_replace_depth_n: the side tables. kTsdfSideRing slots of 2 * kTsdfReplaceMaxPairs sides each, in pinned staging and on the device; side_ev[q] lies behind
    // the copy out of staging slot q, and a call that comes round to a slot waits for it (only when kTsdfSideRing calls are still queued)
    HostBuf<TsdfSideDev> side_stage; DevBuf<TsdfSideDev> side_tab; Event side_ev[4]; bool side_used[4] = {false, false, false, false}; int side_slot = 0;
    // nalo_tsdf_replace_frames: one plane per side that needs one (and a packed colour plane each on a coloured volume); grows on demand, freed with the volume
    std::vector<DevBuf<float>> pool; std::vector<DevBuf<unsigned>> cpool;
    DevBuf<float> block;                             // nalo_tsdf_get / _set staging: one tile of z slices of the sub-block
    DevBuf<float> xyz; HostBuf<float> xyz_h;         // nalo_tsdf_surface_points: as many points as the caller had room for
    DevBuf<float> plane2; DevBuf<unsigned> cplane2;                                 // nalo_tsdf_replace_frame: the plane of the records that were fused, when the frame's list has grown since
    KeyPlane<unsigned long long, 0> key; DevBuf<float> plane;                       // nalo_tsdf_integrate_frame: w h words each; key is zero between calls
    std::vector<MapSeg> segs;                                                       // the frame's segments, host memory: they travel as kernel arguments
    // nalo_tsdf_mesh: 5 B of scratch per sub-box voxel, the two count arrays, and the device mesh itself (nalo_tsdf_mesh_view names mesh_xyz / mesh_tri).
    // nalo_tsdf_surface_points shares mesh_mask, mesh_cntv and mesh_cnt_h (tsdf_mesh_dev): every call rewrites them before it reads them
    DevBuf<unsigned char> mesh_mask; DevBuf<int> mesh_base, mesh_cntv, mesh_cntt; HostBuf<int> mesh_cnt_h;
    DevBuf<float> mesh_xyz; DevBuf<int> mesh_tri;
    long long mesh_nv = 0, mesh_nt = 0; bool have_mesh = false;
    // colour (nalo_tsdf_color_enable): [3][nz][ny][nx], planes B, G, R; no memory while colour is off. cplane: nalo_tsdf_integrate_frame's packed colour plane, w h
    // words; mesh_rgba: one word per vertex of the device mesh, as many as mesh_xyz has room for; mesh_coloured: the last mesh call wrote it
    DevBuf<float> colour; DevBuf<unsigned> cplane, mesh_rgba; bool mesh_coloured = false;
    // nalo_tsdf_raycast: the device images (nalo_tsdf_raycast_view names them), sized by the largest view so far and never shrunk; rc_normal_on / rc_rgba_on:
    // the last call wrote that image. Their pinned staging, and the three counts
    DevBuf<float> rc_depth, rc_normal; DevBuf<unsigned> rc_rgba; DevBuf<unsigned long long> rc_cnt;
    HostBuf<float> rc_depth_h, rc_normal_h; HostBuf<unsigned> rc_rgba_h; HostBuf<unsigned long long> rc_cnt_h;
    int rc_w = 0, rc_h = 0; bool have_rc = false, rc_normal_on = false, rc_rgba_on = false;    // nalo_tsdf_align_*: the workgroups' partial records, the arrival ticket (zero between launches) and the mapped words an evaluation's sums come up in
    DevBuf<double> al_partial; DevBuf<unsigned> al_ticket; HostBuf<double> al_out;
};

// The mesh archive (nalo_tsdf_archive_*): it hangs off the context, not the volume, and outlives volumes. xyz, rgba and key have room for cap_v vertices, tri for
// cap_t triangles; the table is `slots` ints, a power of two, at most half of them taken after any append. The piece's keys, its index map and the counts of new
// vertices are scratch of one append.
struct TsdfArchive {
    bool coloured = false, have_lattice = false;
    unsigned origin0[3] = {0, 0, 0}, voxel_size = 0;                             // the lattice, as words
    DevBuf<float> xyz; DevBuf<unsigned> rgba; DevBuf<int4> key; DevBuf<int> tri, table;
    long long nv = 0, nt = 0, cap_v = 0, cap_t = 0, slots = 0;
    DevBuf<int4> p_key; DevBuf<int> p_map, cnt, err; HostBuf<int> back;          // back: the count of new vertices and the flag, as they come up
    long long added_v = 0, welded_v = 0, added_t = 0;                            // the last append
};

// a caller's colour plane as the integration kernel reads it: byte strides, sc[X] the offset of the channel that feeds plane X (B, G, R)
struct TsdfColourSrc { const unsigned char* p; long long sy, sx, sc[3]; };

constexpr long long kTsdfMeshMaxVoxels = 1LL << 28;                               // seven vertices a voxel must fit an int index
constexpr long long kTsdfMeshFirstVertices = 1LL << 14, kTsdfMeshFirstTriangles = 1LL << 15;   // the device mesh's first capacity; it grows to what a call finds plus a quarter

constexpr long long kTsdfArchiveFirstVertices = 1LL << 12, kTsdfArchiveFirstTriangles = 1LL << 13, kTsdfArchiveFirstSlots = 1LL << 13;
constexpr long long kTsdfArchiveMax = 2147483647LL;                                // an index is an int

constexpr int kTsdfSideRing = 4;                                                   // TsdfVolume::side_ev
constexpr int kTsdfCounts = 4 * kTsdfReplaceMaxPairs + 1;                           // TsdfVolume::updated

constexpr size_t kTsdfTileFloats = (size_t)1 << 22;   // nalo_tsdf_get / _set: 16 MiB of staging

void tsdf_destroy(nalo_ctx* c) { delete c->tsdf; c->tsdf = nullptr; c->tsdf_log.clear(); }
void tsdf_archive_destroy(nalo_ctx* c) { delete c->tsdf_archive; c->tsdf_archive = nullptr; }

static int tsdf_need(nalo_ctx* c, const char* who) {
    if (!c) return NALO_ERR_ARG;
    if (!c->tsdf) return fail(c, NALO_ERR_STATE, std::string(who) + ": no volume (nalo_tsdf_create)");
    return NALO_OK;
}
static int tsdf_need_colour(nalo_ctx* c, const TsdfVolume& v, const std::string& who) {
    return v.colour.p ? NALO_OK : fail(c, NALO_ERR_STATE, who + ": the volume holds no colour (nalo_tsdf_color_enable)");
}

// the grid as every kernel takes it; colour: with the colour planes (tsdf_need_colour has passed)
static TsdfGridDev tsdf_grid(const TsdfVolume& v, bool colour) {
    TsdfGridDev g{};
    g.tsdf = v.tsdf.p; g.weight = v.weight.p; g.nx = v.d.dims[0]; g.ny = v.d.dims[1]; g.nz = v.d.dims[2];
    for (int a = 0; a < 3; ++a) g.origin[a] = v.d.origin[a];
    g.vs = v.d.voxel_size; g.col = colour ? v.colour.p : nullptr; g.col_plane = v.n;
    return g;
}

// the box [lo, lo + size) a call works on, the caller's (use_box) or the whole grid, and its voxels (<= 2^29: nalo_tsdf_create). `what` names it in the refusal.
// B may be NULL: the check alone, for a caller that goes on with its own lo and size
struct TsdfBox { int lo[3], size[3]; long long total; };
static int tsdf_sub_box(nalo_ctx* c, const std::string& who, const char* what, const TsdfVolume& v, bool use_box, const int lo[3], const int size[3], TsdfBox* B) {
    TsdfBox own; if (!B) B = &own;
    B->total = 1;
    for (int k = 0; k < 3; ++k) {
        B->lo[k] = use_box ? lo[k] : 0; B->size[k] = use_box ? size[k] : v.d.dims[k];
        if (B->lo[k] < 0 || B->size[k] < 1 || B->lo[k] > v.d.dims[k] - B->size[k]) return fail(c, NALO_ERR_ARG, who + ": the " + what + " is empty or leaves the grid");
        B->total *= B->size[k];
    }
    return NALO_OK;
}

// the TsdfMeshDev of a sub-box, with the scratch reserved that the mesh and the surface points share: a mask byte per voxel, the vertex counts, the pinned words
// the totals come up in. The outputs (xyz, capv, and the mesh's vbase, cntt, tri, capt, rgba) are the caller's to fill in.
static int tsdf_mesh_dev(nalo_ctx* c, TsdfVolume& v, const TsdfBox& B, float min_weight, bool coloured, TsdfMeshDev* D) {
    *D = TsdfMeshDev{};
    D->g = tsdf_grid(v, coloured);
    for (int k = 0; k < 3; ++k) { D->lo[k] = B.lo[k]; D->size[k] = B.size[k]; }
    D->total = (int)B.total; D->nb = (int)((B.total + kTsdfVoxPerBlock - 1) / kTsdfVoxPerBlock);
    D->min_weight = min_weight;
    NALO_HIP(c, v.mesh_mask.reserve((size_t)B.total + 3));                     // whole lanes of four voxels
    NALO_HIP(c, v.mesh_cntv.reserve((size_t)D->nb + 1)); NALO_HIP(c, v.mesh_cnt_h.reserve(2));
    D->vmask = v.mesh_mask.p; D->cntv = v.mesh_cntv.p;
    return NALO_OK;
}

// the checks of both integrations behind the plane's own; M and the box on success
static int tsdf_integrate_check(nalo_ctx* c, const char* who, const TsdfVolume& v, int w, int h, const float K[4], const double camToWorld[12], float min_depth, float max_depth,
                                float M[12], int lo[3], int hi[3]) {
    for (int i = 0; i < 4; ++i) if (!std::isfinite(K[i])) return fail(c, NALO_ERR_ARG, std::string(who) + ": K is not finite");
    if (!tsdf_world_to_cam(camToWorld, M)) return fail(c, NALO_ERR_ARG, std::string(who) + ": camToWorld is not finite");
    if (!std::isfinite(min_depth) || !std::isfinite(max_depth) || min_depth > max_depth) return fail(c, NALO_ERR_ARG, std::string(who) + ": min_depth / max_depth not finite, or min_depth > max_depth");
    if (nalo_tsdf_frustum_box(&v.d, w, h, K, camToWorld, max_depth, lo, hi) != NALO_OK) return fail(c, NALO_ERR_ARG, std::string(who) + ": the culling box refused the arguments");
    return NALO_OK;
}

// everything is validated: zero the count, the kernel over the box, the call's record for nalo_tsdf_last. Enqueues only.
static int tsdf_integrate_enqueue(nalo_ctx* c, TsdfVolume& v, const char* depth, long long sy, long long sx, int w, int h, const float K[4], const float M[12], float min_depth,
                                  float max_depth, const int lo[3], const int hi[3], const TsdfColourSrc* colour = nullptr) {
    NALO_HIP(c, hipMemsetAsync(v.updated.p, 0, sizeof(unsigned long long), c->stream));
    nalo_tsdf_stats st{};
    if (hi[0] > lo[0]) {
        TsdfIntegrateDev D{};
        D.g = tsdf_grid(v, colour != nullptr);
        for (int a = 0; a < 3; ++a) { D.lo[a] = st.lo[a] = lo[a]; D.hi[a] = st.hi[a] = hi[a]; }
        D.trunc = v.d.trunc; D.max_weight = v.d.max_weight;
        std::copy(M, M + 12, D.M);
        D.fx = K[0]; D.fy = K[1]; D.cx = K[2]; D.cy = K[3]; D.min_depth = min_depth; D.max_depth = max_depth;
        D.depth = depth; D.sy = sy; D.sx = sx; D.w = w; D.h = h; D.updated = v.updated.p;
        if (colour) {
            D.colour = colour->p; D.csy = colour->sy; D.csx = colour->sx;
            for (int X = 0; X < 3; ++X) D.csc[X] = colour->sc[X];
        }
        st.visited = (long long)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
        const int rc = tsdf_integrate_launch(c, D); if (rc) return rc;
    }
    v.last = st; v.have_last = true; v.last_replace = false; v.last_n = 0;
    return NALO_OK;
}

// ---- the replacement (nalo_tsdf_replace_*)
// the camera half of a side's checks, for a plane of w x h: K, the estimate, the range; M, the side's own culling box and on = 1 on success. `who` already names the side
static int tsdf_side_camera(nalo_ctx* c, const std::string& who, const TsdfVolume& v, int w, int h, const float K[4], const nalo_tsdf_align_est* est, float min_depth, float max_depth,
                            TsdfSideDev* S) {
    for (int i = 0; i < 4; ++i) if (!std::isfinite(K[i])) return fail(c, NALO_ERR_ARG, who + ": K is not finite");
    if (nalo_tsdf_est_world_to_cam(est, S->M) != NALO_OK) return fail(c, NALO_ERR_ARG, who + ": camToWorld is not finite, or s is not finite or <= 0");
    if (!std::isfinite(min_depth) || !std::isfinite(max_depth) || min_depth > max_depth) return fail(c, NALO_ERR_ARG, who + ": min_depth / max_depth not finite, or min_depth > max_depth");
    if (nalo_tsdf_frustum_box_est(&v.d, w, h, K, est, max_depth, S->lo, S->hi) != NALO_OK) return fail(c, NALO_ERR_ARG, who + ": the culling box refused the arguments");
    S->on = 1;
    S->fx = K[0]; S->fy = K[1]; S->cx = K[2]; S->cy = K[3]; S->min_depth = min_depth; S->max_depth = max_depth; S->s = (float)est->s; S->w = w; S->h = h;
    return NALO_OK;
}
// a caller's side behind its checks: the kernel's side with the side's own culling box, on = 1. `who` already names the side. Refusals as tsdf_integrate_depth's
static int tsdf_side_check(nalo_ctx* c, const std::string& who, const TsdfVolume& v, const nalo_tsdf_side* s, TsdfSideDev* S) {
    *S = TsdfSideDev{};
    const bool coloured = s->colour.ptr != nullptr;
    if (coloured) { const int rc = tsdf_need_colour(c, v, who); if (rc) return rc; }
    { const int rc = nalo_dev_plane_check(c, &s->depth); if (rc) return rc; }
    if (s->depth.dtype != NALO_DT_F32 || s->depth.channels != 1) return fail(c, NALO_ERR_ARG, who + ": the depth plane is one channel of F32");
    if (coloured) {
        { const int rc = nalo_dev_plane_check(c, &s->colour); if (rc) return rc; }
        if (s->colour.dtype != NALO_DT_U8 || s->colour.channels != 3 || s->colour.w != s->depth.w || s->colour.h != s->depth.h)
            return fail(c, NALO_ERR_ARG, who + ": the colour plane is three channels of U8 in the depth plane's size");
        S->colour = static_cast<const unsigned char*>(s->colour.ptr); S->csy = s->colour.stride_y; S->csx = s->colour.stride_x;
        for (int X = 0; X < 3; ++X) S->csc[X] = (s->colour_is_rgb ? 2 - X : X) * s->colour.stride_c;      // the planes are B, G, R
    }
    S->coloured = coloured;
    S->depth = static_cast<const char*>(s->depth.ptr); S->sy = s->depth.stride_y; S->sx = s->depth.stride_x;
    return tsdf_side_camera(c, who, v, s->depth.w, s->depth.h, s->K, &s->est, s->min_depth, s->max_depth, S);
}
static void tsdf_side_settle(TsdfSideDev& S) { for (int a = 0; a < 3; ++a) if (S.lo[a] >= S.hi[a]) S.on = 0; }   // an empty box: the side touches nothing

// everything is validated; box (NULL: none) cuts the remove side. Zero the counts, the kernel over the hull, the call's record for nalo_tsdf_last /
// nalo_tsdf_replace_last. Enqueues only.
static int tsdf_replace_enqueue(nalo_ctx* c, TsdfVolume& v, TsdfSideDev rem, TsdfSideDev add, const TsdfBox* box) {
    if (rem.on && box) for (int a = 0; a < 3; ++a) { rem.lo[a] = std::max(rem.lo[a], box->lo[a]); rem.hi[a] = std::min(rem.hi[a], box->lo[a] + box->size[a]); }
    tsdf_side_settle(rem); tsdf_side_settle(add);
    NALO_HIP(c, hipMemsetAsync(v.updated.p, 0, 4 * sizeof(unsigned long long), c->stream));
    nalo_tsdf_stats st{};
    if (rem.on || add.on) {
        TsdfReplaceDev D{};
        D.g = tsdf_grid(v, rem.coloured || add.coloured);
        for (int a = 0; a < 3; ++a) {
            D.lo[a] = st.lo[a] = !add.on ? rem.lo[a] : !rem.on ? add.lo[a] : std::min(rem.lo[a], add.lo[a]);
            D.hi[a] = st.hi[a] = !add.on ? rem.hi[a] : !rem.on ? add.hi[a] : std::max(rem.hi[a], add.hi[a]);
        }
        D.trunc = v.d.trunc; D.max_weight = v.d.max_weight; D.rem = rem; D.add = add; D.counts = v.updated.p;
        st.visited = (long long)(D.hi[0] - D.lo[0]) * (D.hi[1] - D.lo[1]) * (D.hi[2] - D.lo[2]);
        const int rc = tsdf_replace_launch(c, D); if (rc) return rc;
    }
    v.last = st; v.have_last = true; v.last_replace = true; v.last_n = 0;
    return NALO_OK;
}

// the window replacement: sides[2k] / sides[2k + 1] are pair k's remove / add side (on = 0: absent), validated, the remove sides already cut by their boxes.
// Zero the 4 n + 1 counts, the table through a staging slot, ONE kernel over the hull, the call's record. Enqueues only (but see TsdfVolume::side_ev).
static int tsdf_replace_n_enqueue(nalo_ctx* c, TsdfVolume& v, std::vector<TsdfSideDev>& sides) {
    const int n = (int)sides.size() / 2;
    bool any = false, coloured = false;
    nalo_tsdf_stats st{};
    for (TsdfSideDev& S : sides) {
        tsdf_side_settle(S);
        if (!S.on) continue;
        for (int a = 0; a < 3; ++a) { st.lo[a] = any ? std::min(st.lo[a], S.lo[a]) : S.lo[a]; st.hi[a] = any ? std::max(st.hi[a], S.hi[a]) : S.hi[a]; }
        any = true; coloured = coloured || S.coloured;
    }
    if (any) {
        // everything that can refuse comes before the first thing that is queued
        NALO_HIP(c, v.side_stage.reserve((size_t)kTsdfSideRing * 2 * kTsdfReplaceMaxPairs));
        NALO_HIP(c, v.side_tab.reserve((size_t)kTsdfSideRing * 2 * kTsdfReplaceMaxPairs));
        for (Event& e : v.side_ev) NALO_HIP(c, e.create(hipEventDisableTiming));
    }
    NALO_HIP(c, hipMemsetAsync(v.updated.p, 0, (size_t)(4 * n + 1) * sizeof(unsigned long long), c->stream));
    if (any) {
        const int q = v.side_slot;
        const size_t at = (size_t)q * 2 * kTsdfReplaceMaxPairs;
        if (v.side_used[q]) NALO_HIP(c, hipEventSynchronize(v.side_ev[q]));    // the copy of kTsdfSideRing calls ago: long done unless that many calls are still queued
        std::copy(sides.begin(), sides.end(), v.side_stage.p + at);
        NALO_HIP(c, hipMemcpyAsync(v.side_tab.p + at, v.side_stage.p + at, sides.size() * sizeof(TsdfSideDev), hipMemcpyHostToDevice, c->stream));
        NALO_HIP(c, hipEventRecord(v.side_ev[q], c->stream));
        v.side_used[q] = true; v.side_slot = (q + 1) % kTsdfSideRing;
        TsdfReplaceNDev D{};
        D.g = tsdf_grid(v, coloured);
        for (int a = 0; a < 3; ++a) { D.lo[a] = st.lo[a]; D.hi[a] = st.hi[a]; }
        D.trunc = v.d.trunc; D.max_weight = v.d.max_weight; D.n = n; D.sides = v.side_tab.p + at; D.counts = v.updated.p;
        st.visited = (long long)(D.hi[0] - D.lo[0]) * (D.hi[1] - D.lo[1]) * (D.hi[2] - D.lo[2]);
        const int rc = tsdf_replace_n_launch(c, D); if (rc) return rc;
    }
    v.last = st; v.have_last = true; v.last_replace = true; v.last_n = n;
    return NALO_OK;
}

// ---- the fusion log (nalo_tsdf_log_*): c->tsdf_log, host memory
static nalo_tsdf_log_entry* tsdf_log_find(nalo_ctx* c, int frame_id) {
    for (nalo_tsdf_log_entry& e : c->tsdf_log) if (e.frame_id == frame_id) return &e;
    return nullptr;
}
// the frame's entry, new or rewritten in place: what it was fused with just now (with colour iff the volume holds colour now), resident in the whole grid
static void tsdf_log_put(nalo_ctx* c, const TsdfVolume& v, int frame_id, int n_records, const nalo_tsdf_align_est& est, const float K[4], float min_depth, float max_depth) {
    nalo_tsdf_log_entry* e = tsdf_log_find(c, frame_id);
    if (!e) { c->tsdf_log.push_back(nalo_tsdf_log_entry{}); e = &c->tsdf_log.back(); }
    e->frame_id = frame_id; e->n_records = n_records; e->coloured = v.colour.p ? 1 : 0; e->est = est; std::copy(K, K + 4, e->K); e->min_depth = min_depth; e->max_depth = max_depth;
    for (int a = 0; a < 3; ++a) { e->lo[a] = 0; e->size[a] = v.d.dims[a]; }
}
// behind a non-zero shift: every resident box moves with its voxels, and an entry whose voxels have all left goes
static void tsdf_log_shift(nalo_ctx* c, const TsdfVolume& v, const int shift[3]) {
    std::vector<nalo_tsdf_log_entry> kept;
    for (nalo_tsdf_log_entry e : c->tsdf_log) { nalo_tsdf_box_shift(v.d.dims, shift, e.lo, e.size); if (e.size[0] > 0) kept.push_back(e); }
    c->tsdf_log.swap(kept);
}

// the counts of the last window replacement: one copy, one wait. total: the hull, written = written_total, removed / reset / added summed over the pairs;
// per_pair (may be NULL): min(last_n, cap) rows
static int tsdf_replace_last_n(nalo_ctx* c, TsdfVolume& v, nalo_tsdf_replace_stats* total, nalo_tsdf_replace_pair_stats* per_pair, int cap) {
    const int n = v.last_n;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipMemcpyAsync(v.updated_h.p, v.updated.p, (size_t)(4 * n + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) { total->lo[k] = v.last.lo[k]; total->hi[k] = v.last.hi[k]; }
    total->visited = v.last.visited; total->removed = total->reset = total->added = 0;
    total->written = (long long)v.updated_h.p[4 * n];
    for (int k = 0; k < n; ++k) {
        const unsigned long long* q = v.updated_h.p + 4 * k;
        total->removed += (long long)q[0]; total->reset += (long long)q[1]; total->added += (long long)q[2];
        if (k < cap) per_pair[k] = nalo_tsdf_replace_pair_stats{(long long)q[0], (long long)q[1], (long long)q[2], (long long)q[3]};
    }
    return NALO_OK;
}

}  // namespace nalo

using namespace nalo;

int nalo_tsdf_create(nalo_ctx* c, const nalo_tsdf_desc* desc) {
    if (!c) return NALO_ERR_ARG;
    if (const char* why = tsdf_desc_refusal(desc)) return fail(c, NALO_ERR_ARG, std::string("nalo_tsdf_create: ") + why);
    NALO_HIP(c, hipSetDevice(c->device));
    // the new volume is complete before the old one goes: a failed allocation leaves the context as it was
    TsdfVolume* v = new TsdfVolume();
    v->d = *desc; v->n = (size_t)desc->dims[0] * desc->dims[1] * desc->dims[2];
    std::copy(desc->origin, desc->origin + 3, v->origin0);
    hipError_t e = v->tsdf.reserve(v->n);
    if (e == hipSuccess) e = v->weight.reserve(v->n);
    if (e == hipSuccess) e = v->updated.reserve(kTsdfCounts);
    if (e == hipSuccess) e = v->updated_h.reserve(kTsdfCounts);
    if (e == hipSuccess) e = v->ev_read.create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->ev_prod.create(hipEventDisableTiming);
    if (e != hipSuccess) { delete v; (void)hipGetLastError(); return fail(c, NALO_ERR_HIP, std::string("nalo_tsdf_create: ") + hipGetErrorString(e)); }
    if (c->tsdf) { NALO_HIP(c, hipStreamSynchronize(c->stream)); tsdf_destroy(c); }      // kernels of the old volume may still be queued
    c->tsdf = v;
    c->tsdf_log.clear();
    return tsdf_fill_launch(c, v->tsdf.p, v->weight.p, v->n);
}

int nalo_tsdf_reset(nalo_ctx* c) {
    { const int rc = tsdf_need(c, "nalo_tsdf_reset"); if (rc) return rc; }
    NALO_HIP(c, hipSetDevice(c->device));
    c->tsdf->have_last = false;
    c->tsdf_log.clear();
    if (c->tsdf->colour.p) NALO_HIP(c, hipMemsetAsync(c->tsdf->colour.p, 0, 3 * c->tsdf->n * sizeof(float), c->stream));      // 0.0f is all bits zero
    return tsdf_fill_launch(c, c->tsdf->tsdf.p, c->tsdf->weight.p, c->tsdf->n);
}

int nalo_tsdf_color_enable(nalo_ctx* c) {
    { const int rc = tsdf_need(c, "nalo_tsdf_color_enable"); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    if (v.colour.p) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    DevBuf<float> col;
    const hipError_t e = col.reserve(3 * v.n);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, NALO_ERR_HIP, std::string("nalo_tsdf_color_enable: ") + hipGetErrorString(e)); }
    NALO_HIP(c, hipMemsetAsync(col.p, 0, 3 * v.n * sizeof(float), c->stream));
    v.colour = std::move(col);
    return NALO_OK;
}

int nalo_tsdf_color_disable(nalo_ctx* c) {
    { const int rc = tsdf_need(c, "nalo_tsdf_color_disable"); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    if (!v.colour.p) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamSynchronize(c->stream));                              // kernels that name the planes may still be queued
    v.colour.release(); v.colour2.release(); v.cplane.release(); v.cplane2.release(); v.mesh_rgba.release(); v.mesh_coloured = false;
    for (nalo_tsdf_log_entry& e : c->tsdf_log) e.coloured = 0;                 // the colour words the logged frames were fused into are gone
    return NALO_OK;
}

int nalo_tsdf_shift(nalo_ctx* c, const int shift[3]) {
    const char* who = "nalo_tsdf_shift";
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!shift) return fail(c, NALO_ERR_ARG, "nalo_tsdf_shift: bad argument");
    TsdfVolume& v = *c->tsdf;
    int base[3]; float origin[3];
    if (const char* why = tsdf_shift_geometry(v.origin0, v.d.voxel_size, v.base, shift, base, origin)) return fail(c, NALO_ERR_ARG, std::string("nalo_tsdf_shift: ") + why);
    if (!shift[0] && !shift[1] && !shift[2]) return NALO_OK;
    // ---- accepted: from here on only the runtime can fail
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "tsdf_shift");
    const bool coloured = v.colour.p != nullptr;
    if (!v.tsdf2.p || (coloured && !v.colour2.p)) {                            // the first shift (of a coloured volume): whatever is missing, all of it or none
        DevBuf<float> t2, w2, c2;
        hipError_t e = hipSuccess;
        if (!v.tsdf2.p) { e = t2.reserve(v.n); if (e == hipSuccess) e = w2.reserve(v.n); }
        if (e == hipSuccess && coloured && !v.colour2.p) e = c2.reserve(3 * v.n);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, NALO_ERR_HIP, std::string("nalo_tsdf_shift: ") + hipGetErrorString(e)); }
        if (t2.p) { v.tsdf2 = std::move(t2); v.weight2 = std::move(w2); }
        if (c2.p) v.colour2 = std::move(c2);
    }
    TsdfShiftDev D{};
    D.src_tsdf = reinterpret_cast<const unsigned*>(v.tsdf.p); D.src_weight = reinterpret_cast<const unsigned*>(v.weight.p);
    D.dst_tsdf = reinterpret_cast<unsigned*>(v.tsdf2.p); D.dst_weight = reinterpret_cast<unsigned*>(v.weight2.p);
    if (coloured) { D.src_col = reinterpret_cast<const unsigned*>(v.colour.p); D.dst_col = reinterpret_cast<unsigned*>(v.colour2.p); }
    D.nx = v.d.dims[0]; D.ny = v.d.dims[1]; D.nz = v.d.dims[2]; D.n = (long long)v.n;
    for (int a = 0; a < 3; ++a) D.s[a] = std::max(-v.d.dims[a], std::min(v.d.dims[a], shift[a]));      // beyond the grid's extent nothing is kept either way
    { const int rc = tsdf_shift_launch(c, D); if (rc) return rc; }
    // the kernel is queued: everything behind it on the main stream reads the arrays it writes
    std::swap(v.tsdf, v.tsdf2); std::swap(v.weight, v.weight2);
    if (coloured) std::swap(v.colour, v.colour2);
    for (int a = 0; a < 3; ++a) { v.base[a] = base[a]; v.d.origin[a] = origin[a]; }
    v.have_last = false;                                                       // the last integration's box was in the old indices
    if (c->tsdf_log_on) tsdf_log_shift(c, v, shift);
    return NALO_OK;
}

int nalo_tsdf_geometry(nalo_ctx* c, struct nalo_tsdf_geometry* out) {
    { const int rc = tsdf_need(c, "nalo_tsdf_geometry"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_geometry: bad argument");
    const TsdfVolume& v = *c->tsdf;
    out->desc = v.d;
    for (int a = 0; a < 3; ++a) { out->origin0[a] = v.origin0[a]; out->base[a] = v.base[a]; }
    return NALO_OK;
}

int nalo_tsdf_destroy(nalo_ctx* c) {
    if (!c) return NALO_ERR_ARG;
    if (!c->tsdf) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    tsdf_destroy(c);
    return NALO_OK;
}

// nalo_tsdf_integrate_depth (coloured = false; colour is not looked at) and nalo_tsdf_integrate_depth_color
static int tsdf_integrate_depth(nalo_ctx* c, const char* who, const nalo_tsdf_integrate_args* a, bool coloured, const nalo_dev_plane* colour, int colour_is_rgb) {
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!a) return fail(c, NALO_ERR_ARG, std::string(who) + ": bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfVolume& v = *c->tsdf;
    if (coloured) { const int rc = tsdf_need_colour(c, v, who); if (rc) return rc; }
    if (coloured && !colour) return fail(c, NALO_ERR_ARG, std::string(who) + ": no colour plane");
    { const int rc = nalo_dev_plane_check(c, &a->depth); if (rc) return rc; }
    if (a->depth.dtype != NALO_DT_F32 || a->depth.channels != 1) return fail(c, NALO_ERR_ARG, std::string(who) + ": the depth plane is one channel of F32");
    TsdfColourSrc src{};
    if (coloured) {
        { const int rc = nalo_dev_plane_check(c, colour); if (rc) return rc; }
        if (colour->dtype != NALO_DT_U8 || colour->channels != 3 || colour->w != a->depth.w || colour->h != a->depth.h)
            return fail(c, NALO_ERR_ARG, std::string(who) + ": the colour plane is three channels of U8 in the depth plane's size");
        src.p = static_cast<const unsigned char*>(colour->ptr); src.sy = colour->stride_y; src.sx = colour->stride_x;
        for (int X = 0; X < 3; ++X) src.sc[X] = (colour_is_rgb ? 2 - X : X) * colour->stride_c;      // the planes are B, G, R
    }
    float M[12]; int lo[3], hi[3];
    { const int rc = tsdf_integrate_check(c, who, v, a->depth.w, a->depth.h, a->K, a->camToWorld, a->min_depth, a->max_depth, M, lo, hi); if (rc) return rc; }
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "tsdf_integrate_depth");
    hipStream_t prod = (hipStream_t)a->producer_stream;                      // NULL: the null stream, which the context's non-blocking stream does not wait for by itself
    if (prod != (hipStream_t)c->stream) { NALO_HIP(c, hipEventRecord(c->ev_prod, prod)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0)); }
    { const int rc = tsdf_integrate_enqueue(c, v, static_cast<const char*>(a->depth.ptr), a->depth.stride_y, a->depth.stride_x, a->depth.w, a->depth.h, a->K, M, a->min_depth,
                                            a->max_depth, lo, hi, coloured ? &src : nullptr); if (rc) return rc; }
    NALO_HIP(c, hipEventRecord(v.ev_read, c->stream));                         // the caller's planes have been read (one kernel reads both): nalo_tsdf_release
    v.read_pending = true;
    return NALO_OK;
}
int nalo_tsdf_integrate_depth(nalo_ctx* c, const nalo_tsdf_integrate_args* a) { return tsdf_integrate_depth(c, "nalo_tsdf_integrate_depth", a, false, nullptr, 0); }
int nalo_tsdf_integrate_depth_color(nalo_ctx* c, const nalo_tsdf_integrate_args* a, const nalo_dev_plane* colour, int colour_is_rgb) {
    return tsdf_integrate_depth(c, "nalo_tsdf_integrate_depth_color", a, true, colour, colour_is_rgb);
}

int nalo_tsdf_release(nalo_ctx* c, void* stream) {
    { const int rc = tsdf_need(c, "nalo_tsdf_release"); if (rc) return rc; }
    if (!c->tsdf->read_pending) return NALO_OK;                                // no plane of a caller's was ever read: nothing to wait for
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamWaitEvent((hipStream_t)stream, c->tsdf->ev_read, 0));
    return NALO_OK;
}

// the plane of the segments in `segs` (a frame's, or a prefix of them) into plane / cplane. Enqueues only.
static int tsdf_frame_plane_of(nalo_ctx* c, TsdfVolume& v, const std::vector<MapSeg>& segs, bool colour, DevBuf<float>& plane, DevBuf<unsigned>& cplane) {
    const size_t npx = (size_t)c->w * c->h;
    NALO_HIP(c, plane.reserve(npx));
    if (colour) NALO_HIP(c, cplane.reserve(npx));                              // every call writes every word of it: a winner's colour, or zero behind the resolve
    NALO_HIP(c, v.key.begin(npx, c->stream));
    { const int rc = tsdf_frame_plane_launch(c, segs.data(), (int)segs.size(), v.key.p, plane.p, colour ? cplane.p : nullptr, c->w, c->h); if (rc) return rc; }
    v.key.settled();
    return NALO_OK;
}
// the context-owned plane of a frame's dense list (the header's last-record rule) for nalo_tsdf_integrate_frame and nalo_tsdf_align_frame: v.plane, and
// v.cplane on a coloured volume when `colour` is asked for. Its refusals are map_dense_segments'. Enqueues only.
// total (may be NULL): the length of the frame's list.
static int tsdf_frame_plane(nalo_ctx* c, const char* who, TsdfVolume& v, int frame_id, bool colour, int* total_out = nullptr) {
    NALO_HIP(c, hipSetDevice(c->device));
    int total = 0;
    { const int rc = map_dense_segments(c, who, frame_id, &v.segs, &total); if (rc) return rc; }
    if (total_out) *total_out = total;
    return tsdf_frame_plane_of(c, v, v.segs, colour, v.plane, v.cplane);
}

int nalo_tsdf_integrate_frame(nalo_ctx* c, int frame_id, const double camToWorld[12], const float K[4], float min_depth, float max_depth) {
    const char* who = "nalo_tsdf_integrate_frame";
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!camToWorld || !K) return fail(c, NALO_ERR_ARG, "nalo_tsdf_integrate_frame: bad argument");
    if (!map_dense_on(c)) return fail(c, NALO_ERR_STATE, "nalo_tsdf_integrate_frame: the dense archive is not enabled (nalo_map_dense_enable)");
    TsdfVolume& v = *c->tsdf;
    float M[12]; int lo[3], hi[3];
    { const int rc = tsdf_integrate_check(c, who, v, c->w, c->h, K, camToWorld, min_depth, max_depth, M, lo, hi); if (rc) return rc; }
    if (c->tsdf_log_on && tsdf_log_find(c, frame_id)) return fail(c, NALO_ERR_STATE, "nalo_tsdf_integrate_frame: the fusion log holds this frame (nalo_tsdf_replace_frame)");
    const bool coloured = v.colour.p != nullptr;
    HostTimer ht(c, "tsdf_integrate_frame");
    int total = 0;
    { const int rc = tsdf_frame_plane(c, who, v, frame_id, coloured, &total); if (rc) return rc; }
    // the packed plane is a U8 plane of three channels, B first: stride_x 4, stride_c 1
    const TsdfColourSrc src = {reinterpret_cast<const unsigned char*>(v.cplane.p), (long long)c->w * 4, 4, {0, 1, 2}};
    { const int rc = tsdf_integrate_enqueue(c, v, reinterpret_cast<const char*>(v.plane.p), (long long)c->w * 4, 4, c->w, c->h, K, M, min_depth, max_depth, lo, hi, coloured ? &src : nullptr); if (rc) return rc; }
    if (c->tsdf_log_on) {
        nalo_tsdf_align_est est{}; std::copy(camToWorld, camToWorld + 12, est.camToWorld); est.s = 1.0;
        tsdf_log_put(c, v, frame_id, total, est, K, min_depth, max_depth);
    }
    return NALO_OK;
}

int nalo_tsdf_log_enable(nalo_ctx* c, int on) {
    if (!c) return NALO_ERR_ARG;
    c->tsdf_log_on = on != 0;
    if (!on) c->tsdf_log.clear();
    return NALO_OK;
}

int nalo_tsdf_log_get(nalo_ctx* c, nalo_tsdf_log_entry* out, int cap, int* n) {
    if (!c) return NALO_ERR_ARG;
    if (!n || cap < 0 || (cap > 0 && !out)) return fail(c, NALO_ERR_ARG, "nalo_tsdf_log_get: bad argument");
    *n = (int)c->tsdf_log.size();
    std::copy(c->tsdf_log.begin(), c->tsdf_log.begin() + std::min(*n, cap), out);
    return NALO_OK;
}

int nalo_tsdf_replace_frame(nalo_ctx* c, int frame_id, const nalo_tsdf_align_est* est_new, const float K[4], float min_depth, float max_depth) {
    const char* who = "nalo_tsdf_replace_frame";
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!c->tsdf_log_on) return fail(c, NALO_ERR_STATE, "nalo_tsdf_replace_frame: the fusion log is not enabled (nalo_tsdf_log_enable)");
    if (!map_dense_on(c)) return fail(c, NALO_ERR_STATE, "nalo_tsdf_replace_frame: the dense archive is not enabled (nalo_map_dense_enable)");
    if (est_new && !K) return fail(c, NALO_ERR_ARG, "nalo_tsdf_replace_frame: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfVolume& v = *c->tsdf;
    int total = 0;
    { const int rc = map_dense_segments(c, who, frame_id, &v.segs, &total); if (rc) return rc; }       // a sharded window, a frame the archive has never seen
    const nalo_tsdf_log_entry* e = tsdf_log_find(c, frame_id);
    if (!e && !est_new) return fail(c, NALO_ERR_ARG, "nalo_tsdf_replace_frame: nothing to remove (the log has no entry of this frame) and nothing to add");
    if (e && total < e->n_records) return fail(c, NALO_ERR_STATE, "nalo_tsdf_replace_frame: the frame's dense list is shorter than when it was fused");
    // the add side moves colour iff the volume holds colour now; the remove side iff the frame's fusion moved colour (the entry says so) into planes that still exist (so col_rem implies col_add)
    const bool col_add = v.colour.p != nullptr, col_rem = e && e->coloured && v.colour.p != nullptr;
    TsdfSideDev rem{}, add{};
    if (e) { const int rc = tsdf_side_camera(c, std::string(who) + ", the logged side", v, c->w, c->h, e->K, &e->est, e->min_depth, e->max_depth, &rem); if (rc) return rc; }
    if (est_new) { const int rc = tsdf_side_camera(c, who, v, c->w, c->h, K, est_new, min_depth, max_depth, &add); if (rc) return rc; }
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "tsdf_replace_frame");
    // the whole list's plane serves both sides unless the list has grown since the frame was fused: then the first n_records records get a plane of their own
    const bool own = e && est_new && total > e->n_records;
    if (e && (own || !est_new)) {
        std::vector<MapSeg> head;
        for (const MapSeg& sg : v.segs) if (sg.start < e->n_records) { head.push_back(sg); head.back().n = std::min(sg.n, e->n_records - sg.start); }
        { const int rc = tsdf_frame_plane_of(c, v, head, col_rem, own ? v.plane2 : v.plane, own ? v.cplane2 : v.cplane); if (rc) return rc; }
    }
    if (est_new) { const int rc = tsdf_frame_plane_of(c, v, v.segs, col_add, v.plane, v.cplane); if (rc) return rc; }
    // a packed colour plane is a U8 plane of three channels, B first: stride_x 4, stride_c 1
    for (TsdfSideDev* S : {&rem, &add}) {
        if (!S->on) continue;
        const bool second = S == &rem && own;
        S->depth = reinterpret_cast<const char*>(second ? v.plane2.p : v.plane.p); S->sy = (long long)c->w * 4; S->sx = 4;
        const bool coloured = S == &rem ? col_rem : col_add;
        S->coloured = coloured;
        if (coloured) { S->colour = reinterpret_cast<const unsigned char*>(second ? v.cplane2.p : v.cplane.p); S->csy = (long long)c->w * 4; S->csx = 4; S->csc[0] = 0; S->csc[1] = 1; S->csc[2] = 2; }
    }
    TsdfBox B{};
    if (e) for (int a = 0; a < 3; ++a) { B.lo[a] = e->lo[a]; B.size[a] = e->size[a]; }
    { const int rc = tsdf_replace_enqueue(c, v, rem, add, e ? &B : nullptr); if (rc) return rc; }
    if (est_new) tsdf_log_put(c, v, frame_id, total, *est_new, K, min_depth, max_depth);
    else c->tsdf_log.erase(c->tsdf_log.begin() + (e - c->tsdf_log.data()));
    return NALO_OK;
}

int nalo_tsdf_last(nalo_ctx* c, nalo_tsdf_stats* stats) {
    { const int rc = tsdf_need(c, "nalo_tsdf_last"); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    if (!stats) return fail(c, NALO_ERR_ARG, "nalo_tsdf_last: bad argument");
    if (!v.have_last) return fail(c, NALO_ERR_STATE, "nalo_tsdf_last: nothing has been integrated into this volume");
    NALO_HIP(c, hipSetDevice(c->device));
    // behind a window replacement the voxels written, each counted once, lie behind the pairs' counts
    NALO_HIP(c, hipMemcpyAsync(v.updated_h.p, v.updated.p + 4 * v.last_n, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    *stats = v.last;
    stats->updated = (long long)v.updated_h.p[0];
    return NALO_OK;
}

int nalo_tsdf_replace_depth(nalo_ctx* c, const nalo_tsdf_replace_args* a) {
    const std::string who = "nalo_tsdf_replace_depth";
    { const int rc = tsdf_need(c, who.c_str()); if (rc) return rc; }
    if (!a || (!a->remove && !a->add)) return fail(c, NALO_ERR_ARG, who + ": bad argument (a side, remove or add, is needed)");
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfVolume& v = *c->tsdf;
    TsdfSideDev rem{}, add{};
    if (a->remove) { const int rc = tsdf_side_check(c, who + ", remove", v, a->remove, &rem); if (rc) return rc; }
    if (a->add) { const int rc = tsdf_side_check(c, who + ", add", v, a->add, &add); if (rc) return rc; }
    TsdfBox B;
    if (a->use_box) { const int rc = tsdf_sub_box(c, who, "box", v, true, a->lo, a->size, &B); if (rc) return rc; }
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "tsdf_replace_depth");
    hipStream_t prod = (hipStream_t)a->producer_stream;                      // NULL: the null stream, which the context's non-blocking stream does not wait for by itself
    if (prod != (hipStream_t)c->stream) { NALO_HIP(c, hipEventRecord(c->ev_prod, prod)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0)); }
    { const int rc = tsdf_replace_enqueue(c, v, rem, add, a->use_box ? &B : nullptr); if (rc) return rc; }
    NALO_HIP(c, hipEventRecord(v.ev_read, c->stream));                         // the callers' planes have been read (one kernel reads all of them): nalo_tsdf_release
    v.read_pending = true;
    return NALO_OK;
}

int nalo_tsdf_replace_last(nalo_ctx* c, nalo_tsdf_replace_stats* stats) {
    { const int rc = tsdf_need(c, "nalo_tsdf_replace_last"); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    if (!stats) return fail(c, NALO_ERR_ARG, "nalo_tsdf_replace_last: bad argument");
    if (!v.have_last || !v.last_replace) return fail(c, NALO_ERR_STATE, "nalo_tsdf_replace_last: the last operation on this volume was not a replacement");
    NALO_HIP(c, hipSetDevice(c->device));
    if (v.last_n) return tsdf_replace_last_n(c, v, stats, nullptr, 0);
    NALO_HIP(c, hipMemcpyAsync(v.updated_h.p, v.updated.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) { stats->lo[k] = v.last.lo[k]; stats->hi[k] = v.last.hi[k]; }
    stats->visited = v.last.visited;
    stats->written = (long long)v.updated_h.p[0]; stats->removed = (long long)v.updated_h.p[1]; stats->reset = (long long)v.updated_h.p[2]; stats->added = (long long)v.updated_h.p[3];
    return NALO_OK;
}

int nalo_tsdf_replace_last_n(nalo_ctx* c, nalo_tsdf_replace_stats* total, nalo_tsdf_replace_pair_stats* per_pair, int cap, int* n) {
    { const int rc = tsdf_need(c, "nalo_tsdf_replace_last_n"); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    if (!n || cap < 0 || (cap > 0 && !per_pair)) return fail(c, NALO_ERR_ARG, "nalo_tsdf_replace_last_n: bad argument");
    if (!v.have_last || !v.last_replace || !v.last_n) return fail(c, NALO_ERR_STATE, "nalo_tsdf_replace_last_n: the last operation on this volume was not a window replacement");
    nalo_tsdf_replace_stats own;
    { const int rc = tsdf_replace_last_n(c, v, total ? total : &own, per_pair, cap); if (rc) return rc; }
    *n = v.last_n;
    return NALO_OK;
}

int nalo_tsdf_replace_depth_n(nalo_ctx* c, const nalo_tsdf_replace_args* pairs, int n) {
    const std::string who = "nalo_tsdf_replace_depth_n";
    { const int rc = tsdf_need(c, who.c_str()); if (rc) return rc; }
    if (!pairs || n < 1 || n > kTsdfReplaceMaxPairs) return fail(c, NALO_ERR_ARG, who + ": bad argument (a list of 1 .. 16 pairs is needed)");
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfVolume& v = *c->tsdf;
    // every pair is checked before anything is queued; a refusal is nalo_tsdf_replace_depth's of that pair, with the pair's index in front
    std::vector<TsdfSideDev> sides((size_t)2 * n);
    for (int k = 0; k < n; ++k) {
        const nalo_tsdf_replace_args& a = pairs[k];
        const std::string pk = who + ", pair " + std::to_string(k);
        if (!a.remove && !a.add) return fail(c, NALO_ERR_ARG, pk + ": a side, remove or add, is needed");
        int rc = NALO_OK;
        if (a.remove) rc = tsdf_side_check(c, pk + ", remove", v, a.remove, &sides[2 * k]);
        if (!rc && a.add) rc = tsdf_side_check(c, pk + ", add", v, a.add, &sides[2 * k + 1]);
        TsdfBox B;
        if (!rc && a.use_box) rc = tsdf_sub_box(c, pk, "box", v, true, a.lo, a.size, &B);
        if (rc) return c->err.compare(0, pk.size(), pk) == 0 ? rc : fail(c, rc, pk + ": " + c->err);
        TsdfSideDev& R = sides[2 * k];
        if (R.on && a.use_box) for (int x = 0; x < 3; ++x) { R.lo[x] = std::max(R.lo[x], B.lo[x]); R.hi[x] = std::min(R.hi[x], B.lo[x] + B.size[x]); }
    }
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "tsdf_replace_depth_n");
    for (int k = 0; k < n; ++k) {                                               // every distinct producer stream, once
        hipStream_t prod = (hipStream_t)pairs[k].producer_stream;              // NULL: the null stream, which the context's non-blocking stream does not wait for by itself
        bool seen = prod == (hipStream_t)c->stream;
        for (int q = 0; q < k && !seen; ++q) seen = (hipStream_t)pairs[q].producer_stream == prod;
        if (!seen) { NALO_HIP(c, hipEventRecord(c->ev_prod, prod)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0)); }
    }
    { const int rc = tsdf_replace_n_enqueue(c, v, sides); if (rc) return rc; }
    NALO_HIP(c, hipEventRecord(v.ev_read, c->stream));                         // the callers' planes have been read (one kernel reads all of them): nalo_tsdf_release
    v.read_pending = true;
    return NALO_OK;
}

int nalo_tsdf_replace_frames(nalo_ctx* c, nalo_tsdf_replace_frames_args* a) {
    const std::string who = "nalo_tsdf_replace_frames";
    { const int rc = tsdf_need(c, who.c_str()); if (rc) return rc; }
    if (!c->tsdf_log_on) return fail(c, NALO_ERR_STATE, who + ": the fusion log is not enabled (nalo_tsdf_log_enable)");
    if (!map_dense_on(c)) return fail(c, NALO_ERR_STATE, who + ": the dense archive is not enabled (nalo_map_dense_enable)");
    if (!a) return fail(c, NALO_ERR_ARG, who + ": bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfVolume& v = *c->tsdf;
    // ---- every frame is checked before anything is queued or the log is touched. No frame_id appears twice, so what the loop of nalo_tsdf_replace_frame would
    // find in the log at its call k is what the log holds now
    struct Frame { const nalo_tsdf_log_entry* e; bool has_est, own; int total; std::vector<MapSeg> segs; TsdfSideDev rem{}, add{}; };
    int list_len[kTsdfReplaceMaxPairs]; unsigned char skip[kTsdfReplaceMaxPairs];
    const int n = a->n;
    if (n < 1 || n > kTsdfReplaceMaxPairs) return fail(c, NALO_ERR_ARG, who + ": n outside 1 .. 16");
    if (!a->frame_id) return fail(c, NALO_ERR_ARG, who + ": bad argument");
    std::vector<Frame> fr((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int rc = map_dense_segments(c, who.c_str(), a->frame_id[k], &fr[k].segs, &fr[k].total);      // a sharded window, a frame the archive has never seen
        if (rc) return fail(c, rc, who + ", frame " + std::to_string(k) + ": " + c->err);
        list_len[k] = fr[k].total;
    }
    if (const char* why = tsdf_replace_frames_plan(a, c->tsdf_log.data(), (int)c->tsdf_log.size(), list_len, skip)) return fail(c, NALO_ERR_ARG, who + ": " + why);
    const bool col_now = v.colour.p != nullptr;
    int n_pairs = 0;
    for (int k = 0; k < n; ++k) {
        Frame& f = fr[k];
        const std::string fk = who + ", frame " + std::to_string(k);
        f.e = tsdf_log_find(c, a->frame_id[k]);
        f.has_est = a->est_new && (!a->has_est || a->has_est[k]);
        if (!f.e && !f.has_est) return fail(c, NALO_ERR_ARG, fk + ": nothing to remove (the log has no entry of this frame) and nothing to add");
        if (f.e && f.total < f.e->n_records) return fail(c, NALO_ERR_STATE, fk + ": the frame's dense list is shorter than when it was fused");
        if (skip[k]) continue;
        if (f.e) { const int rc = tsdf_side_camera(c, fk + ", the logged side", v, c->w, c->h, f.e->K, &f.e->est, f.e->min_depth, f.e->max_depth, &f.rem); if (rc) return rc; }
        if (f.has_est) { const int rc = tsdf_side_camera(c, fk, v, c->w, c->h, a->K, &a->est_new[k], a->min_depth, a->max_depth, &f.add); if (rc) return rc; }
        f.own = f.e && f.has_est && f.total > f.e->n_records;
        ++n_pairs;
    }
    a->n_skipped = n - n_pairs;
    if (!n_pairs) return NALO_OK;                                              // every frame is where it was fused: nothing is launched, nalo_tsdf_last stays
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "tsdf_replace_frames");
    size_t need = 0;
    for (int k = 0; k < n; ++k) if (!skip[k]) need += (fr[k].e && (fr[k].own || !fr[k].has_est) ? 1 : 0) + (fr[k].has_est ? 1 : 0);
    if (v.pool.size() < need) v.pool.resize(need);
    if (col_now && v.cpool.size() < need) v.cpool.resize(need);
    if (v.cpool.empty()) v.cpool.resize(1);                                    // tsdf_frame_plane_of names one, and leaves it alone without colour
    std::vector<TsdfSideDev> sides; sides.reserve((size_t)2 * n_pairs);
    size_t at = 0;
    for (int k = 0; k < n; ++k) {
        Frame& f = fr[k];
        if (skip[k]) continue;
        // the add side moves colour iff the volume holds colour now; the remove side iff the frame's fusion moved colour into planes that still exist
        const bool col_add = col_now, col_rem = f.e && f.e->coloured && col_now;
        // the whole list's plane serves both sides unless the list has grown since the frame was fused: then the first n_records records get a plane of their own
        size_t p_rem = 0, p_add = 0;
        if (f.e && (f.own || !f.has_est)) {
            std::vector<MapSeg> head;
            for (const MapSeg& sg : f.segs) if (sg.start < f.e->n_records) { head.push_back(sg); head.back().n = std::min(sg.n, f.e->n_records - sg.start); }
            p_rem = at++;
            const int rc = tsdf_frame_plane_of(c, v, head, col_rem, v.pool[p_rem], v.cpool[col_rem ? p_rem : 0]); if (rc) return rc;
        }
        if (f.has_est) {
            p_add = at++;
            const int rc = tsdf_frame_plane_of(c, v, f.segs, col_add, v.pool[p_add], v.cpool[col_add ? p_add : 0]); if (rc) return rc;
            if (f.e && !f.own) p_rem = p_add;
        }
        // a packed colour plane is a U8 plane of three channels, B first: stride_x 4, stride_c 1
        for (TsdfSideDev* S : {&f.rem, &f.add}) {
            if (!S->on) continue;
            const size_t pl = S == &f.rem ? p_rem : p_add;
            S->depth = reinterpret_cast<const char*>(v.pool[pl].p); S->sy = (long long)c->w * 4; S->sx = 4;
            const bool coloured = S == &f.rem ? col_rem : col_add;
            S->coloured = coloured;
            if (coloured) { S->colour = reinterpret_cast<const unsigned char*>(v.cpool[pl].p); S->csy = (long long)c->w * 4; S->csx = 4; S->csc[0] = 0; S->csc[1] = 1; S->csc[2] = 2; }
        }
        if (f.rem.on) for (int x = 0; x < 3; ++x) { f.rem.lo[x] = std::max(f.rem.lo[x], f.e->lo[x]); f.rem.hi[x] = std::min(f.rem.hi[x], f.e->lo[x] + f.e->size[x]); }      // the resident box
        sides.push_back(f.rem); sides.push_back(f.add);
    }
    { const int rc = tsdf_replace_n_enqueue(c, v, sides); if (rc) return rc; }
    // the log, for all pairs, as the loop would leave it, in the loop's order. tsdf_log_put may move the entries: the frames' pointers are dead from here on
    for (int k = 0; k < n; ++k) {
        if (skip[k]) continue;
        if (fr[k].has_est) tsdf_log_put(c, v, a->frame_id[k], fr[k].total, a->est_new[k], a->K, a->min_depth, a->max_depth);
        else { const nalo_tsdf_log_entry* e = tsdf_log_find(c, a->frame_id[k]); c->tsdf_log.erase(c->tsdf_log.begin() + (e - c->tsdf_log.data())); }
    }
    return NALO_OK;
}

// nalo_tsdf_get (to_volume = 0) and nalo_tsdf_set (1)
// and nalo_tsdf_color_get / _set (bgr != NULL, tsdf = weight = NULL): the three planes of the block, one after the other
static int tsdf_block(nalo_ctx* c, const char* who, const int lo[3], const int size[3], float* tsdf, float* weight, int to_volume, float* bgr = nullptr, bool colour = false) {
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    if (colour) { const int rc = tsdf_need_colour(c, v, who); if (rc) return rc; }
    if (!lo || !size || (!tsdf && !weight && !bgr)) return fail(c, NALO_ERR_ARG, std::string(who) + ": bad argument");
    { const int rc = tsdf_sub_box(c, who, "block", v, true, lo, size, nullptr); if (rc) return rc; }
    NALO_HIP(c, hipSetDevice(c->device));
    // the block goes through a staging tile of whole z slices, at most kTsdfTileFloats (or one slice, at most 2048 x 2048 floats): never a second volume
    const size_t slice = (size_t)size[0] * size[1];
    const int zs = (int)std::max<size_t>(1, std::min<size_t>((size_t)size[2], kTsdfTileFloats / slice));
    NALO_HIP(c, v.block.reserve(slice * zs));
    const size_t blk = slice * size[2];
    float* host[5] = {tsdf, weight, bgr, bgr ? bgr + blk : nullptr, bgr ? bgr + 2 * blk : nullptr};
    float* vol[5] = {v.tsdf.p, v.weight.p, v.colour.p, bgr ? v.colour.p + v.n : nullptr, bgr ? v.colour.p + 2 * v.n : nullptr};
    for (int k = 0; k < 5; ++k) {
        if (!host[k]) continue;
        for (int z0 = 0; z0 < size[2]; z0 += zs) {
            const int tlo[3] = {lo[0], lo[1], lo[2] + z0}, tsz[3] = {size[0], size[1], std::min(zs, size[2] - z0)};
            const size_t nb = slice * tsz[2];
            float* h = host[k] + slice * z0;
            if (to_volume) NALO_HIP(c, hipMemcpyAsync(v.block.p, h, nb * 4, hipMemcpyHostToDevice, c->stream));
            { const int rc = tsdf_block_launch(c, vol[k], v.block.p, v.d.dims, tlo, tsz, to_volume); if (rc) return rc; }
            if (!to_volume) NALO_HIP(c, hipMemcpyAsync(h, v.block.p, nb * 4, hipMemcpyDeviceToHost, c->stream));
            NALO_HIP(c, hipStreamSynchronize(c->stream));                    // the tile is used again, and the caller's memory is its own again
        }
    }
    return NALO_OK;
}
int nalo_tsdf_get(nalo_ctx* c, const int lo[3], const int size[3], float* tsdf, float* weight) { return tsdf_block(c, "nalo_tsdf_get", lo, size, tsdf, weight, 0); }
int nalo_tsdf_set(nalo_ctx* c, const int lo[3], const int size[3], const float* tsdf, const float* weight) {
    return tsdf_block(c, "nalo_tsdf_set", lo, size, const_cast<float*>(tsdf), const_cast<float*>(weight), 1);
}
int nalo_tsdf_color_get(nalo_ctx* c, const int lo[3], const int size[3], float* bgr) { return tsdf_block(c, "nalo_tsdf_color_get", lo, size, nullptr, nullptr, 0, bgr, true); }
int nalo_tsdf_color_set(nalo_ctx* c, const int lo[3], const int size[3], const float* bgr) {
    return tsdf_block(c, "nalo_tsdf_color_set", lo, size, nullptr, nullptr, 1, const_cast<float*>(bgr), true);
}

int nalo_tsdf_color_view(nalo_ctx* c, nalo_tsdf_color_volume_view* out) {
    { const int rc = tsdf_need(c, "nalo_tsdf_color_view"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_color_view: bad argument");
    const TsdfVolume& v = *c->tsdf;
    { const int rc = tsdf_need_colour(c, v, "nalo_tsdf_color_view"); if (rc) return rc; }
    out->bgr = v.colour.p;
    for (int a = 0; a < 3; ++a) out->dims[a] = v.d.dims[a];
    out->stream = (void*)(hipStream_t)c->stream;
    return NALO_OK;
}

int nalo_tsdf_view(nalo_ctx* c, nalo_tsdf_volume_view* out) {
    { const int rc = tsdf_need(c, "nalo_tsdf_view"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_view: bad argument");
    const TsdfVolume& v = *c->tsdf;
    out->tsdf = v.tsdf.p; out->weight = v.weight.p;
    for (int a = 0; a < 3; ++a) out->dims[a] = v.d.dims[a];
    out->stream = (void*)(hipStream_t)c->stream;
    return NALO_OK;
}

int nalo_tsdf_surface_points(nalo_ctx* c, nalo_tsdf_surface_args* a) {
    const char* who = "nalo_tsdf_surface_points";
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!a) return fail(c, NALO_ERR_ARG, "nalo_tsdf_surface_points: bad argument");
    a->n = 0; a->n_needed = 0;
    TsdfVolume& v = *c->tsdf;
    if (a->cap < 0 || (a->cap > 0 && !a->xyz) || std::isnan(a->min_weight)) return fail(c, NALO_ERR_ARG, "nalo_tsdf_surface_points: bad argument");
    TsdfBox B;
    { const int rc = tsdf_sub_box(c, who, "sub-box", v, a->use_box != 0, a->lo, a->size, &B); if (rc) return rc; }
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "tsdf_surface_points");
    // the mesh's vertices on the axis edges: its classify and vertex pass, into this call's own xyz. The device mesh is not touched. Three crossings a voxel
    // of 2^29 stay below 2^31
    TsdfMeshDev D;
    { const int rc = tsdf_mesh_dev(c, v, B, a->min_weight, false, &D); if (rc) return rc; }
    // the device holds room for what the caller has room for, and never for more than the sub-box can give
    const long long room = std::min<long long>(a->cap, 3LL * D.total);
    NALO_HIP(c, v.xyz.reserve(3 * (size_t)std::max<long long>(room, 1))); NALO_HIP(c, v.xyz_h.reserve(3 * (size_t)std::max<long long>(room, 1)));
    D.xyz = v.xyz.p; D.capv = room;
    {
        ProfScope ps(c, "tsdf_surface");
        { const int rc = tsdf_mesh_classify_launch(c, D, true); if (rc) return rc; }
        if (room > 0) { const int rc = tsdf_mesh_write_launch(c, D, true); if (rc) return rc; }
    }
    // the count is known only behind the scan: everything the call may have written comes up in the one wait
    NALO_HIP(c, hipMemcpyAsync(v.mesh_cnt_h.p, D.cntv + D.nb, 4, hipMemcpyDeviceToHost, c->stream));
    if (room > 0) NALO_HIP(c, hipMemcpyAsync(v.xyz_h.p, v.xyz.p, 3 * (size_t)room * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const long long need = v.mesh_cnt_h.p[0];
    if (need < 0 || need > 3LL * D.total) return fail(c, NALO_ERR_HIP, "nalo_tsdf_surface_points: the device counted more crossings than the sub-box can hold");
    a->n_needed = need;
    if (a->cap < need) return fail(c, NALO_ERR_ARG, "nalo_tsdf_surface_points: cap is below the crossings found (n_needed)");
    std::copy(v.xyz_h.p, v.xyz_h.p + 3 * need, a->xyz);
    a->n = need;
    return NALO_OK;
}

// nalo_tsdf_mesh (coloured = false; cc is not looked at) and nalo_tsdf_mesh_color. Dout (nalo_tsdf_archive_mesh): what the passes ran with, once the device mesh is built
static int tsdf_mesh(nalo_ctx* c, const std::string& who, nalo_tsdf_mesh_args* a, bool coloured, nalo_tsdf_mesh_color_args* cc, TsdfMeshDev* Dout = nullptr) {
    { const int rc = tsdf_need(c, who.c_str()); if (rc) return rc; }
    if (!a || (coloured && !cc)) return fail(c, NALO_ERR_ARG, who + ": bad argument");
    a->n_vertices = 0; a->n_triangles = 0;
    TsdfVolume& v = *c->tsdf;
    if (coloured) { const int rc = tsdf_need_colour(c, v, who); if (rc) return rc; }
    if (a->cap_vertices < 0 || a->cap_triangles < 0 || (a->cap_vertices > 0 && !a->xyz) || (a->cap_triangles > 0 && !a->tri) || std::isnan(a->min_weight) ||
        (coloured && (cc->cap < 0 || (cc->cap > 0 && !cc->rgba))))
        return fail(c, NALO_ERR_ARG, who + ": bad argument");
    TsdfBox B;
    { const int rc = tsdf_sub_box(c, who, "sub-box", v, a->use_box != 0, a->lo, a->size, &B); if (rc) return rc; }
    const long long total = B.total;
    if (total > kTsdfMeshMaxVoxels) return fail(c, NALO_ERR_ARG, who + ": the sub-box holds more than 2^28 voxels");
    // ---- accepted: from here on only the runtime can fail, or a host array turn out too small for what the device found
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "tsdf_mesh");
    TsdfMeshDev D;
    { const int rc = tsdf_mesh_dev(c, v, B, a->min_weight, coloured, &D); if (rc) return rc; }
    NALO_HIP(c, v.mesh_base.reserve((size_t)total + 3)); NALO_HIP(c, v.mesh_cntt.reserve((size_t)D.nb + 1));      // mesh_base: whole lanes of four voxels
    if (!v.mesh_xyz.p || !v.mesh_tri.p) {                                      // both or neither: a failure leaves neither
        DevBuf<float> xyz; DevBuf<int> tri;
        NALO_HIP(c, xyz.reserve(3 * (size_t)kTsdfMeshFirstVertices)); NALO_HIP(c, tri.reserve(3 * (size_t)kTsdfMeshFirstTriangles));
        v.mesh_xyz = std::move(xyz); v.mesh_tri = std::move(tri);
    }
    D.vbase = v.mesh_base.p; D.cntt = v.mesh_cntt.p;
    D.xyz = v.mesh_xyz.p; D.tri = v.mesh_tri.p; D.capv = (long long)(v.mesh_xyz.cap / 3); D.capt = (long long)(v.mesh_tri.cap / 3);
    if (coloured) {
        // a word per vertex xyz has room for. It can be short only behind plain meshes that grew xyz, and then holds no mesh's colours (mesh_coloured is false)
        if (v.mesh_rgba.cap < (size_t)D.capv) { v.mesh_coloured = false; NALO_HIP(c, v.mesh_rgba.reserve((size_t)D.capv)); }
        D.rgba = v.mesh_rgba.p;
    }
    // all four passes against the room there is: the steady state waits once, for the two totals
    {
        ProfScope ps(c, "tsdf_mesh");
        { const int rc = tsdf_mesh_classify_launch(c, D, false); if (rc) return rc; }
        { const int rc = tsdf_mesh_write_launch(c, D, false); if (rc) return rc; }
    }
    NALO_HIP(c, hipMemcpyAsync(v.mesh_cnt_h.p, D.cntv + D.nb, 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(v.mesh_cnt_h.p + 1, D.cntt + D.nb, 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const long long nv = v.mesh_cnt_h.p[0], nt = (long long)(unsigned)v.mesh_cnt_h.p[1];
    if (nv < 0 || nv > 7 * total || nt > 12 * total) return fail(c, NALO_ERR_HIP, who + ": the device counted more than the sub-box can hold");
    if (nv > D.capv || nt > D.capt) {
        // nothing was written: the previous mesh is still whole, and stays if the new room cannot be had
        DevBuf<float> xyz; DevBuf<int> tri; DevBuf<unsigned> rgba;
        const long long rv = std::max(D.capv, nv + nv / 4), rt = std::max(D.capt, nt + nt / 4);
        hipError_t e = xyz.reserve(3 * (size_t)rv);
        if (e == hipSuccess) e = tri.reserve(3 * (size_t)rt);
        if (e == hipSuccess && coloured) e = rgba.reserve((size_t)rv);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, NALO_ERR_HIP, who + ": " + hipGetErrorString(e)); }
        v.mesh_xyz = std::move(xyz); v.mesh_tri = std::move(tri);              // the old pair is freed as xyz / tri leave scope: nothing queued names it
        D.xyz = v.mesh_xyz.p; D.tri = v.mesh_tri.p; D.capv = rv; D.capt = rt;
        if (coloured) { v.mesh_rgba = std::move(rgba); D.rgba = v.mesh_rgba.p; }
        ProfScope ps(c, "tsdf_mesh");
        { const int rc = tsdf_mesh_write_launch(c, D, false); if (rc) return rc; }
    }
    v.mesh_nv = nv; v.mesh_nt = nt; v.have_mesh = true; v.mesh_coloured = coloured;
    if (Dout) *Dout = D;
    a->n_vertices = nv; a->n_triangles = nt;
    uint8_t* rgba = coloured ? cc->rgba : nullptr;
    if ((a->xyz && a->cap_vertices < nv) || (a->tri && a->cap_triangles < nt) || (rgba && cc->cap < nv))
        return fail(c, NALO_ERR_ARG, who + ": a cap is below what the mesh holds (n_vertices, n_triangles); the device mesh is built");
    if (a->xyz && nv > 0) NALO_HIP(c, hipMemcpyAsync(a->xyz, v.mesh_xyz.p, 3 * (size_t)nv * 4, hipMemcpyDeviceToHost, c->stream));
    if (a->tri && nt > 0) NALO_HIP(c, hipMemcpyAsync(a->tri, v.mesh_tri.p, 3 * (size_t)nt * 4, hipMemcpyDeviceToHost, c->stream));
    if (rgba && nv > 0) NALO_HIP(c, hipMemcpyAsync(rgba, v.mesh_rgba.p, (size_t)nv * 4, hipMemcpyDeviceToHost, c->stream));
    if ((a->xyz && nv > 0) || (a->tri && nt > 0) || (rgba && nv > 0)) NALO_HIP(c, hipStreamSynchronize(c->stream));
    return NALO_OK;
}
int nalo_tsdf_mesh(nalo_ctx* c, nalo_tsdf_mesh_args* a) { return tsdf_mesh(c, "nalo_tsdf_mesh", a, false, nullptr); }
int nalo_tsdf_mesh_color(nalo_ctx* c, nalo_tsdf_mesh_args* a, nalo_tsdf_mesh_color_args* cc) { return tsdf_mesh(c, "nalo_tsdf_mesh_color", a, true, cc); }


int nalo_tsdf_mesh_view(nalo_ctx* c, nalo_tsdf_mesh_dev* out) {
    { const int rc = tsdf_need(c, "nalo_tsdf_mesh_view"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_mesh_view: bad argument");
    const TsdfVolume& v = *c->tsdf;
    if (!v.have_mesh) return fail(c, NALO_ERR_STATE, "nalo_tsdf_mesh_view: no mesh has been built from this volume (nalo_tsdf_mesh)");
    out->xyz = v.mesh_xyz.p; out->tri = v.mesh_tri.p; out->n_vertices = v.mesh_nv; out->n_triangles = v.mesh_nt;
    out->stream = (void*)(hipStream_t)c->stream;
    return NALO_OK;
}

int nalo_tsdf_mesh_color_view(nalo_ctx* c, nalo_tsdf_mesh_color_dev* out) {
    { const int rc = tsdf_need(c, "nalo_tsdf_mesh_color_view"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_mesh_color_view: bad argument");
    const TsdfVolume& v = *c->tsdf;
    if (!v.have_mesh || !v.mesh_coloured) return fail(c, NALO_ERR_STATE, "nalo_tsdf_mesh_color_view: the last mesh of this volume was not built by nalo_tsdf_mesh_color");
    out->rgba = reinterpret_cast<uint8_t*>(v.mesh_rgba.p); out->n_vertices = v.mesh_nv;
    out->stream = (void*)(hipStream_t)c->stream;
    return NALO_OK;
}

int nalo_tsdf_raycast(nalo_ctx* c, nalo_tsdf_raycast_args* a) {
    const char* who = "nalo_tsdf_raycast";
    if (!c) return NALO_ERR_ARG;
    if (!a) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: bad argument");
    a->n_hit = a->n_back = a->n_normal = 0; a->n_steps = 0;
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    if (a->with_colour) { const int rc = tsdf_need_colour(c, v, who); if (rc) return rc; }
    if (a->w < 1 || a->h < 1 || (long long)a->w * a->h > (1LL << 26)) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: w or h < 1, or more than 2^26 pixels");
    for (int i = 0; i < 4; ++i) if (!std::isfinite(a->K[i])) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: K is not finite");
    if (a->K[0] == 0.0f || a->K[1] == 0.0f) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: fx or fy is 0");
    for (int i = 0; i < 12; ++i) if (!std::isfinite(a->camToWorld[i])) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: camToWorld is not finite");
    int N = 0;
    if (nalo_tsdf_raycast_steps(a->min_depth, a->max_depth, a->step, &N) != NALO_OK)
        return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: min_depth / max_depth / step not finite, min_depth < 0 or > max_depth, step <= 0, or more than 4096 steps");
    if (std::isnan(a->min_weight)) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: min_weight is NaN");
    if ((a->normal && !a->with_normals) || (a->rgba && !a->with_colour)) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast: a host normal / rgba array without its with_ flag");
    // ---- accepted: from here on only the runtime can fail
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "tsdf_raycast");
    const size_t npx = (size_t)a->w * a->h;
    const bool nrm = a->with_normals != 0, col = a->with_colour != 0;
    // everything that has to grow is allocated before anything is replaced: a failed allocation leaves the previous images whole
    {
        DevBuf<float> depth, normal; DevBuf<unsigned> rgba;
        hipError_t e = hipSuccess;
        if (v.rc_depth.cap < npx) e = depth.reserve(npx);
        if (e == hipSuccess && nrm && v.rc_normal.cap < 3 * npx) e = normal.reserve(3 * npx);
        if (e == hipSuccess && col && v.rc_rgba.cap < npx) e = rgba.reserve(npx);
        if (e == hipSuccess) e = v.rc_cnt.reserve(3);
        if (e == hipSuccess) e = v.rc_cnt_h.reserve(3);
        if (e == hipSuccess && a->depth) e = v.rc_depth_h.reserve(npx);
        if (e == hipSuccess && a->normal) e = v.rc_normal_h.reserve(3 * npx);
        if (e == hipSuccess && a->rgba) e = v.rc_rgba_h.reserve(npx);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, NALO_ERR_HIP, std::string("nalo_tsdf_raycast: ") + hipGetErrorString(e)); }
        if (depth.p) v.rc_depth = std::move(depth);                            // the old images are freed as the locals leave scope (hipFree waits for the device)
        if (normal.p) v.rc_normal = std::move(normal);
        if (rgba.p) v.rc_rgba = std::move(rgba);
    }
    TsdfRaycastDev D{};
    D.g = tsdf_grid(v, col);
    for (int k = 0; k < 3; ++k) {
        D.t[k] = (float)a->camToWorld[4 * k + 3];
        for (int j = 0; j < 3; ++j) D.R[3 * k + j] = (float)a->camToWorld[4 * k + j];
    }
    D.min_weight = a->min_weight;
    D.fx = a->K[0]; D.fy = a->K[1]; D.cx = a->K[2]; D.cy = a->K[3]; D.w = a->w; D.h = a->h;
    D.min_depth = a->min_depth; D.step = a->step; D.N = N;
    D.depth = v.rc_depth.p; D.normal = nrm ? v.rc_normal.p : nullptr; D.rgba = col ? v.rc_rgba.p : nullptr; D.cnt = v.rc_cnt.p;
    v.have_rc = false;                                                         // until the new images are queued
    NALO_HIP(c, hipMemsetAsync(v.rc_cnt.p, 0, 3 * sizeof(unsigned long long), c->stream));
    { const int rc = tsdf_raycast_launch(c, D); if (rc) return rc; }
    v.rc_w = a->w; v.rc_h = a->h; v.rc_normal_on = nrm; v.rc_rgba_on = col; v.have_rc = true;
    // one wait, for the counts and whatever is downloaded; the images reach the caller's arrays only behind it
    NALO_HIP(c, hipMemcpyAsync(v.rc_cnt_h.p, v.rc_cnt.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (a->depth) NALO_HIP(c, hipMemcpyAsync(v.rc_depth_h.p, v.rc_depth.p, npx * 4, hipMemcpyDeviceToHost, c->stream));
    if (a->normal) NALO_HIP(c, hipMemcpyAsync(v.rc_normal_h.p, v.rc_normal.p, 3 * npx * 4, hipMemcpyDeviceToHost, c->stream));
    if (a->rgba) NALO_HIP(c, hipMemcpyAsync(v.rc_rgba_h.p, v.rc_rgba.p, npx * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const unsigned long long* n = v.rc_cnt_h.p;
    if (n[0] + n[1] > npx || n[2] > n[0]) return fail(c, NALO_ERR_HIP, "nalo_tsdf_raycast: the device counted more than the view holds");
    if (a->depth) std::copy(v.rc_depth_h.p, v.rc_depth_h.p + npx, a->depth);
    if (a->normal) std::copy(v.rc_normal_h.p, v.rc_normal_h.p + 3 * npx, a->normal);
    if (a->rgba) std::copy(reinterpret_cast<const uint8_t*>(v.rc_rgba_h.p), reinterpret_cast<const uint8_t*>(v.rc_rgba_h.p) + 4 * npx, a->rgba);
    a->n_hit = (long long)n[0]; a->n_back = (long long)n[1]; a->n_normal = (long long)n[2]; a->n_steps = N;
    return NALO_OK;
}

int nalo_tsdf_raycast_view(nalo_ctx* c, nalo_tsdf_raycast_dev* out) {
    { const int rc = tsdf_need(c, "nalo_tsdf_raycast_view"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_raycast_view: bad argument");
    const TsdfVolume& v = *c->tsdf;
    if (!v.have_rc) return fail(c, NALO_ERR_STATE, "nalo_tsdf_raycast_view: this volume has not been ray-cast (nalo_tsdf_raycast)");
    const long long w = v.rc_w;
    out->depth = nalo_dev_plane{v.rc_depth.p, NALO_DT_F32, v.rc_w, v.rc_h, 1, 4 * w, 4, 0};
    out->normal = nalo_dev_plane{v.rc_normal_on ? v.rc_normal.p : nullptr, NALO_DT_F32, v.rc_w, v.rc_h, 3, 12 * w, 12, 4};
    out->rgba = nalo_dev_plane{v.rc_rgba_on ? v.rc_rgba.p : nullptr, NALO_DT_U8, v.rc_w, v.rc_h, 3, 4 * w, 4, 1};   // R, G, B as three channels; the alpha byte lies between pixels
    out->w = v.rc_w; out->h = v.rc_h;
    out->stream = (void*)(hipStream_t)c->stream;
    return NALO_OK;
}

// ---- the alignment (nalo_tsdf_align_*)
// the checks every alignment call makes of args and estimate behind the plane's own; NULL when good, else the reason
static const char* tsdf_align_refusal(const nalo_tsdf_align_args* a, const nalo_tsdf_align_est* e, int w, int h) {
    if (a->step < 1) return "step < 1";
    if (a->dof != 6 && a->dof != 7) return "dof is 6 or 7";
    for (int i = 0; i < 12; ++i) if (!std::isfinite(e->camToWorld[i])) return "camToWorld is not finite";
    for (int i = 0; i < 4; ++i) if (!std::isfinite(a->K[i])) return "K is not finite";
    if (!std::isfinite(e->s) || e->s <= 0.0) return "s is not finite or <= 0";
    if (!std::isfinite(a->huber) || a->huber <= 0.0f) return "huber is not finite or <= 0";
    if (!std::isfinite(a->min_depth) || !std::isfinite(a->max_depth) || a->min_depth > a->max_depth) return "min_depth / max_depth not finite, or min_depth > max_depth";
    if (std::isnan(a->min_weight)) return "min_weight is NaN";
    if (a->records && a->records_cap < (long long)w * h * 10) return "records_cap is below h w 10";
    return nullptr;
}
static const char* tsdf_align_loop_refusal(const nalo_tsdf_align_args* a, const nalo_tsdf_align_result* r) {
    if (a->max_iterations < 1 || a->max_iterations > 64) return "max_iterations outside 1..64";
    if (!std::isfinite(a->lambda0) || a->lambda0 < 0.0 || !std::isfinite(a->eps) || a->eps < 0.0) return "lambda0 or eps is negative or not finite";
    if (r->trace_cap < 0 || (r->trace_cap > 0 && !r->trace)) return "a negative trace_cap, or a trace_cap without a trace";
    return nullptr;
}
static void tsdf_align_zero(nalo_tsdf_align_result* r) { r->iterations = r->evaluations = r->n_trace = 0; r->n_first = r->n_last = 0; }

// one plane as the kernel reads it
struct TsdfAlignPlane { const char* p; long long sy, sx; int w, h; };

// everything is validated: one launch, one wait, the sums. The scratch is sized here, before anything is queued
static int tsdf_align_evaluate(nalo_ctx* c, TsdfVolume& v, const TsdfAlignPlane& pl, const nalo_tsdf_align_args* a, const nalo_tsdf_align_est* e, nalo_tsdf_align_sums* out) {
    TsdfAlignDev D{};
    D.g = tsdf_grid(v, false);
    D.min_weight = a->min_weight;
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) D.M[4 * k + j] = (float)(e->s * e->camToWorld[4 * k + j]);
        D.M[4 * k + 3] = (float)e->camToWorld[4 * k + 3];
    }
    D.fx = a->K[0]; D.fy = a->K[1]; D.cx = a->K[2]; D.cy = a->K[3];
    D.min_depth = a->min_depth; D.max_depth = a->max_depth; D.huber = a->huber; D.step = a->step; D.dof = a->dof;
    D.depth = pl.p; D.sy = pl.sy; D.sx = pl.sx; D.w = pl.w; D.h = pl.h;
    D.vw = (int)(((long long)pl.w + a->step - 1) / a->step); D.vh = (int)(((long long)pl.h + a->step - 1) / a->step);
    D.records = a->records;
    const size_t nb = (size_t)tsdf_align_blocks(D.vw, D.vh);
    NALO_HIP(c, v.al_partial.reserve(nb * kTsdfAlignStride));
    if (!v.al_ticket.p) { NALO_HIP(c, v.al_ticket.reserve(4)); NALO_HIP(c, hipMemsetAsync(v.al_ticket.p, 0, 16, c->stream)); }
    NALO_HIP(c, v.al_out.reserve(48, hipHostMallocMapped));
    D.partial = v.al_partial.p; D.ticket = v.al_ticket.p; D.out = v.al_out.dev;
    { const int rc = tsdf_align_launch(c, D); if (rc) return rc; }
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const double* o = v.al_out.p;
    std::copy(o, o + 28, out->H); std::copy(o + 28, o + 35, out->b); out->E = o[35]; out->rr = o[36];
    long long total = 0;
    for (int k = 0; k < 4; ++k) { out->count[k] = (long long)reinterpret_cast<const unsigned long long*>(o)[kTsdfAlignSums + k]; total += out->count[k]; }
    if (total != (long long)D.vw * D.vh) return fail(c, NALO_ERR_HIP, "nalo_tsdf_align: the device's state counts do not add up to the visited pixels");
    return NALO_OK;
}

// the Levenberg-Marquardt loop of the header over tsdf_align_evaluate; everything is validated
static int tsdf_align_loop(nalo_ctx* c, TsdfVolume& v, const TsdfAlignPlane& pl, const nalo_tsdf_align_args* a, const nalo_tsdf_align_est* est_in, nalo_tsdf_align_result* r) {
    const long long need = std::max(a->min_used, 1);
    auto trace = [&](const nalo_tsdf_align_est& e, double lambda, const nalo_tsdf_align_sums& s, int accepted) {
        if (r->evaluations < r->trace_cap) {
            nalo_tsdf_align_trace& t = r->trace[r->evaluations];
            t.est = e; t.lambda = lambda; t.E = s.E; std::copy(s.count, s.count + 4, t.count); t.accepted = accepted;
            r->n_trace = r->evaluations + 1;
        }
        ++r->evaluations;
    };
    tsdf_align_zero(r);
    nalo_tsdf_align_est cur = *est_in;
    nalo_tsdf_align_sums S{};
    double lambda = a->lambda0 == 0.0 ? 0.01 : a->lambda0;
    { const int rc = tsdf_align_evaluate(c, v, pl, a, &cur, &S); if (rc) return rc; }
    trace(cur, lambda, S, 1);
    r->E_first = S.E; r->n_first = S.count[0];
    r->status = NALO_TSDF_ALIGN_ITERATION_LIMIT;
    if (S.count[0] < need) r->status = NALO_TSDF_ALIGN_TOO_FEW;
    else
        for (int it = 0; it < a->max_iterations; ++it) {
            double inc[7]; nalo_tsdf_align_est cand; nalo_tsdf_align_sums Sn{};
            if (nalo_tsdf_align_step(S.H, S.b, lambda, a->dof, &cur, inc, &cand) != NALO_OK) { r->status = NALO_TSDF_ALIGN_SOLVE_FAILED; break; }
            ++r->iterations;
            { const int rc = tsdf_align_evaluate(c, v, pl, a, &cand, &Sn); if (rc) return rc; }
            const bool ok = Sn.count[0] >= need && Sn.E / (double)Sn.count[0] < S.E / (double)S.count[0];
            trace(cand, lambda, Sn, ok ? 1 : 0);
            if (ok) { cur = cand; S = Sn; lambda *= 0.5; } else lambda *= 4.0;
            double n2 = 0.0;
            for (int i = 0; i < 7; ++i) n2 += inc[i] * inc[i];
            if (std::sqrt(n2) <= a->eps) { r->status = NALO_TSDF_ALIGN_CONVERGED; break; }
        }
    r->est = cur; r->last = S; r->E_last = S.E; r->n_last = S.count[0];
    return NALO_OK;
}

// the caller's plane, checked as nalo_tsdf_integrate_depth checks its own
static int tsdf_align_plane(nalo_ctx* c, const char* who, const nalo_dev_plane* d, TsdfAlignPlane* pl) {
    { const int rc = nalo_dev_plane_check(c, d); if (rc) return rc; }
    if (d->dtype != NALO_DT_F32 || d->channels != 1) return fail(c, NALO_ERR_ARG, std::string(who) + ": the depth plane is one channel of F32");
    *pl = TsdfAlignPlane{static_cast<const char*>(d->ptr), d->stride_y, d->stride_x, d->w, d->h};
    return NALO_OK;
}
// the main stream behind the plane's producer, as nalo_tsdf_integrate_depth; tsdf_align_read behind the last kernel that reads the plane
static int tsdf_align_order(nalo_ctx* c, void* producer) {
    hipStream_t prod = (hipStream_t)producer;
    NALO_HIP(c, c->ev_prod.create(hipEventDisableTiming));
    if (prod != (hipStream_t)c->stream) { NALO_HIP(c, hipEventRecord(c->ev_prod, prod)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0)); }
    return NALO_OK;
}
static int tsdf_align_read(nalo_ctx* c, TsdfVolume& v) {
    NALO_HIP(c, hipEventRecord(v.ev_read, c->stream));
    v.read_pending = true;
    return NALO_OK;
}

int nalo_tsdf_align_eval(nalo_ctx* c, const nalo_tsdf_align_args* a, const nalo_tsdf_align_est* est, nalo_tsdf_align_sums* out) {
    const char* who = "nalo_tsdf_align_eval";
    if (!c) return NALO_ERR_ARG;
    if (out) std::fill(out->count, out->count + 4, 0LL);
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!a || !est || !out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_align_eval: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfVolume& v = *c->tsdf;
    TsdfAlignPlane pl;
    { const int rc = tsdf_align_plane(c, who, &a->depth, &pl); if (rc) return rc; }
    if (const char* why = tsdf_align_refusal(a, est, pl.w, pl.h)) return fail(c, NALO_ERR_ARG, std::string(who) + ": " + why);
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "tsdf_align_eval");
    { const int rc = tsdf_align_order(c, a->producer_stream); if (rc) return rc; }
    nalo_tsdf_align_sums S{};
    { const int rc = tsdf_align_evaluate(c, v, pl, a, est, &S); if (rc) return rc; }
    *out = S;
    return tsdf_align_read(c, v);
}

int nalo_tsdf_align_depth(nalo_ctx* c, const nalo_tsdf_align_args* a, const nalo_tsdf_align_est* est_in, nalo_tsdf_align_result* r) {
    const char* who = "nalo_tsdf_align_depth";
    if (!c) return NALO_ERR_ARG;
    if (r) tsdf_align_zero(r);
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!a || !est_in || !r) return fail(c, NALO_ERR_ARG, "nalo_tsdf_align_depth: bad argument");
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfVolume& v = *c->tsdf;
    TsdfAlignPlane pl;
    { const int rc = tsdf_align_plane(c, who, &a->depth, &pl); if (rc) return rc; }
    if (const char* why = tsdf_align_refusal(a, est_in, pl.w, pl.h)) return fail(c, NALO_ERR_ARG, std::string(who) + ": " + why);
    if (const char* why = tsdf_align_loop_refusal(a, r)) return fail(c, NALO_ERR_ARG, std::string(who) + ": " + why);
    // ---- accepted: from here on only the runtime can fail
    HostTimer ht(c, "tsdf_align_depth");
    { const int rc = tsdf_align_order(c, a->producer_stream); if (rc) return rc; }
    { const int rc = tsdf_align_loop(c, v, pl, a, est_in, r); if (rc) return rc; }
    return tsdf_align_read(c, v);
}

int nalo_tsdf_align_frame(nalo_ctx* c, int frame_id, const nalo_tsdf_align_args* a, const nalo_tsdf_align_est* est_in, nalo_tsdf_align_result* r) {
    const char* who = "nalo_tsdf_align_frame";
    if (!c) return NALO_ERR_ARG;
    if (r) tsdf_align_zero(r);
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    if (!a || !est_in || !r) return fail(c, NALO_ERR_ARG, "nalo_tsdf_align_frame: bad argument");
    if (!map_dense_on(c)) return fail(c, NALO_ERR_STATE, "nalo_tsdf_align_frame: the dense archive is not enabled (nalo_map_dense_enable)");
    TsdfVolume& v = *c->tsdf;
    if (const char* why = tsdf_align_refusal(a, est_in, c->w, c->h)) return fail(c, NALO_ERR_ARG, std::string(who) + ": " + why);
    if (const char* why = tsdf_align_loop_refusal(a, r)) return fail(c, NALO_ERR_ARG, std::string(who) + ": " + why);
    HostTimer ht(c, "tsdf_align_frame");
    { const int rc = tsdf_frame_plane(c, who, v, frame_id, false); if (rc) return rc; }
    const TsdfAlignPlane pl = {reinterpret_cast<const char*>(v.plane.p), (long long)c->w * 4, 4, c->w, c->h};
    return tsdf_align_loop(c, v, pl, a, est_in, r);
}

// ---- the mesh archive
static int tsdf_archive_need(nalo_ctx* c, const char* who) {
    if (!c) return NALO_ERR_ARG;
    if (!c->tsdf_archive) return fail(c, NALO_ERR_STATE, std::string(who) + ": the archive is not enabled (nalo_tsdf_archive_enable)");
    return NALO_OK;
}
static void tsdf_archive_fill_stats(const TsdfArchive& A, struct nalo_tsdf_archive_stats* out) {
    out->added_vertices = A.added_v; out->welded_vertices = A.welded_v; out->added_triangles = A.added_t;
    out->n_vertices = A.nv; out->n_triangles = A.nt;
    out->cap_vertices = A.cap_v; out->cap_triangles = A.cap_t; out->table_slots = A.slots;
    out->coloured = A.coloured ? 1 : 0; out->have_lattice = A.have_lattice ? 1 : 0;
    std::memcpy(out->origin0, A.origin0, sizeof A.origin0); std::memcpy(&out->voxel_size, &A.voxel_size, 4);
}
static unsigned tsdf_word(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
// the smallest power of two of slots that holds nv vertices at a load of one half or less
static long long tsdf_archive_slots_for(long long nv) {
    long long s = kTsdfArchiveFirstSlots;
    while (s < 2 * nv) s *= 2;
    return s;
}

int nalo_tsdf_archive_enable(nalo_ctx* c) {
    if (!c) return NALO_ERR_ARG;
    if (c->tsdf_archive) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    TsdfArchive* A = new TsdfArchive();
    A->coloured = c->tsdf && c->tsdf->colour.p;
    hipError_t e = A->xyz.reserve(3 * (size_t)kTsdfArchiveFirstVertices);
    if (e == hipSuccess) e = A->key.reserve((size_t)kTsdfArchiveFirstVertices);
    if (e == hipSuccess && A->coloured) e = A->rgba.reserve((size_t)kTsdfArchiveFirstVertices);
    if (e == hipSuccess) e = A->tri.reserve(3 * (size_t)kTsdfArchiveFirstTriangles);
    if (e == hipSuccess) e = A->table.reserve((size_t)kTsdfArchiveFirstSlots);
    if (e == hipSuccess) e = A->err.reserve(1);
    if (e == hipSuccess) e = A->back.reserve(2);
    if (e == hipSuccess) e = hipMemsetAsync(A->table.p, 0xFF, (size_t)kTsdfArchiveFirstSlots * sizeof(int), c->stream);      // kTsdfArchiveEmpty is all bits set
    if (e == hipSuccess) e = hipMemsetAsync(A->err.p, 0, sizeof(int), c->stream);
    if (e != hipSuccess) { delete A; (void)hipGetLastError(); return fail(c, NALO_ERR_HIP, std::string("nalo_tsdf_archive_enable: ") + hipGetErrorString(e)); }
    A->cap_v = kTsdfArchiveFirstVertices; A->cap_t = kTsdfArchiveFirstTriangles; A->slots = kTsdfArchiveFirstSlots;
    c->tsdf_archive = A;
    return NALO_OK;
}

int nalo_tsdf_archive_disable(nalo_ctx* c) {
    if (!c) return NALO_ERR_ARG;
    if (!c->tsdf_archive) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamSynchronize(c->stream));                              // kernels that name the arrays may still be queued
    tsdf_archive_destroy(c);
    return NALO_OK;
}

int nalo_tsdf_archive_reset(nalo_ctx* c) {
    { const int rc = tsdf_archive_need(c, "nalo_tsdf_archive_reset"); if (rc) return rc; }
    TsdfArchive& A = *c->tsdf_archive;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipMemsetAsync(A.table.p, 0xFF, (size_t)A.slots * sizeof(int), c->stream));
    A.nv = A.nt = 0; A.added_v = A.welded_v = A.added_t = 0; A.have_lattice = false;
    return NALO_OK;
}

int nalo_tsdf_archive_stats(nalo_ctx* c, struct nalo_tsdf_archive_stats* out) {
    { const int rc = tsdf_archive_need(c, "nalo_tsdf_archive_stats"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_archive_stats: bad argument");
    tsdf_archive_fill_stats(*c->tsdf_archive, out);
    return NALO_OK;
}

// an all-empty table of `slots` filled from the first nv keys
static int tsdf_archive_rebuild(nalo_ctx* c, TsdfArchive& A, int* table, long long slots, long long nv) {
    NALO_HIP(c, hipMemsetAsync(table, 0xFF, (size_t)slots * sizeof(int), c->stream));
    return tsdf_archive_rebuild_launch(c, A.key.p, (int)nv, table, (unsigned)(slots - 1), A.err.p);
}

// the append behind a mesh call that succeeded: D is what its passes ran with, v.mesh_* the device mesh
static int tsdf_archive_append(nalo_ctx* c, TsdfArchive& A, TsdfVolume& v, const TsdfMeshDev& D) {
    const char* who = "nalo_tsdf_archive_mesh";
    const long long nv = v.mesh_nv, nt = v.mesh_nt;
    const long long need_v = A.nv + nv, need_t = A.nt + nt;                       // the worst case: every piece vertex is new
    if (need_v > kTsdfArchiveMax || need_t > kTsdfArchiveMax) return fail(c, NALO_ERR_ARG, "nalo_tsdf_archive_mesh: the archive would pass 2^31 - 1 vertices or triangles");
    if (nv == 0) {                                                             // no vertex, so no triangle: nothing to queue
        A.added_v = A.welded_v = A.added_t = 0;
        if (!A.have_lattice) { for (int k = 0; k < 3; ++k) A.origin0[k] = tsdf_word(v.origin0[k]); A.voxel_size = tsdf_word(v.d.voxel_size); A.have_lattice = true; }
        return NALO_OK;
    }
    // everything that has to grow is allocated before anything is replaced: a failed allocation leaves the archive as it was
    const long long rv = need_v > A.cap_v ? std::min(kTsdfArchiveMax, need_v + need_v / 4) : A.cap_v;
    const long long rt = need_t > A.cap_t ? std::min(kTsdfArchiveMax, need_t + need_t / 4) : A.cap_t;
    const long long slots = std::max(A.slots, tsdf_archive_slots_for(need_v));
    const int nb = (int)((nv + 255) / 256);
    {
        DevBuf<float> xyz; DevBuf<unsigned> rgba; DevBuf<int4> key; DevBuf<int> tri, table;
        hipError_t e = hipSuccess;
        if (rv > A.cap_v) {
            e = xyz.reserve(3 * (size_t)rv);
            if (e == hipSuccess) e = key.reserve((size_t)rv);
            if (e == hipSuccess && A.coloured) e = rgba.reserve((size_t)rv);
        }
        if (e == hipSuccess && rt > A.cap_t) e = tri.reserve(3 * (size_t)rt);
        if (e == hipSuccess && slots > A.slots) e = table.reserve((size_t)slots);
        if (e == hipSuccess) e = A.p_key.reserve((size_t)nv);
        if (e == hipSuccess) e = A.p_map.reserve((size_t)nv);
        if (e == hipSuccess) e = A.cnt.reserve((size_t)nb + 1);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, NALO_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
        // the contents move on the main stream, behind everything that wrote them; the old arrays are freed as the locals leave scope (hipFree waits for the device)
        if (xyz.p) {
            if (A.nv > 0) {
                NALO_HIP(c, hipMemcpyAsync(xyz.p, A.xyz.p, 3 * (size_t)A.nv * 4, hipMemcpyDeviceToDevice, c->stream));
                NALO_HIP(c, hipMemcpyAsync(key.p, A.key.p, (size_t)A.nv * sizeof(int4), hipMemcpyDeviceToDevice, c->stream));
                if (A.coloured) NALO_HIP(c, hipMemcpyAsync(rgba.p, A.rgba.p, (size_t)A.nv * 4, hipMemcpyDeviceToDevice, c->stream));
            }
            A.xyz = std::move(xyz); A.key = std::move(key); if (A.coloured) A.rgba = std::move(rgba);
            A.cap_v = rv;
        }
        if (tri.p) {
            if (A.nt > 0) NALO_HIP(c, hipMemcpyAsync(tri.p, A.tri.p, 3 * (size_t)A.nt * 4, hipMemcpyDeviceToDevice, c->stream));
            A.tri = std::move(tri); A.cap_t = rt;
        }
        if (table.p) {
            { const int rc = tsdf_archive_rebuild(c, A, table.p, slots, A.nv); if (rc) return rc; }
            A.table = std::move(table); A.slots = slots;
        }
    }
    TsdfArchiveDev P{};
    P.vmask = D.vmask; P.vbase = D.vbase; P.total = D.total;
    for (int k = 0; k < 3; ++k) { P.lo[k] = D.lo[k]; P.size[k] = D.size[k]; P.base[k] = v.base[k]; }
    P.p_xyz = v.mesh_xyz.p; P.p_rgba = A.coloured ? v.mesh_rgba.p : nullptr; P.p_tri = v.mesh_tri.p; P.p_nv = (int)nv; P.p_nt = (int)nt;
    P.p_key = A.p_key.p; P.p_map = A.p_map.p; P.cnt = A.cnt.p; P.nb = nb;
    P.xyz = A.xyz.p; P.rgba = A.coloured ? A.rgba.p : nullptr; P.key = A.key.p; P.tri = A.tri.p; P.nv = (int)A.nv; P.nt = (int)A.nt;
    P.table = A.table.p; P.mask = (unsigned)(A.slots - 1); P.err = A.err.p;
    {
        ProfScope ps(c, "tsdf_archive");
        { const int rc = tsdf_archive_keys_launch(c, P); if (rc) return rc; }
        { const int rc = tsdf_archive_append_launch(c, P); if (rc) return rc; }
    }
    // the one wait of the append: how many vertices were new, and the flag
    NALO_HIP(c, hipMemcpyAsync(A.back.p, P.cnt + nb, 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(A.back.p + 1, A.err.p, 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const long long added = A.back.p[0];
    if (A.back.p[1] != 0 || added < 0 || added > nv) {
        // what the passes wrote lies behind nv and nt and is not part of the archive; the table may name it, so it is made again from the vertices that are
        NALO_HIP(c, hipMemsetAsync(A.err.p, 0, sizeof(int), c->stream));
        { const int rc = tsdf_archive_rebuild(c, A, A.table.p, A.slots, A.nv); if (rc) return rc; }
        return fail(c, NALO_ERR_HIP, "nalo_tsdf_archive_mesh: a probe ran through the whole table, or the device counted more new vertices than the piece holds");
    }
    A.nv += added; A.nt += nt;
    A.added_v = added; A.welded_v = nv - added; A.added_t = nt;
    if (!A.have_lattice) { for (int k = 0; k < 3; ++k) A.origin0[k] = tsdf_word(v.origin0[k]); A.voxel_size = tsdf_word(v.d.voxel_size); A.have_lattice = true; }
    return NALO_OK;
}

int nalo_tsdf_archive_mesh(nalo_ctx* c, nalo_tsdf_mesh_args* m, struct nalo_tsdf_archive_stats* out) {
    const char* who = "nalo_tsdf_archive_mesh";
    if (out) { const struct nalo_tsdf_archive_stats none = {}; *out = none; }
    { const int rc = tsdf_archive_need(c, who); if (rc) return rc; }
    TsdfArchive& A = *c->tsdf_archive;
    if (out) { tsdf_archive_fill_stats(A, out); out->added_vertices = out->welded_vertices = out->added_triangles = 0; }
    { const int rc = tsdf_need(c, who); if (rc) return rc; }
    TsdfVolume& v = *c->tsdf;
    const bool other_colour = (v.colour.p != nullptr) != A.coloured;
    bool other_lattice = false;
    if (A.have_lattice) {
        for (int k = 0; k < 3; ++k) other_lattice |= tsdf_word(v.origin0[k]) != A.origin0[k];
        other_lattice |= tsdf_word(v.d.voxel_size) != A.voxel_size;
    }
    if (other_colour || other_lattice) {
        // refused, but behind a mesh call: the plain mesh of the box is built as nalo_tsdf_mesh would build it
        { const int rc = tsdf_mesh(c, who, m, false, nullptr); if (rc) return rc; }
        return fail(c, NALO_ERR_STATE, other_colour ? "nalo_tsdf_archive_mesh: the volume's colour state differs from the archive's (the device mesh is built)"
                                                    : "nalo_tsdf_archive_mesh: the volume's origin0 or voxel_size differ from the archive's lattice (the device mesh is built)");
    }
    TsdfMeshDev D;
    nalo_tsdf_mesh_color_args cc{0, nullptr};
    { const int rc = tsdf_mesh(c, who, m, A.coloured, &cc, &D); if (rc) return rc; }
    HostTimer ht(c, "tsdf_archive");
    { const int rc = tsdf_archive_append(c, A, v, D); if (rc) return rc; }
    if (out) tsdf_archive_fill_stats(A, out);
    return NALO_OK;
}

int nalo_tsdf_archive_get(nalo_ctx* c, nalo_tsdf_archive_get_args* a) {
    const char* who = "nalo_tsdf_archive_get";
    { const int rc = tsdf_archive_need(c, who); if (rc) return rc; }
    if (!a) return fail(c, NALO_ERR_ARG, "nalo_tsdf_archive_get: bad argument");
    TsdfArchive& A = *c->tsdf_archive;
    a->n_vertices = A.nv; a->n_triangles = A.nt;
    if (a->cap_vertices < 0 || a->cap_triangles < 0 || a->cap_rgba < 0 || a->cap_key < 0 || (a->cap_vertices > 0 && !a->xyz) || (a->cap_triangles > 0 && !a->tri) ||
        (a->cap_rgba > 0 && !a->rgba) || (a->cap_key > 0 && !a->key))
        return fail(c, NALO_ERR_ARG, "nalo_tsdf_archive_get: bad argument");
    if (a->rgba && !A.coloured) return fail(c, NALO_ERR_STATE, "nalo_tsdf_archive_get: the archive holds no colour");
    if ((a->xyz && a->cap_vertices < A.nv) || (a->tri && a->cap_triangles < A.nt) || (a->rgba && a->cap_rgba < A.nv) || (a->key && a->cap_key < A.nv))
        return fail(c, NALO_ERR_ARG, "nalo_tsdf_archive_get: a cap is below what the archive holds (n_vertices, n_triangles)");
    NALO_HIP(c, hipSetDevice(c->device));
    bool any = false;
    if (a->xyz && A.nv > 0) { NALO_HIP(c, hipMemcpyAsync(a->xyz, A.xyz.p, 3 * (size_t)A.nv * 4, hipMemcpyDeviceToHost, c->stream)); any = true; }
    if (a->tri && A.nt > 0) { NALO_HIP(c, hipMemcpyAsync(a->tri, A.tri.p, 3 * (size_t)A.nt * 4, hipMemcpyDeviceToHost, c->stream)); any = true; }
    if (a->rgba && A.nv > 0) { NALO_HIP(c, hipMemcpyAsync(a->rgba, A.rgba.p, (size_t)A.nv * 4, hipMemcpyDeviceToHost, c->stream)); any = true; }
    if (a->key && A.nv > 0) { NALO_HIP(c, hipMemcpyAsync(a->key, A.key.p, (size_t)A.nv * sizeof(int4), hipMemcpyDeviceToHost, c->stream)); any = true; }
    if (any) NALO_HIP(c, hipStreamSynchronize(c->stream));
    return NALO_OK;
}

int nalo_tsdf_archive_view(nalo_ctx* c, nalo_tsdf_archive_dev* out) {
    { const int rc = tsdf_archive_need(c, "nalo_tsdf_archive_view"); if (rc) return rc; }
    if (!out) return fail(c, NALO_ERR_ARG, "nalo_tsdf_archive_view: bad argument");
    const TsdfArchive& A = *c->tsdf_archive;
    out->xyz = A.xyz.p; out->tri = A.tri.p; out->rgba = A.coloured ? reinterpret_cast<uint8_t*>(A.rgba.p) : nullptr; out->key = reinterpret_cast<int*>(A.key.p);
    out->n_vertices = A.nv; out->n_triangles = A.nt;
    out->stream = (void*)(hipStream_t)c->stream;
    return NALO_OK;
}

int nalo_tsdf_follow(nalo_ctx* c, const double centre[3], const int margin[3], float min_weight, int shift_out[3], nalo_tsdf_follow_stats* stats) {
    const char* who = "nalo_tsdf_follow";
    if (stats) *stats = nalo_tsdf_follow_stats{};
    { const int rc = tsdf_archive_need(c, who); if (rc) return rc; }
    struct nalo_tsdf_geometry g;
    { const int rc = nalo_tsdf_geometry(c, &g); if (rc) return rc; }
    int shift[3];
    if (nalo_tsdf_shift_for(&g.desc, centre, margin, shift) != NALO_OK) return fail(c, NALO_ERR_ARG, "nalo_tsdf_follow: nalo_tsdf_shift_for refused centre or margin");
    if (shift_out) std::copy(shift, shift + 3, shift_out);
    if (shift[0] || shift[1] || shift[2]) {
        struct nalo_tsdf_shift_boxes B;
        if (nalo_tsdf_shift_boxes(g.desc.dims, shift, &B) != NALO_OK) return fail(c, NALO_ERR_ARG, "nalo_tsdf_follow: nalo_tsdf_shift_boxes refused the shift");
        for (int b = 0; b < B.n_boxes; ++b) {
            nalo_tsdf_mesh_args m{};
            m.use_box = 1; m.min_weight = min_weight;
            for (int k = 0; k < 3; ++k) { m.lo[k] = B.lo[b][k]; m.size[k] = B.size[b][k]; }
            struct nalo_tsdf_archive_stats st;
            { const int rc = nalo_tsdf_archive_mesh(c, &m, &st); if (rc) return rc; }
            if (stats) {
                stats->n_boxes = b + 1;
                stats->added_vertices += st.added_vertices; stats->welded_vertices += st.welded_vertices; stats->added_triangles += st.added_triangles;
            }
        }
    }
    { const int rc = nalo_tsdf_shift(c, shift); if (rc) return rc; }
    if (stats) { stats->n_vertices = c->tsdf_archive->nv; stats->n_triangles = c->tsdf_archive->nt; }
    return NALO_OK;
}
