// The archive of removed points and the entry points that publish from it (nalo_map_*, include/nalo_gpu.h; kernels: kernels_map.hip).
// The archive is a list of device chunks of `chunk` records; position q of the archive is record q % chunk of chunk q / chunk. A chunk is allocated once and
// never moved. The host keeps, per frame_id, the runs (position, count) its records were appended in and the two totals: W small integers per keyframe.
#include "nalo_internal.h"
#include "map_point_math.h"

#include <algorithm>
#include <cmath>
#include <memory>

namespace nalo {

struct MapRun { long long off; int n; };
struct MapFrame { std::vector<MapRun> runs; int cnt[2] = {0, 0}; };          // cnt: {marginalised, out}

struct MapArchive {
    bool on = false;
    int chunk = 0;                                                          // records per chunk; fixed while the archive holds chunks
    long long filled = 0;
    std::vector<DevBuf<nalo_map_record>> chunks;
    DevBuf<nalo_map_record*> tab; size_t tab_n = 0;                         // the chunks' addresses on the device, re-sent when one is added
    std::map<int, MapFrame> frames;
    // the append of nalo_ba_marginalize_flagged: block counts, the per-host counters (two buffers of 2 * NALO_MAX_WINDOW, the idle one zero) and their pinned mirror
    DevBuf<int> cnt, hs; int hs_buf = 0; HostBuf<int> hs_host;
    MapAppendDev pend{}; int pend_W = 0; bool pending = false;
    // the clouds: segment table (pinned staging + device), draws, block counts + statistics, outputs and their pinned mirrors
    HostBuf<MapSeg> seg_h; DevBuf<MapSeg> seg_d; HostBuf<int> draws_h; DevBuf<int> draws_d, qcnt;
    DevBuf<double> wxyz; HostBuf<double> wxyz_h;
    DevBuf<float> cxyz; DevBuf<uint8_t> crgb; HostBuf<float> cxyz_h; HostBuf<uint8_t> crgb_h; HostBuf<int> stats_h;
    // the window panel (nalo_map_window_plot): segment table (pinned staging + device), the key plane (zero between calls), the sources' colours, the images, the
    // select's results, the ring counters (two buffers, the idle one zero; refilled with the plane) and the pinned block results, counters and images come up through
    HostBuf<PlotSeg> wp_seg_h; DevBuf<PlotSeg> wp_seg_d; KeyPlane<unsigned, 0> wp_key; DevBuf<unsigned> wp_col, wp_res; DevBuf<uint8_t> wp_bgr; DevBuf<int> wp_cnt; int wp_cnt_buf = 0;
    HostBuf<uint8_t> wp_host;
    // the 3-D panel (nalo_map_render): the transform table and the clipped segments (pinned staging + device), the 64-bit key plane (all-ones between calls), the
    // counters (two buffers, the idle one zero; refilled with the plane), the images and the pinned block counters and images come up through
    HostBuf<float> mr_M_h; DevBuf<float> mr_M_d, mr_depth; HostBuf<MrLine> mr_lines_h; DevBuf<MrLine> mr_lines_d;
    KeyPlane<unsigned long long, 0xFF> mr_key; DevBuf<unsigned long long> mr_cnt; int mr_cnt_buf = 0;
    DevBuf<uint8_t> mr_rgb; HostBuf<uint8_t> mr_host;
};

bool map_on(const nalo_ctx* c) { return c->map && c->map->on; }
void map_destroy(nalo_ctx* c) { delete c->map; c->map = nullptr; }

// room for positions [0, want): new chunks are new allocations; the table goes down again when one was added
static int map_reserve(nalo_ctx* c, MapArchive& m, long long want) {
    const size_t need = (size_t)((want + m.chunk - 1) / m.chunk);
    if (need <= m.chunks.size()) return NALO_OK;
    std::vector<DevBuf<nalo_map_record>> fresh(need - m.chunks.size());
    for (auto& b : fresh) NALO_HIP(c, b.reserve((size_t)m.chunk));          // a failure frees what this call allocated and leaves the archive as it was
    DevBuf<nalo_map_record*> tab;
    NALO_HIP(c, tab.reserve(need));
    std::vector<nalo_map_record*> ptrs;
    for (auto& b : m.chunks) ptrs.push_back(b.p);
    for (auto& b : fresh) ptrs.push_back(b.p);
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    NALO_HIP(c, hipMemcpy(tab.p, ptrs.data(), need * sizeof(nalo_map_record*), hipMemcpyHostToDevice));
    for (auto& b : fresh) m.chunks.push_back(std::move(b));
    m.tab = std::move(tab); m.tab_n = need;
    return NALO_OK;
}

int map_append_begin(nalo_ctx* c, MapAppendDev& A, int W, int ub) {
    MapArchive& m = *c->map;
    m.pending = false;
    A.nb = (A.P + 255) / 256;
    if (A.nb == 0) return NALO_OK;
    { int rc = map_reserve(c, m, m.filled + ub); if (rc) return rc; }
    NALO_HIP(c, m.cnt.reserve((size_t)A.nb + 1));
    if (!m.hs.p) {
        NALO_HIP(c, m.hs.reserve(4 * NALO_MAX_WINDOW)); NALO_HIP(c, m.hs_host.reserve(2 * NALO_MAX_WINDOW));
        NALO_HIP(c, hipMemsetAsync(m.hs.p, 0, 4 * NALO_MAX_WINDOW * 4, c->stream)); m.hs_buf = 0;
    }
    A.cnt = m.cnt.p; A.hs = m.hs.p + m.hs_buf * 2 * NALO_MAX_WINDOW; m.hs_buf ^= 1; A.hs_next = m.hs.p + m.hs_buf * 2 * NALO_MAX_WINDOW;
    A.chunks = m.tab.p; A.base = m.filled; A.cap = (long long)m.chunks.size() * m.chunk; A.chunk = m.chunk;
    { int rc = map_append_rank_launch(c, A); if (rc) return rc; }
    { int rc = map_append_write_launch(c, A, false); if (rc) return rc; }
    m.pend = A; m.pend_W = W; m.pending = true;
    return NALO_OK;
}
int map_append_patch(nalo_ctx* c) {
    MapArchive& m = *c->map;
    return m.pending ? map_append_write_launch(c, m.pend, true) : NALO_OK;
}
int map_append_fetch(nalo_ctx* c) {
    MapArchive& m = *c->map;
    if (m.pending) NALO_HIP(c, hipMemcpyAsync(m.hs_host.p, m.pend.hs, 2 * NALO_MAX_WINDOW * 4, hipMemcpyDeviceToHost, c->stream));
    return NALO_OK;
}
void map_append_commit(nalo_ctx* c) {
    MapArchive& m = *c->map;
    if (!m.pending) return;
    m.pending = false;
    for (int h = 0; h < m.pend_W; ++h) {
        const int n2 = m.hs_host.p[2 * h], n3 = m.hs_host.p[2 * h + 1];
        MapFrame& f = m.frames[m.pend.frame_id[h]];                          // a frame the archive has seen, with or without records
        f.cnt[0] += n2; f.cnt[1] += n3;
        for (int left = n2 + n3; left > 0;) {                                // a run that would straddle a chunk border is split here
            const int n = (int)std::min<long long>(left, m.chunk - m.filled % m.chunk);
            if (!f.runs.empty() && f.runs.back().off + f.runs.back().n == m.filled && m.filled % m.chunk != 0) f.runs.back().n += n;
            else f.runs.push_back({m.filled, n});
            m.filled += n; left -= n;
        }
    }
}

// the runs of a frame in an archive (MapArchive / DenseArchive: the same position -> chunk mapping) as segments of `kind` for listed frame `frame` behind `start`.
// start is 64 bits wide so that a caller can refuse a list an int cannot index; nothing is pushed past that point
template <typename Archive, typename Frame>
static void map_push_runs(const Archive& m, const Frame* f, int kind, std::vector<MapSeg>& segs, long long& start, int frame = 0) {
    if (!f) return;
    for (const MapRun& r : f->runs) {
        if (start <= INT32_MAX) segs.push_back({m.chunks[(size_t)(r.off / m.chunk)].p + r.off % m.chunk, (int)start, r.n, kind, frame});
        start += r.n;
    }
}
static int map_send_segs(nalo_ctx* c, MapArchive& m, const std::vector<MapSeg>& segs, int total, MapSrcDev& S) {
    const size_t n = std::max<size_t>(segs.size(), 1);
    NALO_HIP(c, m.seg_h.reserve(n)); NALO_HIP(c, m.seg_d.reserve(n));
    std::copy(segs.begin(), segs.end(), m.seg_h.p);
    if (!segs.empty()) NALO_HIP(c, hipMemcpyAsync(m.seg_d.p, m.seg_h.p, segs.size() * sizeof(MapSeg), hipMemcpyHostToDevice, c->stream));
    S.segs = m.seg_d.p; S.nseg = (int)segs.size(); S.total = total; S.nb = (total + 255) / 256;
    NALO_HIP(c, m.qcnt.reserve((size_t)S.nb + 1 + 8));
    S.cnt = m.qcnt.p;
    return NALO_OK;
}

// ---- the dense map: FrameHessian::mapPoints of every frame, 16-byte points in chunks of their own (the same position -> chunk mapping as the archive above).
// Per frame_id the host keeps the pieces (position, count) its points lie in, in append order, and the two totals.
struct DenseFrame { std::vector<MapRun> runs; long long points = 0; int n_runs = 0; };
struct DenseArchive {
    bool on = false;
    int chunk = 0;
    long long filled = 0;
    std::vector<DevBuf<nalo_dense_point>> chunks;
    DevBuf<nalo_dense_point*> tab;
    std::map<int, DenseFrame> frames;
    // the consumers: segment table, draws, block counts, outputs and their pinned mirrors
    HostBuf<MapSeg> seg_h; DevBuf<MapSeg> seg_d; HostBuf<int> draws_h; DevBuf<int> draws_d, cnt; HostBuf<int> cnt_h;
    DevBuf<double> wxyz; HostBuf<double> wxyz_h; DevBuf<float> cxyz; DevBuf<uint8_t> crgb; HostBuf<float> cxyz_h; HostBuf<uint8_t> crgb_h;
};

bool map_dense_on(const nalo_ctx* c) { return c->dmap && c->dmap->on; }
void map_dense_destroy(nalo_ctx* c) { delete c->dmap; c->dmap = nullptr; }

int map_dense_reserve(nalo_ctx* c, long long ub, DenseArchiveView* V) {
    DenseArchive& m = *c->dmap;
    const size_t need = (size_t)((m.filled + ub + m.chunk - 1) / m.chunk);
    if (need > m.chunks.size()) {
        std::vector<DevBuf<nalo_dense_point>> fresh(need - m.chunks.size());
        for (auto& b : fresh) NALO_HIP(c, b.reserve((size_t)m.chunk));      // a failure frees what this call allocated and leaves the archive as it was
        DevBuf<nalo_dense_point*> tab;
        NALO_HIP(c, tab.reserve(need));
        std::vector<nalo_dense_point*> ptrs;
        for (auto& b : m.chunks) ptrs.push_back(b.p);
        for (auto& b : fresh) ptrs.push_back(b.p);
        NALO_HIP(c, hipStreamSynchronize(c->stream));
        NALO_HIP(c, hipMemcpy(tab.p, ptrs.data(), need * sizeof(nalo_dense_point*), hipMemcpyHostToDevice));
        for (auto& b : fresh) m.chunks.push_back(std::move(b));
        m.tab = std::move(tab);
    }
    V->chunks = m.tab.p; V->base = m.filled; V->cap = (long long)m.chunks.size() * m.chunk; V->chunk = m.chunk;
    return NALO_OK;
}
long long map_dense_frame_points(nalo_ctx* c, int frame_id) {
    const auto it = c->dmap->frames.find(frame_id);
    return it == c->dmap->frames.end() ? 0 : it->second.points;
}
void map_dense_commit(nalo_ctx* c, int frame_id, int n_points, int n_runs) {
    DenseArchive& m = *c->dmap;
    DenseFrame& f = m.frames[frame_id];
    f.points += n_points; f.n_runs += n_runs;
    for (int left = n_points; left > 0;) {                                   // a piece never straddles a chunk border
        const int n = (int)std::min<long long>(left, m.chunk - m.filled % m.chunk);
        if (!f.runs.empty() && f.runs.back().off + f.runs.back().n == m.filled && m.filled % m.chunk != 0) f.runs.back().n += n;
        else f.runs.push_back({m.filled, n});
        m.filled += n; left -= n;
    }
}
// the frame of a consumer call, its pieces as segments on the device, the block counts
static int map_dense_frame(nalo_ctx* c, const char* who, int frame_id, DenseFrame** f) {
    const auto it = c->dmap ? c->dmap->frames.find(frame_id) : std::map<int, DenseFrame>::iterator();
    if (!c->dmap || it == c->dmap->frames.end()) return fail(c, NALO_ERR_ARG, std::string(who) + ": the dense archive has never seen this frame_id");
    *f = &it->second;
    return NALO_OK;
}
static int map_dense_send(nalo_ctx* c, DenseArchive& m, const DenseFrame& f, MapDenseDev& D) {
    const size_t n = std::max<size_t>(f.runs.size(), 1);
    NALO_HIP(c, m.seg_h.reserve(n)); NALO_HIP(c, m.seg_d.reserve(n));
    int start = 0, k = 0;
    for (const MapRun& r : f.runs) { m.seg_h.p[k++] = MapSeg{m.chunks[(size_t)(r.off / m.chunk)].p + r.off % m.chunk, start, r.n, 0, 0}; start += r.n; }
    if (k) NALO_HIP(c, hipMemcpyAsync(m.seg_d.p, m.seg_h.p, (size_t)k * sizeof(MapSeg), hipMemcpyHostToDevice, c->stream));
    D.segs = m.seg_d.p; D.nseg = k; D.total = start; D.nb = (start + 255) / 256;
    NALO_HIP(c, m.cnt.reserve((size_t)D.nb + 1));
    D.cnt = m.cnt.p;
    return NALO_OK;
}

int map_dense_segments(nalo_ctx* c, const char* who, int frame_id, std::vector<MapSeg>* segs, int* total) {
    if (!map_dense_on(c)) return fail(c, NALO_ERR_STATE, std::string(who) + ": the dense archive is not enabled (nalo_map_dense_enable)");
    MapWindowView V;
    if (c->ba && ba_map_view(c, -1, &V) == NALO_OK && V.sharded) return fail(c, NALO_ERR_STATE, std::string(who) + ": the window is sharded (a rank holds only its own points)");
    DenseFrame* f = nullptr;
    { int rc = map_dense_frame(c, who, frame_id, &f); if (rc) return rc; }
    // host code only: the archive's own staging table (map_dense_send) belongs to the calls that wait before they return
    const DenseArchive& m = *c->dmap;
    segs->clear();
    long long start = 0;
    for (const MapRun& r : f->runs) { segs->push_back(MapSeg{m.chunks[(size_t)(r.off / m.chunk)].p + r.off % m.chunk, (int)start, r.n, 0, 0}); start += r.n; }
    if (start > INT32_MAX) return fail(c, NALO_ERR_UNSUPPORTED, std::string(who) + ": the frame's dense list has more than 2^31 - 1 points");
    *total = (int)start;
    return NALO_OK;
}

// ---- the keyframe graph: EnergyFunctional::connectivityMap (EnergyFunctional.cpp:423, 453-458, 493, 628-634). The host keeps the keys and [1]; [0] is counted
// from the resident slots when the graph is read (ba_graph_view)
static uint64_t graph_key(int host_id, int target_id) { return ((uint64_t)host_id << 32) + (uint64_t)target_id; }
void graph_add_frames(nalo_ctx* c, int W, const int* ids) {
    for (int i = 0; i < W; ++i) for (int j = 0; j < W; ++j) c->graph_marg.emplace(graph_key(ids[i], ids[j]), 0);      // an existing entry keeps its count
}
void graph_add_marg(nalo_ctx* c, int W, const int* id_of_row, const double* misc) {
    for (int h = 0; h < W; ++h) for (int t = 0; t < W; ++t) {
        const int n = (int)(misc[2 * (h + t * W)] + 0.5);
        if (n > 0) c->graph_marg[graph_key(id_of_row[h], id_of_row[t])] += n;
    }
}
// every entry in key order with [0] from the window's count; NALO_ERR_STATE while off or without resident points
static int graph_entries(nalo_ctx* c, const char* who, std::vector<nalo_graph_edge>& E) {
    if (!c->graph_on) return fail(c, NALO_ERR_STATE, std::string(who) + ": the graph is off (nalo_map_graph_enable)");
    GraphWindowView V;
    { const int rc = ba_graph_view(c, true, &V); if (rc) return rc; }
    std::map<uint64_t, int> act;
    for (int i = 0; i < V.W; ++i) for (int j = 0; j < V.W; ++j) act[graph_key(V.ids[i], V.ids[j])] = V.act[i * NALO_MAX_WINDOW + j];
    E.clear(); E.reserve(c->graph_marg.size());
    for (const auto& kv : c->graph_marg) {
        const auto a = act.find(kv.first);
        E.push_back({(int)(kv.first >> 32), (int)(kv.first & 0xFFFFFFFFu), a == act.end() ? 0 : a->second, kv.second});
    }
    return NALO_OK;
}
// PangolinDSOViewer::publishGraph (PangolinDSOViewer.cpp:528-571): keys with host < target in key order, the backward pair from the inverse key
static int graph_connections(nalo_ctx* c, const char* who, std::vector<nalo_graph_connection>& C) {
    std::vector<nalo_graph_edge> E;
    { const int rc = graph_entries(c, who, E); if (rc) return rc; }
    std::map<uint64_t, const nalo_graph_edge*> by_key;
    for (const nalo_graph_edge& e : E) by_key[graph_key(e.host_id, e.target_id)] = &e;
    C.clear();
    for (const nalo_graph_edge& e : E) {
        if (e.host_id >= e.target_id) continue;
        const auto inv = by_key.find(graph_key(e.target_id, e.host_id));
        const nalo_graph_edge* b = inv == by_key.end() ? nullptr : inv->second;      // (pairs are created in both directions: the reference's .at() never throws)
        C.push_back({e.host_id, e.target_id, e.act, b ? b->act : 0, e.marg, b ? b->marg : 0});
    }
    return NALO_OK;
}

}  // namespace nalo

using namespace nalo;

extern "C" {

int nalo_map_enable(nalo_ctx* c, int on, int chunk_points) {
    if (!c) return NALO_ERR_ARG;
    if (chunk_points < 0) return fail(c, NALO_ERR_ARG, "nalo_map_enable: chunk_points must not be negative");
    if (on) {
        if (c->xchg_failed) return fail(c, NALO_ERR_STATE, "nalo_map_enable: a cross-rank sum of this context failed earlier");
        MapWindowView V;
        if (c->ba && ba_map_view(c, -1, &V) == NALO_OK && V.sharded) return fail(c, NALO_ERR_STATE, "nalo_map_enable: the window is sharded (a rank holds only its own points)");
    }
    if (!c->map) { if (!on) return NALO_OK; c->map = new MapArchive(); }
    MapArchive& m = *c->map;
    if (on && m.chunks.empty()) m.chunk = chunk_points > 0 ? chunk_points : 65536;
    m.on = on != 0;
    return NALO_OK;
}

int nalo_map_reset(nalo_ctx* c) {
    if (!c) return NALO_ERR_ARG;
    if (c->dmap) { c->dmap->frames.clear(); c->dmap->filled = 0; }
    if (c->graph_on) {                                                      // an EnergyFunctional that has just inserted the window's frames
        c->graph_marg.clear();
        GraphWindowView V;
        if (ba_graph_view(c, false, &V) == NALO_OK) graph_add_frames(c, V.W, V.ids);
    }
    if (!c->map) return NALO_OK;
    c->map->frames.clear(); c->map->filled = 0; c->map->pending = false;
    return NALO_OK;
}

int nalo_map_counts(nalo_ctx* c, int frame_id, int counts[2]) {
    if (!c || !counts) return fail(c, NALO_ERR_ARG, "nalo_map_counts: bad argument");
    const auto it = c->map ? c->map->frames.find(frame_id) : std::map<int, MapFrame>::iterator();
    if (!c->map || it == c->map->frames.end()) return fail(c, NALO_ERR_ARG, "nalo_map_counts: the archive has never seen this frame_id");
    counts[0] = it->second.cnt[0]; counts[1] = it->second.cnt[1];
    return NALO_OK;
}

int nalo_map_get_frame(nalo_ctx* c, int frame_id, nalo_map_record* records, int cap, int* n) {
    if (!c || !n || cap < 0) return fail(c, NALO_ERR_ARG, "nalo_map_get_frame: bad argument");
    const auto it = c->map ? c->map->frames.find(frame_id) : std::map<int, MapFrame>::iterator();
    if (!c->map || it == c->map->frames.end()) return fail(c, NALO_ERR_ARG, "nalo_map_get_frame: the archive has never seen this frame_id");
    MapArchive& m = *c->map;
    const MapFrame& f = it->second;
    *n = f.cnt[0] + f.cnt[1];
    if (cap < *n || (*n > 0 && !records)) return fail(c, NALO_ERR_ARG, "nalo_map_get_frame: cap is smaller than the frame's record count");
    if (*n == 0) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<nalo_map_record> all((size_t)*n);
    size_t at = 0;
    for (const MapRun& r : f.runs) {
        NALO_HIP(c, hipMemcpy(all.data() + at, m.chunks[(size_t)(r.off / m.chunk)].p + r.off % m.chunk, (size_t)r.n * sizeof(nalo_map_record), hipMemcpyDeviceToHost));
        at += (size_t)r.n;
    }
    size_t o = 0;
    for (int st = 2; st <= 3; ++st) for (const nalo_map_record& r : all) if (r.status == st) records[o++] = r;
    return NALO_OK;
}

int nalo_map_world_points(nalo_ctx* c, int frame_id, const double camToWorld[12], double* xyz, int cap, int* n) {
    if (!c || !camToWorld || !n || cap < 0) return fail(c, NALO_ERR_ARG, "nalo_map_world_points: bad argument");
    const auto it = c->map ? c->map->frames.find(frame_id) : std::map<int, MapFrame>::iterator();
    if (!c->map || it == c->map->frames.end()) return fail(c, NALO_ERR_ARG, "nalo_map_world_points: the archive has never seen this frame_id");
    MapArchive& m = *c->map;
    *n = it->second.cnt[0];
    if (cap < *n || (*n > 0 && !xyz)) return fail(c, NALO_ERR_ARG, "nalo_map_world_points: cap is smaller than the frame's marginalised points");
    if (*n == 0) return NALO_OK;
    MapWindowView V;
    { int rc = ba_map_view(c, frame_id, &V); if (rc) return rc; }
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "map_world_points");
    std::vector<MapSeg> segs; long long total = 0;
    map_push_runs(m, &it->second, 2, segs, total);
    MapWorldDev D{};
    { int rc = map_send_segs(c, m, segs, (int)total, D.S); if (rc) return rc; }
    NALO_HIP(c, m.wxyz.reserve(3 * (size_t)*n)); NALO_HIP(c, m.wxyz_h.reserve(3 * (size_t)*n));
    std::memcpy(D.ci, V.ci, sizeof(D.ci)); std::memcpy(D.m, camToWorld, sizeof(D.m)); D.xyz = m.wxyz.p; D.cap = *n;
    { int rc = map_world_launch(c, D); if (rc) return rc; }
    NALO_HIP(c, hipMemcpyAsync(m.wxyz_h.p, m.wxyz.p, 3 * (size_t)*n * 8, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(xyz, m.wxyz_h.p, 3 * (size_t)*n * 8);
    return NALO_OK;
}

int nalo_map_world_points_host(int n, const float* u, const float* v, const float* idepth, const float calib_inv[4], const double m[12], double* xyz) {
    if (n < 0 || !calib_inv || !m || (n > 0 && (!u || !v || !idepth || !xyz))) return NALO_ERR_ARG;
    for (int i = 0; i < n; ++i) map_world_point(u[i], v[i], idepth[i], calib_inv, m, xyz + 3 * i);
    return NALO_OK;
}

int nalo_map_frame_cloud(nalo_ctx* c, nalo_map_cloud_args* a) {
    if (!c || !a) return fail(c, NALO_ERR_ARG, "nalo_map_frame_cloud: bad argument");
    a->n = 0; a->n_needed = 0;
    for (int i = 0; i < 4; ++i) a->records[i] = a->survivors[i] = 0;
    if (a->sparsity > 1) return fail(c, NALO_ERR_ARG, "nalo_map_frame_cloud: sparsity > 1 is not supported (rand() % factor makes every later draw index depend on earlier draws)");
    if (a->cap < 0 || a->n_draws < 0) return fail(c, NALO_ERR_ARG, "nalo_map_frame_cloud: bad argument");
    MapWindowView V;
    { int rc = ba_map_view(c, a->frame_id, &V); if (rc) return rc; }
    const MapFrame* f = nullptr;
    if (c->map) { const auto it = c->map->frames.find(a->frame_id); if (it != c->map->frames.end()) f = &it->second; }
    if (V.widx < 0 && !f) return fail(c, NALO_ERR_ARG, "nalo_map_frame_cloud: frame_id is neither in the window nor in the archive");
    if (V.widx >= 0 && !V.pts_ok) return fail(c, NALO_ERR_STATE, "nalo_map_frame_cloud: the frame is in the window but the window's points are unset (or sharded): carry or re-issue the window first");
    if (!c->map) c->map = new MapArchive();                                 // the clouds' scratch lives there (the archive stays off)
    MapArchive& m = *c->map;
    // the record list, counted from the host's mirrors
    int n_imm = 0;
    const bool imm = a->with_immature && V.widx >= 0 && c->imm_res_n > 0;
    if (imm) for (int i = 0; i < c->imm_res_n && i < (int)c->imm_host_h.size(); ++i) n_imm += c->imm_host_h[i] == V.widx;
    const int records = n_imm + (V.widx >= 0 ? V.n_valid : 0) + (f ? f->cnt[0] + f->cnt[1] : 0);
    a->n_needed = 8 * records;
    if (a->cap < a->n_needed || (a->draws && a->n_draws < a->n_needed)) return fail(c, NALO_ERR_ARG, "nalo_map_frame_cloud: cap / n_draws below 8 x the frame's records (n_needed)");
    if (records > 0 && (!a->xyz || !a->rgb)) return fail(c, NALO_ERR_ARG, "nalo_map_frame_cloud: xyz and rgb required");
    if (records == 0) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "map_frame_cloud");
    std::vector<MapSeg> segs; long long total = 0;
    if (imm && n_imm) { segs.push_back({nullptr, (int)total, c->imm_res_n, 0, 0}); total += c->imm_res_n; }
    if (V.widx >= 0 && V.seg) { segs.push_back({V.kmap, (int)total, V.seg, 1, 0}); total += V.seg; }
    map_push_runs(m, f, 2, segs, total);
    map_push_runs(m, f, 3, segs, total);
    MapCloudDev D{};
    { int rc = map_send_segs(c, m, segs, (int)total, D.S); if (rc) return rc; }
    D.S.imm = c->imm_res.p; D.S.immN = c->imm_res_n;
    for (int i = 0; i < NALO_MAX_WINDOW; ++i) D.S.imm_frame[i] = i == V.widx ? 0 : -1;
    D.S.flags = V.flags; D.S.geo = V.geo; D.S.col0 = V.col0; D.S.col1 = V.col1; D.S.acc = V.acc; D.S.prior = V.prior; D.S.relbs = V.relbs;
    D.mode = a->display_mode; D.scaledTH = a->scaledTH; D.absTH = a->absTH; D.minRelBS = a->minRelBS; std::memcpy(D.ci, V.ci, sizeof(D.ci));
    const size_t nv = (size_t)a->n_needed;
    NALO_HIP(c, m.cxyz.reserve(3 * nv)); NALO_HIP(c, m.crgb.reserve(3 * nv)); NALO_HIP(c, m.cxyz_h.reserve(3 * nv)); NALO_HIP(c, m.crgb_h.reserve(3 * nv)); NALO_HIP(c, m.stats_h.reserve(9));
    D.xyz = m.cxyz.p; D.rgb = m.crgb.p; D.cap = records; D.stats = D.S.cnt + D.S.nb + 1;
    NALO_HIP(c, hipMemsetAsync(D.stats, 0, 8 * 4, c->stream));
    if (a->draws) {
        NALO_HIP(c, m.draws_h.reserve(nv)); NALO_HIP(c, m.draws_d.reserve(nv));
        std::memcpy(m.draws_h.p, a->draws, nv * 4);
        NALO_HIP(c, hipMemcpyAsync(m.draws_d.p, m.draws_h.p, nv * 4, hipMemcpyHostToDevice, c->stream));
        D.draws = m.draws_d.p;
    }
    { int rc = map_cloud_launch(c, D); if (rc) return rc; }
    // the vertex count is known only behind the scan: everything the call may have written comes up in the one wait
    NALO_HIP(c, hipMemcpyAsync(m.stats_h.p, D.S.cnt + D.S.nb, 9 * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(m.cxyz_h.p, m.cxyz.p, 3 * nv * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(m.crgb_h.p, m.crgb.p, 3 * nv, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const int ns = m.stats_h.p[0];
    for (int i = 0; i < 4; ++i) { a->records[i] = m.stats_h.p[1 + i]; a->survivors[i] = m.stats_h.p[5 + i]; }
    if (ns < 0 || 8 * (size_t)ns > nv) return fail(c, NALO_ERR_HIP, "nalo_map_frame_cloud: the device counted more survivors than the frame has records");
    a->n = 8 * ns;
    std::memcpy(a->xyz, m.cxyz_h.p, 3 * (size_t)a->n * 4); std::memcpy(a->rgb, m.crgb_h.p, 3 * (size_t)a->n);
    return NALO_OK;
}

// FullSystem::debugPlot (FullSystemDebugStuff.cpp:109-358) for the frames of the window (kernels_window_plot.hip). Everything is enqueued on the main stream; results,
// counters and images come up through one pinned block behind ONE wait and reach the caller only when the call succeeds.
int nalo_map_window_plot(nalo_ctx* c, nalo_window_plot_args* a) {
    if (!c || !a || !a->bgr) return fail(c, NALO_ERR_ARG, "nalo_map_window_plot: bad argument");
    if (a->mode < 0 || a->mode > 9) return fail(c, NALO_ERR_ARG, "nalo_map_window_plot: mode outside 0..9");
    if (!std::isfinite(a->rainbow_scale) || !std::isfinite(a->quality_scale)) return fail(c, NALO_ERR_ARG, "nalo_map_window_plot: rainbow_scale / quality_scale must be finite");
    if (a->mode == 6) return fail(c, NALO_ERR_UNSUPPORTED, "nalo_map_window_plot: mode 6 paints PointHessian::my_type, which is not part of the resident window");
    if (c->xchg_failed) return fail(c, NALO_ERR_HIP, "nalo_map_window_plot: a cross-rank sum of this context failed earlier; rebuild on a new context");
    if (!c->ba) return fail(c, NALO_ERR_STATE, "nalo_map_window_plot: no window");
    NALO_HIP(c, hipSetDevice(c->device));
    PlotWindowView V;
    { const int rc = ba_plot_view(c, &V); if (rc) return rc; }
    if (a->frame_mask >> V.W) return fail(c, NALO_ERR_ARG, "nalo_map_window_plot: frame_mask names a frame outside the window");
    if (V.sharded) return fail(c, NALO_ERR_STATE, "nalo_map_window_plot: the window is sharded (a rank holds only its own points)");
    if (!V.pts_ok) return fail(c, NALO_ERR_STATE, "nalo_map_window_plot: the window's points are unset: carry or re-issue the window first");
    WindowPlotDev D{};
    int frame_of[NALO_MAX_WINDOW];
    { const int rc = ba_plot_frames(c, "nalo_map_window_plot", V, a->frame_mask, D.out_of, frame_of, D.I, &D.n_frames); if (rc) return rc; }
    HostTimer ht(c, "map_window_plot");
    // the sources: a painted frame's sublist in painting order. Mode 7 lists every frame (allID does not know the mask)
    const MapArchive* const arch = c->map;
    const int mode = a->mode;
    std::vector<PlotSeg> segs; long long total = 0;
    if (mode == 3 || mode == 4 || mode == 5) {
        if (c->imm_res_n > 0 && c->imm_res.p) { segs.push_back({nullptr, 0, c->imm_res_n, 0, 0, 0, 0}); total = c->imm_res_n; }
    } else if (mode == 0 || mode == 1 || mode == 7) {
        for (int i = 0; i < V.W; ++i) {
            if (D.out_of[i] < 0 && mode != 7) continue;
            const long long fstart = total;
            if (D.out_of[i] >= 0) D.fstart[D.out_of[i]] = (int)std::min<long long>(fstart, INT32_MAX);
            if (V.seg[i]) { segs.push_back({V.kmap[i], (int)total, V.seg[i], 1, i, (int)fstart, 0}); total += V.seg[i]; }
            const MapFrame* f = nullptr;
            if (arch) { const auto it = arch->frames.find(V.frame_id[i]); if (it != arch->frames.end()) f = &it->second; }
            for (int kind = 2; f && kind <= 3 && total <= INT32_MAX; ++kind)
                for (const MapRun& r : f->runs) {
                    if (total > INT32_MAX) break;
                    segs.push_back({arch->chunks[(size_t)(r.off / arch->chunk)].p + r.off % arch->chunk, (int)total, r.n, kind, i, (int)fstart, 0});
                    total += r.n;
                }
            if (total > INT32_MAX) return fail(c, NALO_ERR_UNSUPPORTED, "nalo_map_window_plot: more sources than the key can index");
        }
    }
    if (!c->map) c->map = new MapArchive();                                 // the call's scratch lives there (the archive stays off)
    MapArchive& m = *c->map;
    const size_t npx = (size_t)c->w * c->h, px = npx * (size_t)D.n_frames, padded = resolve_padded_pixels(px);
    const size_t nseg = std::max<size_t>(segs.size(), 1), off_cnt = 64, off_bgr = 512;
    constexpr int kCnt = 4 * NALO_MAX_WINDOW;
    NALO_HIP(c, m.wp_seg_h.reserve(nseg)); NALO_HIP(c, m.wp_seg_d.reserve(nseg)); NALO_HIP(c, m.wp_col.reserve(std::max<size_t>((size_t)total, 1)));
    NALO_HIP(c, m.wp_bgr.reserve(3 * padded)); NALO_HIP(c, m.wp_res.reserve(kPlotResWords)); NALO_HIP(c, m.wp_host.reserve(off_bgr + 3 * px));
    bool refilled = false;
    NALO_HIP(c, m.wp_cnt.reserve(2 * kCnt)); NALO_HIP(c, m.wp_key.begin(padded, c->stream, &refilled));
    if (refilled) { NALO_HIP(c, hipMemsetAsync(m.wp_cnt.p, 0, 2 * kCnt * 4, c->stream)); m.wp_cnt_buf = 0; }   // the counters are idle exactly when the plane is
    std::copy(segs.begin(), segs.end(), m.wp_seg_h.p);
    if (!segs.empty()) NALO_HIP(c, hipMemcpyAsync(m.wp_seg_d.p, m.wp_seg_h.p, segs.size() * sizeof(PlotSeg), hipMemcpyHostToDevice, c->stream));
    D.segs = m.wp_seg_d.p; D.nseg = (int)segs.size(); D.total = (int)total;
    D.mode = mode; D.w = c->w; D.h = c->h; D.rainbow_scale = a->rainbow_scale; D.quality_scale = a->quality_scale;
    D.imm = c->imm_res.p; D.immN = c->imm_res_n; D.flags = V.flags; D.geo = V.geo;
    D.key = m.wp_key.p; D.col = m.wp_col.p; D.bgr = m.wp_bgr.p; D.res = m.wp_res.p;
    D.cnt = m.wp_cnt.p + m.wp_cnt_buf * kCnt; m.wp_cnt_buf ^= 1; D.cnt_next = m.wp_cnt.p + m.wp_cnt_buf * kCnt;
    const bool io = mode == 7 && a->minmax_io != nullptr;
    D.io_min = io ? a->minmax_io[0] : 0.f; D.io_max = io ? a->minmax_io[1] : 0.f; D.have_io = io ? 1 : 0;
    { const int rc = window_plot_launch(c, D); if (rc) return rc; }
    m.wp_key.settled();
    if (mode == 7) NALO_HIP(c, hipMemcpyAsync(m.wp_host.p, m.wp_res.p, kPlotResWords * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(m.wp_host.p + off_cnt, D.cnt, kCnt * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(m.wp_host.p + off_bgr, m.wp_bgr.p, 3 * px, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    unsigned res[kPlotResWords] = {};
    if (mode == 7) {
        std::memcpy(res, m.wp_host.p, sizeof(res));
        if (res[0] == 0) { a->n_values = 0; return fail(c, NALO_ERR_STATE, "nalo_map_window_plot: mode 7 and the window holds no point with an inverse depth"); }   // the reference indexes an empty vector here
        if (io) std::memcpy(a->minmax_io, &res[5], 8);
    }
    a->n_values = (int)res[0];
    std::memcpy(&a->min_new, &res[1], 4); std::memcpy(&a->max_new, &res[2], 4); std::memcpy(&a->min_used, &res[3], 4); std::memcpy(&a->max_used, &res[4], 4);
    a->n_frames = D.n_frames;
    int cnt[kCnt];
    std::memcpy(cnt, m.wp_host.p + off_cnt, sizeof(cnt));
    for (int i = 0; i < NALO_MAX_WINDOW; ++i) { a->frame_id[i] = 0; for (int k = 0; k < 4; ++k) a->sources[i][k] = 0; }
    for (int j = 0; j < D.n_frames; ++j) {
        a->frame_id[j] = V.frame_id[frame_of[j]];
        for (int k = 0; k < 4; ++k) a->sources[j][k] = cnt[4 * j + k];
    }
    std::memcpy(a->bgr, m.wp_host.p + off_bgr, 3 * px);
    return NALO_OK;
}

// The 3-D panel of PangolinDSOViewer (kernels_map_render.hip; the definition: include/nalo_gpu.h). Every check stands before the first enqueue; kernels on the main
// stream; counters and images come up through one pinned block behind ONE wait (the graph's count, when a constraint flag is set, is nalo_map_graph's own) and
// reach the caller only when the call succeeds.
//
// nalo_map_render_mesh is the same call with the triangles of up to three meshes entered into the key plane between the lines and the resolve pass (mesh != NULL;
// kernels_map_render_mesh.hip). Its own refusals stand with the others, before the first enqueue; a window is needed only for what reads one.
static int map_render_impl(nalo_ctx* c, nalo_map_render_args* a, nalo_map_render_mesh_args* mesh, const char* who) {
    if (mesh) mesh->n_triangles = mesh->n_tri_bad_index = mesh->n_tri_near = mesh->n_tri_guard = mesh->n_tri_degenerate = mesh->n_tri_large = mesh->n_tri_pixels = 0;
    if (a && mesh) a->n_vertices = a->n_drawn_points = a->n_segments = a->n_line_samples = 0;     // every refusal of the mesh call zeroes all eleven counts
    if (!c || !a || !a->rgb) return fail(c, NALO_ERR_ARG, std::string(who) + "bad argument");
    a->n_vertices = a->n_drawn_points = a->n_segments = a->n_line_samples = 0;
    if (mesh) {
        if (a->vw > kMrMaxView || a->vh > kMrMaxView) return fail(c, NALO_ERR_ARG, std::string(who) + "vw and vh must be at most 65536");
        if (mesh->colour_mode < 0 || mesh->colour_mode > 1) return fail(c, NALO_ERR_ARG, std::string(who) + "colour_mode must be 0 or 1");
        if (mesh->max_box_pixels < 0) return fail(c, NALO_ERR_ARG, std::string(who) + "max_box_pixels is negative");
        if (const nalo_render_mesh_src* u = mesh->user) {
            if (u->n_vertices < 0 || u->n_triangles < 0 || u->n_vertices > INT32_MAX || u->n_triangles > INT32_MAX) return fail(c, NALO_ERR_ARG, std::string(who) + "a count of the user mesh is negative or above 2^31 - 1");
            if ((u->n_vertices > 0 && !u->xyz) || (u->n_triangles > 0 && !u->tri)) return fail(c, NALO_ERR_ARG, std::string(who) + "an array of the user mesh is NULL with a positive count");
        }
    }
    if (a->vw < 1 || a->vh < 1 || (long long)a->vw * a->vh > (1ll << 26)) return fail(c, NALO_ERR_ARG, std::string(who) + "vw, vh must be at least 1 and vw * vh at most 2^26");
    for (float f : {a->fx, a->fy, a->cx, a->cy, a->znear, a->zfar}) if (!std::isfinite(f)) return fail(c, NALO_ERR_ARG, std::string(who) + "the camera values must be finite");
    for (double d : a->viewFromWorld) if (!std::isfinite(d)) return fail(c, NALO_ERR_ARG, std::string(who) + "viewFromWorld must be finite");
    if (a->znear <= 0 || a->zfar <= a->znear) return fail(c, NALO_ERR_ARG, std::string(who) + "0 < znear < zfar required");
    if (a->n_frames < 0 || (a->n_frames > 0 && !a->frames)) return fail(c, NALO_ERR_ARG, std::string(who) + "n_frames is negative, or frames is NULL");
    if (a->n_all_poses < 0 || (a->n_all_poses > 0 && !a->all_poses)) return fail(c, NALO_ERR_ARG, std::string(who) + "n_all_poses is negative, or all_poses is NULL");
    if (a->sparsity > 1) return fail(c, NALO_ERR_ARG, std::string(who) + "sparsity > 1 is not supported (as nalo_map_frame_cloud)");
    std::map<int, int> index_of;
    for (int i = 0; i < a->n_frames; ++i) if (!index_of.emplace(a->frames[i].frame_id, i).second) return fail(c, NALO_ERR_ARG, std::string(who) + "a frame_id is listed twice");
    if (c->xchg_failed) return fail(c, NALO_ERR_STATE, std::string(who) + "a cross-rank sum of this context failed earlier; rebuild on a new context");
    if (a->with_dense && !map_dense_on(c)) return fail(c, NALO_ERR_STATE, std::string(who) + "with_dense and the dense archive is off (nalo_map_dense_enable)");
    const bool constraints = a->show_active_constraints || a->show_all_constraints;
    if (constraints && !c->graph_on) return fail(c, NALO_ERR_STATE, std::string(who) + "a constraint flag is set and the graph is off (nalo_map_graph_enable)");
    MapWindowView V0;
    if (!mesh || a->n_frames > 0 || a->show_kf_cams || a->show_current_cam) { const int rc = ba_map_view(c, -1, &V0); if (rc) return rc; }
    else {                                                                      // a mesh call that reads no window: a context with only a volume can draw its mesh
        const std::string err = c->err;
        if (ba_map_view(c, -1, &V0) != NALO_OK) { V0 = MapWindowView{}; c->err = err; }
    }
    if (V0.sharded) return fail(c, NALO_ERR_STATE, std::string(who) + "the window is sharded (a rank holds only its own points)");
    NALO_HIP(c, hipSetDevice(c->device));
    // the record list of all listed frames: per frame what nalo_map_frame_cloud lists, then its dense pieces
    const MapArchive* const arch = c->map;
    const DenseArchive* const dense = a->with_dense ? c->dmap : nullptr;
    std::vector<MapSeg> segs; long long total = 0;
    MapWindowView VW{}; bool have_window = false;
    int imm_frame[NALO_MAX_WINDOW];
    for (int& v : imm_frame) v = -1;
    const bool imm = a->with_immature && c->imm_res_n > 0 && c->imm_res.p;
    if (imm) { segs.push_back({nullptr, 0, c->imm_res_n, 0, 0}); total = c->imm_res_n; }      // the resident set once for all frames: imm_frame names a point's frame
    for (int i = 0; i < a->n_frames; ++i) {
        const int fid = a->frames[i].frame_id;
        MapWindowView V;
        { const int rc = ba_map_view(c, fid, &V); if (rc) return rc; }
        const MapFrame* f = nullptr;
        if (arch) { const auto it = arch->frames.find(fid); if (it != arch->frames.end()) f = &it->second; }
        const DenseFrame* df = nullptr;
        if (c->dmap) { const auto it = c->dmap->frames.find(fid); if (it != c->dmap->frames.end()) df = &it->second; }
        if (V.widx < 0 && !f && !df) return fail(c, NALO_ERR_ARG, std::string(who) + "a frame_id is neither in the window nor in either archive");
        if (V.widx >= 0 && !V.pts_ok) return fail(c, NALO_ERR_STATE, std::string(who) + "a listed frame is in the window but the window's points are unset: carry or re-issue the window first");
        if (V.widx >= 0) { VW = V; have_window = true; if (V.widx < NALO_MAX_WINDOW) imm_frame[V.widx] = i; }
        if (V.widx >= 0 && V.seg) { segs.push_back({V.kmap, (int)total, V.seg, 1, i}); total += V.seg; }
        if (f) { map_push_runs(*arch, f, 2, segs, total, i); map_push_runs(*arch, f, 3, segs, total, i); }
        if (dense && df) map_push_runs(*dense, df, 4, segs, total, i);
        if (total > INT32_MAX) return fail(c, NALO_ERR_UNSUPPORTED, std::string(who) + "more records than a 32-bit index can hold");
    }
    // the mesh sources in the order archive, live mesh, user: the views are host code and launch nothing
    MrTrisDev T{};
    hipStream_t user_stream = nullptr; bool user_wait = false;
    long long n_triangles = 0;                                                   // reaches the caller with the other counts, behind the wait
    if (mesh) {
        auto add_src = [&](const float* xyz, const int* tri, const uint8_t* rgba, long long nv, long long nt) {
            n_triangles += nt;
            if (nt > 0) T.src[T.n_src++] = MrTriSrc{xyz, tri, mesh->colour_mode == 0 ? rgba : nullptr, (int)nv, (int)nt};
        };
        const std::string no_colour = "colour_mode 0 and a selected source has no colours: ";
        if (mesh->with_archive) {
            nalo_tsdf_archive_dev v;
            if (nalo_tsdf_archive_view(c, &v) != NALO_OK) return fail(c, NALO_ERR_STATE, std::string(who) + "with_archive and the mesh archive is not enabled (nalo_tsdf_archive_enable)");
            if (mesh->colour_mode == 0 && !v.rgba) return fail(c, NALO_ERR_STATE, std::string(who) + no_colour + "the archive is uncoloured");
            add_src(v.xyz, v.tri, v.rgba, v.n_vertices, v.n_triangles);
        }
        if (mesh->with_live_mesh) {
            nalo_tsdf_mesh_dev v; nalo_tsdf_mesh_color_dev vc{};
            if (!c->tsdf || nalo_tsdf_mesh_view(c, &v) != NALO_OK) return fail(c, NALO_ERR_STATE, std::string(who) + "with_live_mesh before any mesh call (nalo_tsdf_mesh, nalo_tsdf_mesh_color)");
            if (mesh->colour_mode == 0 && nalo_tsdf_mesh_color_view(c, &vc) != NALO_OK) return fail(c, NALO_ERR_STATE, std::string(who) + no_colour + "the live mesh was left by the plain nalo_tsdf_mesh");
            add_src(v.xyz, v.tri, vc.rgba, v.n_vertices, v.n_triangles);
        }
        if (const nalo_render_mesh_src* u = mesh->user) {
            if (mesh->colour_mode == 0 && !u->rgba && u->n_vertices > 0) return fail(c, NALO_ERR_STATE, std::string(who) + no_colour + "the user mesh's rgba is NULL");
            add_src(u->xyz, u->tri, u->rgba, u->n_vertices, u->n_triangles);
            user_stream = (hipStream_t)u->producer_stream; user_wait = u->n_triangles > 0 && user_stream != (hipStream_t)c->stream;
        }
        for (int s = 0; s < T.n_src; ++s) T.blk0[s + 1] = T.blk0[s] + (unsigned)(((long long)T.src[s].nt + 255) / 256);
        for (int i = 0; i < 12; ++i) T.V[i] = (float)a->viewFromWorld[i];
        T.colour_mode = mesh->colour_mode; T.max_box = mesh->max_box_pixels == 0 ? kMrDefaultBox : mesh->max_box_pixels;
    }
    std::vector<nalo_graph_connection> conn;
    if (constraints) { const int rc = graph_connections(c, "nalo_map_render", conn); if (rc) return rc; }
    HostTimer ht(c, "map_render");
    // ---- the transforms and the segment list
    const MrCam cam{a->vw, a->vh, a->fx, a->fy, a->cx, a->cy, a->znear, a->zfar};
    std::vector<float> M(12 * (size_t)std::max(a->n_frames, 1), 0.f);
    for (int i = 0; i < a->n_frames; ++i) map_render_transform(a->viewFromWorld, a->frames[i].camToWorld, &M[12 * (size_t)i]);
    float Vf[12];
    for (int i = 0; i < 12; ++i) Vf[i] = (float)a->viewFromWorld[i];
    std::vector<MrLine> lines;
    long long n_segments = 0;                                                  // reaches the caller with the other counts, behind the wait
    auto add = [&](const float* Mx, const float p[3], const float q[3], unsigned col, int width) {
        float pa[3], pb[3];
        map_render_apply(Mx, p, pa); map_render_apply(Mx, q, pb);
        MrLine L;
        if (map_render_line(cam, pa, pb, col, width, &L)) { ++n_segments; if (L.count > 0) lines.push_back(L); }
    };
    auto cam_lines = [&](const float* Mx, float sz, unsigned col, int width) {       // drawCam :630-649
        float p[5][3];
        map_render_frustum(V0.cf, c->w, c->h, sz, p);
        constexpr int e[8][2] = {{0, 1}, {0, 2}, {0, 3}, {0, 4}, {4, 3}, {3, 2}, {2, 1}, {1, 4}};
        for (const auto& s : e) add(Mx, p[s[0]], p[s[1]], col, width);
    };
    auto translation = [&](int i, float t[3]) { for (int k = 0; k < 3; ++k) t[k] = (float)a->frames[i].camToWorld[4 * k + 3]; };
    constexpr unsigned kRed = 0xFF0000u, kGreen = 0x00FF00u, kBlue = 0x0000FFu;
    if (a->show_kf_cams) for (int i = 0; i < a->n_frames; ++i) cam_lines(&M[12 * (size_t)i], 0.1f, kBlue, 1);
    if (a->show_current_cam) {
        float Mc[12];
        map_render_transform(a->viewFromWorld, a->currentCamToWorld, Mc);
        cam_lines(Mc, 0.2f, kRed, 2);
    }
    for (const nalo_graph_connection& g : conn) {                                  // drawConstraints :448-493; an unlisted end is the reference's `== 0`
        const auto from = index_of.find(g.from_id), to = index_of.find(g.to_id);
        if (from == index_of.end() || to == index_of.end()) continue;
        const int nAct = g.bwdAct + g.fwdAct, nMarg = g.bwdMarg + g.fwdMarg;
        float p[3], q[3];
        translation(from->second, p); translation(to->second, q);
        if (a->show_all_constraints && nAct == 0 && nMarg > 0) add(Vf, p, q, kGreen, 1);
        if (a->show_active_constraints && nAct > 0) add(Vf, p, q, kBlue, 3);
    }
    if (a->show_trajectory) for (int i = 0; i + 1 < a->n_frames; ++i) { float p[3], q[3]; translation(i, p); translation(i + 1, q); add(Vf, p, q, kRed, 3); }
    if (a->show_full_trajectory) for (int i = 0; i + 1 < a->n_all_poses; ++i) add(Vf, a->all_poses + 3 * (size_t)i, a->all_poses + 3 * (size_t)(i + 1), kGreen, 3);
    // ---- the device side
    if (!c->map) c->map = new MapArchive();                                 // the call's scratch lives there (the archive stays off)
    MapArchive& m = *c->map;
    MapRenderDev D{};
    { const int rc = map_send_segs(c, m, segs, (int)total, D.S); if (rc) return rc; }
    D.S.imm = c->imm_res.p; D.S.immN = c->imm_res_n; std::memcpy(D.S.imm_frame, imm_frame, sizeof(imm_frame));
    if (have_window) { D.S.flags = VW.flags; D.S.geo = VW.geo; D.S.col0 = VW.col0; D.S.col1 = VW.col1; D.S.acc = VW.acc; D.S.prior = VW.prior; D.S.relbs = VW.relbs; }
    const size_t npx = (size_t)a->vw * a->vh, padded = resolve_padded_pixels(npx), off_rgb = 128, off_depth = (off_rgb + 3 * npx + 15) / 16 * 16;
    NALO_HIP(c, m.mr_M_h.reserve(M.size())); NALO_HIP(c, m.mr_M_d.reserve(M.size()));
    NALO_HIP(c, m.mr_lines_h.reserve(std::max<size_t>(lines.size(), 1))); NALO_HIP(c, m.mr_lines_d.reserve(std::max<size_t>(lines.size(), 1)));
    NALO_HIP(c, m.mr_rgb.reserve(3 * padded)); NALO_HIP(c, m.mr_depth.reserve(padded)); NALO_HIP(c, m.mr_host.reserve(off_depth + 4 * npx));
    bool refilled = false;
    NALO_HIP(c, m.mr_cnt.reserve(2 * kMrCounters)); NALO_HIP(c, m.mr_key.begin(padded, c->stream, &refilled));
    if (refilled) { NALO_HIP(c, hipMemsetAsync(m.mr_cnt.p, 0, 2 * kMrCounters * 8, c->stream)); m.mr_cnt_buf = 0; }   // the counters are idle exactly when the plane is
    std::copy(M.begin(), M.end(), m.mr_M_h.p);
    NALO_HIP(c, hipMemcpyAsync(m.mr_M_d.p, m.mr_M_h.p, M.size() * 4, hipMemcpyHostToDevice, c->stream));
    std::copy(lines.begin(), lines.end(), m.mr_lines_h.p);
    if (!lines.empty()) NALO_HIP(c, hipMemcpyAsync(m.mr_lines_d.p, m.mr_lines_h.p, lines.size() * sizeof(MrLine), hipMemcpyHostToDevice, c->stream));
    D.M = m.mr_M_d.p; D.mode = a->display_mode; D.scaledTH = a->scaledTH; D.absTH = a->absTH; D.minRelBS = a->minRelBS; std::memcpy(D.ci, V0.ci, sizeof(D.ci)); D.cam = cam;
    D.lines = m.mr_lines_d.p; D.n_lines = (int)lines.size(); D.key = m.mr_key.p; D.padded = padded;
    D.cnt = m.mr_cnt.p + kMrCounters * m.mr_cnt_buf; m.mr_cnt_buf ^= 1; D.cnt_next = m.mr_cnt.p + kMrCounters * m.mr_cnt_buf;
    D.rgb = m.mr_rgb.p; D.depth = m.mr_depth.p; D.background = ((unsigned)a->background[0] << 16) | ((unsigned)a->background[1] << 8) | a->background[2];
    if (user_wait) {                                                           // the caller's arrays: everything queued on producer_stream so far comes first, on the device
        NALO_HIP(c, c->ev_prod.create(hipEventDisableTiming));
        NALO_HIP(c, hipEventRecord(c->ev_prod, user_stream)); NALO_HIP(c, hipStreamWaitEvent(c->stream, c->ev_prod, 0));
    }
    { const int rc = map_render_launch(c, D, mesh ? &T : nullptr); if (rc) return rc; }
    m.mr_key.settled();
    NALO_HIP(c, hipMemcpyAsync(m.mr_host.p, D.cnt, kMrCounters * 8, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(m.mr_host.p + off_rgb, m.mr_rgb.p, 3 * npx, hipMemcpyDeviceToHost, c->stream));
    if (a->depth) NALO_HIP(c, hipMemcpyAsync(m.mr_host.p + off_depth, m.mr_depth.p, 4 * npx, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    unsigned long long cnt[kMrCounters];
    std::memcpy(cnt, m.mr_host.p, sizeof(cnt));
    a->n_vertices = (long long)cnt[0]; a->n_drawn_points = (long long)cnt[1]; a->n_segments = n_segments; a->n_line_samples = (long long)cnt[2];
    if (mesh) {
        mesh->n_triangles = n_triangles; mesh->n_tri_bad_index = (long long)cnt[4]; mesh->n_tri_near = (long long)cnt[5]; mesh->n_tri_guard = (long long)cnt[6];
        mesh->n_tri_degenerate = (long long)cnt[7]; mesh->n_tri_large = (long long)cnt[8]; mesh->n_tri_pixels = (long long)cnt[9];
    }
    std::memcpy(a->rgb, m.mr_host.p + off_rgb, 3 * npx);
    if (a->depth) std::memcpy(a->depth, m.mr_host.p + off_depth, 4 * npx);
    return NALO_OK;
}

int nalo_map_render(nalo_ctx* c, nalo_map_render_args* a) { return map_render_impl(c, a, nullptr, "nalo_map_render: "); }

int nalo_map_render_mesh(nalo_ctx* c, nalo_map_render_args* a, nalo_map_render_mesh_args* mesh) {
    if (!mesh) {
        if (a) a->n_vertices = a->n_drawn_points = a->n_segments = a->n_line_samples = 0;
        return fail(c, NALO_ERR_ARG, "nalo_map_render_mesh: bad argument");
    }
    return map_render_impl(c, a, mesh, "nalo_map_render_mesh: ");
}

int nalo_map_graph_enable(nalo_ctx* c, int on) {
    if (!c) return NALO_ERR_ARG;
    if (!on) { c->graph_on = false; return NALO_OK; }
    if (c->xchg_failed) return fail(c, NALO_ERR_STATE, "nalo_map_graph_enable: a cross-rank sum of this context failed earlier");
    GraphWindowView V;
    const bool window = ba_graph_view(c, false, &V) == NALO_OK;
    if (window && V.sharded) return fail(c, NALO_ERR_STATE, "nalo_map_graph_enable: the window is sharded (a rank holds only its own points)");
    if (window) for (int i = 0; i < V.W; ++i) if (V.ids[i] < 0) return fail(c, NALO_ERR_ARG, "nalo_map_graph_enable: a window frame has a negative frame_id");
    c->graph_on = true;
    if (window) graph_add_frames(c, V.W, V.ids);
    return NALO_OK;
}

int nalo_map_graph(nalo_ctx* c, nalo_graph_edge* edges, int cap, int* n) {
    if (!c || !n || cap < 0) return fail(c, NALO_ERR_ARG, "nalo_map_graph: bad argument");
    std::vector<nalo_graph_edge> E;
    { const int rc = graph_entries(c, "nalo_map_graph", E); if (rc) return rc; }
    *n = (int)E.size();
    if (cap < *n || (*n > 0 && !edges)) return fail(c, NALO_ERR_ARG, "nalo_map_graph: cap is smaller than the number of entries");
    std::copy(E.begin(), E.end(), edges);
    return NALO_OK;
}

int nalo_map_graph_connections(nalo_ctx* c, nalo_graph_connection* conn, int cap, int* n) {
    if (!c || !n || cap < 0) return fail(c, NALO_ERR_ARG, "nalo_map_graph_connections: bad argument");
    std::vector<nalo_graph_connection> C;
    { const int rc = graph_connections(c, "nalo_map_graph_connections", C); if (rc) return rc; }
    *n = (int)C.size();
    if (cap < *n || (*n > 0 && !conn)) return fail(c, NALO_ERR_ARG, "nalo_map_graph_connections: cap is smaller than the number of connections");
    std::copy(C.begin(), C.end(), conn);
    return NALO_OK;
}

int nalo_map_dense_enable(nalo_ctx* c, int on, int chunk_points) {
    if (!c) return NALO_ERR_ARG;
    if (chunk_points < 0) return fail(c, NALO_ERR_ARG, "nalo_map_dense_enable: chunk_points must not be negative");
    if (on && (c->w > 65535 || c->h > 65535)) return fail(c, NALO_ERR_UNSUPPORTED, "nalo_map_dense_enable: images wider or higher than 65535 (u, v are 16 bits)");
    if (!c->dmap) { if (!on) return NALO_OK; c->dmap = new DenseArchive(); }
    DenseArchive& m = *c->dmap;
    if (on && m.chunks.empty()) m.chunk = chunk_points > 0 ? chunk_points : 262144;
    m.on = on != 0;
    return NALO_OK;
}

int nalo_map_dense_counts(nalo_ctx* c, int frame_id, int* n_points, int* n_runs) {
    if (!c || !n_points || !n_runs) return fail(c, NALO_ERR_ARG, "nalo_map_dense_counts: bad argument");
    DenseFrame* f = nullptr;
    { int rc = map_dense_frame(c, "nalo_map_dense_counts", frame_id, &f); if (rc) return rc; }
    *n_points = (int)f->points; *n_runs = f->n_runs;
    return NALO_OK;
}

int nalo_map_dense_get(nalo_ctx* c, int frame_id, nalo_dense_point* out, int cap, int* n) {
    if (!c || !n || cap < 0) return fail(c, NALO_ERR_ARG, "nalo_map_dense_get: bad argument");
    DenseFrame* f = nullptr;
    { int rc = map_dense_frame(c, "nalo_map_dense_get", frame_id, &f); if (rc) return rc; }
    DenseArchive& m = *c->dmap;
    *n = (int)f->points;
    if (cap < *n || (*n > 0 && !out)) return fail(c, NALO_ERR_ARG, "nalo_map_dense_get: cap is smaller than the frame's point count");
    if (*n == 0) return NALO_OK;
    NALO_HIP(c, hipSetDevice(c->device));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    size_t at = 0;
    for (const MapRun& r : f->runs) {
        NALO_HIP(c, hipMemcpy(out + at, m.chunks[(size_t)(r.off / m.chunk)].p + r.off % m.chunk, (size_t)r.n * sizeof(nalo_dense_point), hipMemcpyDeviceToHost));
        at += (size_t)r.n;
    }
    return NALO_OK;
}

int nalo_map_dense_world_points(nalo_ctx* c, int frame_id, const double camToWorld[12], double* xyz, int cap, int* n) {
    if (!c || !camToWorld || !n || cap < 0) return fail(c, NALO_ERR_ARG, "nalo_map_dense_world_points: bad argument");
    DenseFrame* f = nullptr;
    { int rc = map_dense_frame(c, "nalo_map_dense_world_points", frame_id, &f); if (rc) return rc; }
    DenseArchive& m = *c->dmap;
    *n = (int)f->points;
    if (cap < *n || (*n > 0 && !xyz)) return fail(c, NALO_ERR_ARG, "nalo_map_dense_world_points: cap is smaller than the frame's point count");
    if (*n == 0) return NALO_OK;
    MapWindowView V;
    { int rc = ba_map_view(c, frame_id, &V); if (rc) return rc; }
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "map_dense_world_points");
    MapDenseDev D{};
    { int rc = map_dense_send(c, m, *f, D); if (rc) return rc; }
    NALO_HIP(c, m.wxyz.reserve(3 * (size_t)*n)); NALO_HIP(c, m.wxyz_h.reserve(3 * (size_t)*n));
    std::memcpy(D.ci, V.ci, sizeof(D.ci)); std::memcpy(D.m, camToWorld, sizeof(D.m)); D.wxyz = m.wxyz.p;
    { int rc = map_dense_world_launch(c, D); if (rc) return rc; }
    NALO_HIP(c, hipMemcpyAsync(m.wxyz_h.p, m.wxyz.p, 3 * (size_t)*n * 8, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(xyz, m.wxyz_h.p, 3 * (size_t)*n * 8);
    return NALO_OK;
}

int nalo_map_dense_cloud(nalo_ctx* c, nalo_map_dense_cloud_args* a) {
    if (!c || !a) return fail(c, NALO_ERR_ARG, "nalo_map_dense_cloud: bad argument");
    a->n = 0; a->n_needed = 0; a->records = 0; a->survivors = 0;
    if (a->cap < 0 || a->n_draws < 0) return fail(c, NALO_ERR_ARG, "nalo_map_dense_cloud: bad argument");
    DenseFrame* f = nullptr;
    { int rc = map_dense_frame(c, "nalo_map_dense_cloud", a->frame_id, &f); if (rc) return rc; }
    DenseArchive& m = *c->dmap;
    const int records = (int)f->points;
    a->n_needed = records; a->records = records;
    if (a->cap < records || (a->draws && a->n_draws < records)) return fail(c, NALO_ERR_ARG, "nalo_map_dense_cloud: cap / n_draws below the frame's records (n_needed)");
    if (records > 0 && (!a->xyz || !a->rgb)) return fail(c, NALO_ERR_ARG, "nalo_map_dense_cloud: xyz and rgb required");
    if (records == 0) return NALO_OK;
    MapWindowView V;
    { int rc = ba_map_view(c, a->frame_id, &V); if (rc) return rc; }
    NALO_HIP(c, hipSetDevice(c->device));
    HostTimer ht(c, "map_dense_cloud");
    MapDenseDev D{};
    { int rc = map_dense_send(c, m, *f, D); if (rc) return rc; }
    const size_t nv = (size_t)records;
    NALO_HIP(c, m.cxyz.reserve(3 * nv)); NALO_HIP(c, m.crgb.reserve(3 * nv)); NALO_HIP(c, m.cxyz_h.reserve(3 * nv)); NALO_HIP(c, m.crgb_h.reserve(3 * nv)); NALO_HIP(c, m.cnt_h.reserve(1));
    std::memcpy(D.ci, V.ci, sizeof(D.ci)); D.xyz = m.cxyz.p; D.rgb = m.crgb.p;
    if (a->draws) {
        NALO_HIP(c, m.draws_h.reserve(nv)); NALO_HIP(c, m.draws_d.reserve(nv));
        std::memcpy(m.draws_h.p, a->draws, nv * 4);
        NALO_HIP(c, hipMemcpyAsync(m.draws_d.p, m.draws_h.p, nv * 4, hipMemcpyHostToDevice, c->stream));
        D.draws = m.draws_d.p;
    }
    { int rc = map_dense_cloud_launch(c, D); if (rc) return rc; }
    // the vertex count is known only behind the scan: everything the call may have written comes up in the one wait
    NALO_HIP(c, hipMemcpyAsync(m.cnt_h.p, D.cnt + D.nb, 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(m.cxyz_h.p, m.cxyz.p, 3 * nv * 4, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipMemcpyAsync(m.crgb_h.p, m.crgb.p, 3 * nv, hipMemcpyDeviceToHost, c->stream));
    NALO_HIP(c, hipStreamSynchronize(c->stream));
    const int ns = m.cnt_h.p[0];
    if (ns < 0 || (size_t)ns > nv) return fail(c, NALO_ERR_HIP, "nalo_map_dense_cloud: the device counted more survivors than the frame has records");
    a->n = ns; a->survivors = ns;
    std::memcpy(a->xyz, m.cxyz_h.p, 3 * (size_t)ns * 4); std::memcpy(a->rgb, m.crgb_h.p, 3 * (size_t)ns);
    return NALO_OK;
}

}
