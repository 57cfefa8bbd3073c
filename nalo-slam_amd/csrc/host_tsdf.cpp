// The TSDF section's host-only arithmetic (include/nalo_gpu.h): the descriptor's refusals, worldToCam (and at an estimate: nalo_tsdf_est_world_to_cam), the culling box
// nalo_tsdf_frustum_box[_est], the mesh's triangle table and the geometry of a shifted volume (the origin, nalo_tsdf_shift_for, nalo_tsdf_shift_boxes, nalo_tsdf_box_shift). Plain C++ with no device call, built without FMA contraction: every
// line below is the operation order the header defines, in double (the shifted origin: in float).
#include <cmath>
#include <cstring>

#include "host_math.h"
#include "tsdf_host.h"
#include "tsdf_mesh_table.h"

namespace nalo {

const char* tsdf_desc_refusal(const nalo_tsdf_desc* d) {
    if (!d) return "null descriptor";
    long long n = 1;
    for (int a = 0; a < 3; ++a) {
        if (d->dims[a] < 1 || d->dims[a] > 2048) return "a dimension outside [1, 2048]";
        n *= d->dims[a];
        if (!std::isfinite(d->origin[a])) return "origin is not finite";
    }
    if (n > (1LL << 29)) return "more than 2^29 voxels";
    if (!std::isfinite(d->voxel_size) || d->voxel_size <= 0) return "voxel_size is not finite or <= 0";
    if (!std::isfinite(d->trunc) || d->trunc <= 0) return "trunc is not finite or <= 0";
    if (!std::isfinite(d->max_weight) || d->max_weight <= 0) return "max_weight is not finite or <= 0";
    return nullptr;
}

bool tsdf_world_to_cam(const double c[12], float M[12]) {
    for (int i = 0; i < 12; ++i) if (!std::isfinite(c[i])) return false;
    for (int r = 0; r < 3; ++r) {
        // row r of R^T is column r of R
        const double a = c[0 + r], b = c[4 + r], e = c[8 + r];
        M[4 * r + 0] = (float)a; M[4 * r + 1] = (float)b; M[4 * r + 2] = (float)e;
        M[4 * r + 3] = (float)(-((a * c[3] + b * c[7]) + e * c[11]));
    }
    return true;
}

constexpr long long kTsdfMaxBase = 1LL << 24;                                  // |base| up to here converts to float exactly

const char* tsdf_shift_geometry(const float origin0[3], float voxel_size, const int base[3], const int shift[3], int new_base[3], float origin[3]) {
    int nb[3]; float o[3];
    for (int a = 0; a < 3; ++a) {
        const long long b = (long long)base[a] + (long long)shift[a];
        if (b > kTsdfMaxBase || b < -kTsdfMaxBase) return "base + shift beyond 2^24 voxels";
        nb[a] = (int)b;
        const float step = (float)nb[a] * voxel_size;                           // rounded here; the file is built without contraction, so the sum rounds on its own
        o[a] = origin0[a] + step;
        if (!std::isfinite(o[a])) return "the shifted origin is not finite";
    }
    for (int a = 0; a < 3; ++a) { new_base[a] = nb[a]; origin[a] = o[a]; }
    return nullptr;
}

}  // namespace nalo

extern "C" int nalo_tsdf_shift_for(const nalo_tsdf_desc* now, const double centre[3], const int margin[3], int shift[3]) {
    if (!centre || !margin || !shift || nalo::tsdf_desc_refusal(now)) return NALO_ERR_ARG;
    int s[3];
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(centre[a]) || margin[a] < 0) return NALO_ERR_ARG;
        const double q = std::floor((centre[a] - (double)now->origin[a]) / (double)now->voxel_size);
        const double d = q - (double)(now->dims[a] / 2);
        if (!(std::fabs(d) <= (double)nalo::kTsdfMaxBase)) return NALO_ERR_ARG;     // an infinite quotient fails here too
        s[a] = std::fabs(d) > (double)margin[a] ? (int)d : 0;
    }
    for (int a = 0; a < 3; ++a) shift[a] = s[a];
    return NALO_OK;
}

extern "C" int nalo_tsdf_shift_boxes(const int dims[3], const int shift[3], struct nalo_tsdf_shift_boxes* out) {
    if (!dims || !shift || !out) return NALO_ERR_ARG;
    for (int a = 0; a < 3; ++a) if (dims[a] < 1 || dims[a] > 2048) return NALO_ERR_ARG;
    *out = {};
    // per axis in 64 bits (s + 1 and -s of any int): the kept voxels [klo, klo + kn) and the leaving ones, the seam voxel among them, [llo, llo + ln)
    long long klo[3], kn[3], llo[3], ln[3];
    bool all = false;
    for (int a = 0; a < 3; ++a) {
        const long long n = dims[a], s = shift[a];
        if (s >= n || -s >= n) all = true;
        klo[a] = s > 0 ? s : 0; kn[a] = n - (s > 0 ? s : -s);
        llo[a] = s > 0 ? 0 : s < 0 ? (n + s - 1 > 0 ? n + s - 1 : 0) : 0;
        ln[a] = s > 0 ? (s + 1 < n ? s + 1 : n) : s < 0 ? n - llo[a] : 0;
    }
    if (all) {                                                                  // nothing is kept: the whole grid is the one box
        out->n_boxes = 1;
        for (int a = 0; a < 3; ++a) out->size[0][a] = dims[a];
        return NALO_OK;
    }
    for (int a = 0; a < 3; ++a) { out->kept_lo[a] = (int)klo[a]; out->kept_size[a] = (int)kn[a]; }
    for (int b = 0; b < 3; ++b) {                                               // box b: kept on the axes before b, leaving on b, everything behind it
        if (shift[b] == 0) continue;
        int* lo = out->lo[out->n_boxes]; int* size = out->size[out->n_boxes];
        for (int a = 0; a < 3; ++a) {
            lo[a] = a < b ? (int)klo[a] : a == b ? (int)llo[a] : 0;
            size[a] = a < b ? (int)kn[a] : a == b ? (int)ln[a] : dims[a];
        }
        ++out->n_boxes;                                                         // every extent is >= 1 here: |s| < n on every axis
    }
    return NALO_OK;
}

// nalo_tsdf_frustum_box (s = 1) and nalo_tsdf_frustum_box_est: the one statement of the culling box. With s = 1 the quotient trunc / s and the product with s
// are exact, so the first is the second at a scale of one, bit for bit
static int tsdf_frustum_box(const nalo_tsdf_desc* d, int w, int h, const float K[4], const double c[12], double s, float max_depth, int lo[3], int hi[3]) {
    if (!K || !c || !lo || !hi || w < 1 || h < 1 || nalo::tsdf_desc_refusal(d) || !std::isfinite(max_depth)) return NALO_ERR_ARG;
    for (int i = 0; i < 4; ++i) if (!std::isfinite(K[i])) return NALO_ERR_ARG;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(c[i])) return NALO_ERR_ARG;
    if (!std::isfinite(s) || s <= 0.0) return NALO_ERR_ARG;
    const double z = (double)max_depth + (double)d->trunc / s;
    double mn[3] = {c[3], c[7], c[11]}, mx[3] = {c[3], c[7], c[11]};          // the apex
    bool bad[3] = {false, false, false};
    for (int cv = 0; cv < 2; ++cv)
        for (int cu = 0; cu < 2; ++cu) {
            const double uf = cu ? (double)w : 0.0, vf = cv ? (double)h : 0.0;
            const double X = (((uf - 0.5) - (double)K[2]) / (double)K[0]) * z, Y = (((vf - 0.5) - (double)K[3]) / (double)K[1]) * z;
            for (int a = 0; a < 3; ++a) {
                const double p = (((c[4 * a] * X + c[4 * a + 1] * Y) + c[4 * a + 2] * z) * s) + c[4 * a + 3];
                if (std::isnan(p)) bad[a] = true;                                // inf - inf at an absurd pose: the axis takes the whole grid below
                if (p < mn[a]) mn[a] = p;
                if (p > mx[a]) mx[a] = p;
            }
        }
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        if (bad[a]) { lo[a] = 0; hi[a] = d->dims[a]; continue; }
        const double l = std::floor((mn[a] - (double)d->origin[a]) / (double)d->voxel_size - 0.5) - 1.0;
        const double u = std::ceil((mx[a] - (double)d->origin[a]) / (double)d->voxel_size - 0.5) + 2.0;
        const int n = d->dims[a];
        lo[a] = !(l > 0) ? 0 : l > n ? n : (int)l;                             // compared as doubles before any conversion; a NaN gives the grid's own bound
        hi[a] = !(u < n) ? n : u < 0 ? 0 : (int)u;
        if (lo[a] >= hi[a]) empty = true;
    }
    if (empty) for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0;
    return NALO_OK;
}
extern "C" int nalo_tsdf_frustum_box(const nalo_tsdf_desc* d, int w, int h, const float K[4], const double c[12], float max_depth, int lo[3], int hi[3]) {
    return tsdf_frustum_box(d, w, h, K, c, 1.0, max_depth, lo, hi);
}
extern "C" int nalo_tsdf_frustum_box_est(const nalo_tsdf_desc* d, int w, int h, const float K[4], const nalo_tsdf_align_est* est, float max_depth, int lo[3], int hi[3]) {
    if (!est) return NALO_ERR_ARG;
    return tsdf_frustum_box(d, w, h, K, est->camToWorld, est->s, max_depth, lo, hi);
}

extern "C" int nalo_tsdf_est_world_to_cam(const nalo_tsdf_align_est* est, float M[12]) {
    if (!est || !M) return NALO_ERR_ARG;
    const double* c = est->camToWorld; const double s = est->s;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(c[i])) return NALO_ERR_ARG;
    if (!std::isfinite(s) || s <= 0.0) return NALO_ERR_ARG;
    for (int r = 0; r < 3; ++r) {
        // row r of R^T is column r of R; tsdf_world_to_cam's sums, every entry over s (s = 1: the same bits, a quotient by 1.0 is exact)
        const double a = c[0 + r], b = c[4 + r], e = c[8 + r];
        M[4 * r + 0] = (float)(a / s); M[4 * r + 1] = (float)(b / s); M[4 * r + 2] = (float)(e / s);
        M[4 * r + 3] = (float)(-((a * c[3] + b * c[7]) + e * c[11]) / s);
    }
    return NALO_OK;
}

extern "C" int nalo_tsdf_box_shift(const int dims[3], const int shift[3], int lo[3], int size[3]) {
    if (!dims || !shift || !lo || !size) return NALO_ERR_ARG;
    for (int a = 0; a < 3; ++a) if (dims[a] < 1 || dims[a] > 2048) return NALO_ERR_ARG;
    // per axis in 64 bits (lo - shift and lo + size of any ints): the translated range cut to [0, dims)
    long long l[3], u[3];
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        l[a] = (long long)lo[a] - (long long)shift[a];
        u[a] = l[a] + (long long)size[a];
        if (l[a] < 0) l[a] = 0;
        if (u[a] > dims[a]) u[a] = dims[a];
        if (size[a] < 1 || l[a] >= u[a]) empty = true;
    }
    for (int a = 0; a < 3; ++a) { lo[a] = empty ? 0 : (int)l[a]; size[a] = empty ? 0 : (int)(u[a] - l[a]); }
    return NALO_OK;
}

// nalo_tsdf_replace_frames' host half that needs neither a context nor a device: the list's own refusals, and which frames skip_unchanged leaves out
const char* nalo::tsdf_replace_frames_plan(const nalo_tsdf_replace_frames_args* a, const nalo_tsdf_log_entry* log, int n_log, const int* list_len, unsigned char* skip) {
    if (!a || !skip || n_log < 0 || (n_log > 0 && !log)) return "bad argument";
    if (a->n < 1 || a->n > 16) return "n outside 1 .. 16";
    if (!a->frame_id) return "bad argument";
    for (int k = 0; k < a->n; ++k) skip[k] = 0;
    for (int k = 1; k < a->n; ++k) for (int q = 0; q < k; ++q) if (a->frame_id[q] == a->frame_id[k]) return "a frame_id appears twice";
    bool any_est = false;
    for (int k = 0; k < a->n; ++k) {
        if (!a->est_new || (a->has_est && !a->has_est[k])) continue;
        any_est = true;
        const nalo_tsdf_align_est& e = a->est_new[k];
        for (int i = 0; i < 12; ++i) if (!std::isfinite(e.camToWorld[i])) return "an estimate's camToWorld is not finite";
        if (!std::isfinite(e.s) || e.s <= 0.0) return "an estimate's s is not finite or <= 0";
    }
    if (any_est) {
        for (int i = 0; i < 4; ++i) if (!std::isfinite(a->K[i])) return "K is not finite";
        if (!std::isfinite(a->min_depth) || !std::isfinite(a->max_depth) || a->min_depth > a->max_depth) return "min_depth / max_depth not finite, or min_depth > max_depth";
    }
    if (!a->skip_unchanged) return nullptr;
    // unchanged: the frame has an entry, its estimate, K and range are the entry's bit for bit, and its dense list is as long as when it was fused
    for (int k = 0; k < a->n; ++k) {
        if (!a->est_new || (a->has_est && !a->has_est[k]) || !list_len) continue;
        for (int q = 0; q < n_log; ++q) {
            const nalo_tsdf_log_entry& e = log[q];
            if (e.frame_id != a->frame_id[k]) continue;
            skip[k] = std::memcmp(e.est.camToWorld, a->est_new[k].camToWorld, sizeof e.est.camToWorld) == 0 && std::memcmp(&e.est.s, &a->est_new[k].s, sizeof e.est.s) == 0 &&
                      std::memcmp(e.K, a->K, sizeof e.K) == 0 && std::memcmp(&e.min_depth, &a->min_depth, sizeof(float)) == 0 &&
                      std::memcmp(&e.max_depth, &a->max_depth, sizeof(float)) == 0 && list_len[k] == e.n_records;
            break;
        }
    }
    return nullptr;
}
extern "C" int nalo_tsdf_replace_frames_plan(const nalo_tsdf_replace_frames_args* args, const nalo_tsdf_log_entry* log, int n_log, const int* list_len, unsigned char* skip) {
    return nalo::tsdf_replace_frames_plan(args, log, n_log, list_len, skip) ? NALO_ERR_ARG : NALO_OK;
}

extern "C" int nalo_tsdf_mesh_table(signed char out[6][16][6]) {
    if (!out) return NALO_ERR_ARG;
    static constexpr nalo::TsdfMeshTable T = nalo::tsdf_mesh_make_table();      // built from the rules at compile time; the kernels hold the same object
    for (int t = 0; t < 6; ++t)
        for (int m = 0; m < 16; ++m)
            for (int k = 0; k < 6; ++k) out[t][m][k] = T.e[t][m][k];
    return NALO_OK;
}

extern "C" int nalo_tsdf_align_step(const double H[28], const double b[7], double lambda, int dof, const nalo_tsdf_align_est* est, double inc[7], nalo_tsdf_align_est* est_out) {
    if (!H || !b || !est || !inc || !est_out || (dof != 6 && dof != 7) || !std::isfinite(lambda) || lambda < 0.0) return NALO_ERR_ARG;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(est->camToWorld[i])) return NALO_ERR_ARG;
    if (!std::isfinite(est->s) || est->s <= 0.0) return NALO_ERR_ARG;
    // Hl = H with its diagonal scaled, the leading dof x dof block, from the row-major upper triangle; L L^T = Hl in place of its lower triangle
    double L[7][7], x[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0, k = 0; i < 7; ++i)
        for (int j = i; j < 7; ++j, ++k) {
            if (j >= dof) continue;
            const double h = i == j ? H[k] * (1.0 + lambda) : H[k];
            if (!std::isfinite(h)) return NALO_ERR_ARG;
            L[j][i] = h;
        }
    for (int i = 0; i < dof; ++i) if (!std::isfinite(b[i])) return NALO_ERR_ARG;
    for (int j = 0; j < dof; ++j) {
        double d = L[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !std::isfinite(d)) return NALO_ERR_ARG;              // not positive definite (a NaN fails the comparison)
        const double l = std::sqrt(d);
        L[j][j] = l;
        for (int i = j + 1; i < dof; ++i) {
            double s = L[i][j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / l;
        }
    }
    for (int i = 0; i < dof; ++i) {                                            // L y = -b
        double s = -b[i];
        for (int k = 0; k < i; ++k) s -= L[i][k] * x[k];
        x[i] = s / L[i][i];
    }
    for (int i = dof - 1; i >= 0; --i) {                                       // L^T x = y
        double s = x[i];
        for (int k = i + 1; k < dof; ++k) s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    const nalo::SE3 T = nalo::se3_exp(x) * nalo::SE3::from(est->camToWorld);
    const double s = est->s * std::exp(x[6]);
    for (int i = 0; i < 7; ++i) if (!std::isfinite(x[i])) return NALO_ERR_ARG;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(T.m[i])) return NALO_ERR_ARG;
    if (!std::isfinite(s) || s <= 0.0) return NALO_ERR_ARG;
    for (int i = 0; i < 7; ++i) inc[i] = x[i];
    for (int i = 0; i < 12; ++i) est_out->camToWorld[i] = T.m[i];
    est_out->s = s;
    return NALO_OK;
}

extern "C" int nalo_tsdf_raycast_steps(float min_depth, float max_depth, float step, int* n_steps) {
    if (!n_steps) return NALO_ERR_ARG;
    *n_steps = 0;
    if (!std::isfinite(min_depth) || !std::isfinite(max_depth) || !std::isfinite(step) || min_depth < 0.0f || min_depth > max_depth || !(step > 0.0f)) return NALO_ERR_ARG;
    // z_n = min_depth + (float)n * step does not decrease with n, so the n with z_n <= max_depth form a prefix; n = 0 is always one of them
    int n = 0;
    while (n <= 4096) {
        const float z = min_depth + (float)n * step;
        if (!(z <= max_depth)) break;
        ++n;
    }
    if (n > 4096) return NALO_ERR_ARG;                                          // z_4096 <= max_depth: more than 4096 steps
    *n_steps = n;
    return NALO_OK;
}
