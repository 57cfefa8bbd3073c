// The host half of the ground-plane scale correction: the scale_fix / scale_rate state machine of CoarseTracker::makeCoarseDepthL0 (reference
// src/FullSystem/CoarseTracker.cpp:609-616, 696-816), FullSystem::setglobalplane / resetGlobalPlane (FullSystem.cpp:1911-2001) and the local scale of
// FullSystem::planeOptimize (PlaneOptimize.cpp:203-211) over caller-owned structs. Plain host code without a context: it runs on a machine without a device.
// include/nalo_gpu.h has the semantics, tests/ground_model.py the same in NumPy. Built without FMA contraction: the float arithmetic is the reference's as written.
#include <cmath>
#include <cstring>

#include "../../include/nalo_gpu.h"

extern "C" {

void nalo_ground_tracker_init(nalo_ground_tracker* t) { if (t) { t->ground_height = -1.f; t->last_height = -1.f; t->suc_num = 0; } }      // CoarseTracker.cpp:104-106
void nalo_ground_globals_init(nalo_ground_globals* g) {                                                                               // util/settings.cpp:36-40
    if (!g) return;
    std::memset(g, 0, sizeof(*g));
    g->init_height = -1.f; g->last_ScaleRate = -1.f;
    for (int k = 0; k < 4; ++k) g->last_gp[k] = -1.f;
}
void nalo_ground_frame_init(nalo_ground_frame* f) { if (f) std::memset(f, 0, sizeof(*f)); }

int nalo_ground_update(const nalo_ground_pick* pick, nalo_ground_tracker* tr, nalo_ground_globals* g, nalo_ground_frame* frames, int W) {
    if (!pick || !tr || !g || !frames || W < 1) return NALO_ERR_ARG;
    if (!pick->ran) return NALO_OK;                                     // :563-567: the function returned before the loop
    float gp_raw[4] = {0.f, 0.f, 0.f, 0.f};                             // :577
    if (pick->cluster >= 0) {                                           // :609-616
        for (int k = 0; k < 4; ++k) gp_raw[k] = pick->gp_raw[k];
        tr->ground_height = pick->ground_height;
    }
    nalo_ground_frame& back = frames[W - 1];
    const float ground_height = tr->ground_height;
    if (!g->scale_fix) {                                                // :696-716
        if (tr->last_height < 0) tr->last_height = ground_height;
        else {
            const float diff = std::fabs(tr->last_height - ground_height);
            if (diff < 0.01) tr->suc_num++;                             // a float against the double 0.01
            else tr->suc_num = 0;
        }
        if (tr->suc_num > 3) {
            g->init_height = (ground_height + tr->last_height) / 2;
            g->scale_fix = 1;
        }
        tr->last_height = ground_height;
    } else {                                                            // :717-790
        float scale_rate = ground_height / g->init_height;
        if (g->last_ScaleRate < 0) {
            g->last_ScaleRate = scale_rate;
            for (int k = 0; k < 4; ++k) g->last_gp[k] = gp_raw[k];
            if (g->n_old < 7) g->old_rate[g->n_old++] = g->last_ScaleRate;     // push_back (the deque is empty here in the reference)
        } else {
            float ave2, ave3, ave4, ave5;
            ave2 = ave3 = ave4 = ave5 = scale_rate;
            const int size = g->n_old;
            const float* o = g->old_rate;
            if (size > 2) ave2 = std::fabs(o[size - 1] + o[size - 2]) / 2;
            if (size > 3) ave3 = std::fabs(o[size - 1] + o[size - 2] + o[size - 3]) / 3;
            if (size > 4) ave4 = std::fabs(o[size - 1] + o[size - 2] + o[size - 3] + o[size - 4]) / 4;
            if (size > 5) ave5 = std::fabs(o[size - 1] + o[size - 2] + o[size - 3] + o[size - 4] + o[size - 5]) / 5;
            const float diff = std::fabs(g->last_ScaleRate - scale_rate) / g->last_ScaleRate;
            const float diff2 = std::fabs(ave2 - scale_rate) / ave2;
            const float diff3 = std::fabs(ave3 - scale_rate) / ave3;
            const float diff4 = std::fabs(ave4 - scale_rate) / ave4;
            const float diff5 = std::fabs(ave5 - scale_rate) / ave5;
            if (diff > 0.25 && diff2 > 0.25 && diff3 > 0.25 && diff4 > 0.25 && diff5 > 0.25) {
                scale_rate = g->last_ScaleRate;
                for (int k = 0; k < 4; ++k) back.groundP[k] = g->last_gp[k];  // haveground is NOT set (:768 is commented out)
            } else {
                g->last_ScaleRate = scale_rate;
                back.haveground = 1;
                for (int k = 0; k < 4; ++k) back.groundP[k] = gp_raw[k];
            }
            if (g->n_old < 7) g->old_rate[g->n_old++] = g->last_ScaleRate;
            else { for (int k = 0; k < 6; ++k) g->old_rate[k] = g->old_rate[k + 1]; g->old_rate[6] = g->last_ScaleRate; }      // pop_front, push_back
        }
    }
    if (g->scale_fix && W > 6) {                                        // :792-816 (the assert of :794 is not reproduced)
        for (int fhid = W - 2; fhid > 0; fhid--) {
            if (frames[fhid].groundP[3] == 0) continue;                 // :801-805: the four-zero test is implied by the second one
            for (int k = 0; k < 4; ++k) back.last_ground[k] = frames[fhid].groundP[k];
            break;
        }
    }
    return NALO_OK;
}

int nalo_ground_set_global_plane(const nalo_ground_frame* frames, int W, int max_frames, const double worldToCam_frame1[12], double gplane[4],
                                 double backup_gplane[4], float* lgh) {
    if (!frames || !worldToCam_frame1 || !gplane || !backup_gplane || !lgh) return NALO_ERR_ARG;
    if (W < max_frames || W < 2) return 0;                              // :1913
    double sumnorm = 0;
    double lastpi[4];
    for (int k = 0; k < 4; ++k) lastpi[k] = frames[W - 2].groundP[k];
    for (int i = W - 2; i > 0; i--) {
        double pi[4];
        for (int k = 0; k < 4; ++k) { pi[k] = lastpi[k]; lastpi[k] = frames[i - 1].groundP[k]; }
        if (pi[3] == 0 || std::isnan(pi[3]) || std::isnan(pi[0]) || std::isnan(pi[1]) || std::isnan(pi[2]) || std::fabs(pi[1]) > 1) return 0;     // :1934
        double sq = 0;
        for (int k = 0; k < 4; ++k) { const double d = pi[k] - lastpi[k]; sq += d * d; }
        sumnorm += std::sqrt(sq);
    }
    if (!(sumnorm < 0.2)) return 0;                                     // :1944
    double pih[4], piw[4];
    for (int k = 0; k < 4; ++k) pih[k] = frames[1].groundP[k];
    const double* M = worldToCam_frame1;                                // rows 0-2 of PRE_worldToCam.matrix(); row 3 is (0, 0, 0, 1)
    for (int j = 0; j < 4; ++j) {                                       // piw = M^T pih (:1954)
        double s = M[j] * pih[0];
        s += M[4 + j] * pih[1];
        s += M[8 + j] * pih[2];
        s += (j == 3 ? 1.0 : 0.0) * pih[3];
        piw[j] = s;
    }
    for (int k = 0; k < 4; ++k) { gplane[k] = piw[k]; backup_gplane[k] = piw[k]; }
    *lgh = (float)pih[3];                                               // :1970
    return 1;
}

int nalo_ground_local_scale(const nalo_ground_frame* f, float lgh, double* localscale) {
    if (!f || !localscale) return NALO_ERR_ARG;
    if (!f->haveground) return 0;                                       // PlaneOptimize.cpp:203
    *localscale = (double)lgh / (double)f->groundP[3];                  // :211: float getlocalgh() over the double local_plane[3]
    return 1;
}

int nalo_ground_reset_global_plane(const nalo_ground_frame* frames, int W, const double* worldToCam, double gplane[4]) {
    if (!frames || !worldToCam || !gplane) return NALO_ERR_ARG;
    for (int i = W - 2; i >= 0; i--) {                                  // FullSystem.cpp:1982-2000
        if (!frames[i].haveground) continue;
        const double* M = worldToCam + 12 * (size_t)i;
        const double p[4] = {frames[i].groundP[0], frames[i].groundP[1], frames[i].groundP[2], frames[i].groundP[3]};
        for (int j = 0; j < 4; ++j) {
            double s = M[j] * p[0];
            s += M[4 + j] * p[1];
            s += M[8 + j] * p[2];
            s += (j == 3 ? 1.0 : 0.0) * p[3];
            gplane[j] = s;
        }
        return i;
    }
    return -1;
}

}  // extern "C"
