// nalo_view_triangle (include/nalo_gpu.h, "The mesh in the 3-D panel"): steps 2-5 of nalo_map_render_mesh's definition for one triangle, on the host, through the
// function mr_tris_kernel calls (map_render_tri.h). Plain C++ with no device call, built without FMA contraction, so that a CPU program can exercise it.
#include "../../include/nalo_gpu.h"
#include "map_render_tri.h"

extern "C" int nalo_view_triangle(const nalo_map_render_args* cam, const float view_xyz[3][3], long long max_box_pixels, int* cls, int X[3], int Y[3], int box[4]) {
    if (!cam || !view_xyz || !cls || !X || !Y || !box) return NALO_ERR_ARG;
    if (cam->vw < 1 || cam->vh < 1 || cam->vw > nalo::kMrMaxView || cam->vh > nalo::kMrMaxView || max_box_pixels < 0) return NALO_ERR_ARG;
    const nalo::MrCam c{cam->vw, cam->vh, cam->fx, cam->fy, cam->cx, cam->cy, cam->znear, cam->zfar};
    nalo::MrTri T;
    nalo::mr_tri_classify(c, view_xyz, max_box_pixels == 0 ? nalo::kMrDefaultBox : max_box_pixels, T);
    *cls = T.cls;
    for (int i = 0; i < 3; ++i) { X[i] = T.X[i]; Y[i] = T.Y[i]; }
    for (int i = 0; i < 4; ++i) box[i] = T.box[i];
    return NALO_OK;
}
