// Projection of a solved box x = [sin, cos, l, h, w, X, Y, Z] into the image: rotation_matrix / create_corners /
// calc_proj_corners, utils/model_utils.py:66-152.  The one device statement of that arithmetic, shared by
// rtm3d_project_boxes (decode3d.hip) and the KITTI rows of rtm3d_records_to_camera (frames.hip).  fp64 like the reference;
// translation units that include this are compiled with -ffp-contract=off so that every user rounds alike.
#pragma once
#include "common.h"

// Ry = atan2(x0, x1) (utils/model_utils.py:300) and the rotation's sine / cosine, |sin|, |cos| < 1e-3 snapped to 0 (:66-77)
__device__ __forceinline__ double box_yaw(const double* __restrict__ xs, double& sn, double& cs) {
    const double ry = atan2(xs[0], xs[1]);
    sn = sin(ry); cs = cos(ry);
    if (fabs(sn) < 1e-3) sn = 0.0;
    if (fabs(cs) < 1e-3) cs = 0.0;
    return ry;
}

// pixel (u, v) of corner c through K (9 doubles, row-major): c = 0..7 in the order i, j, k in {1, -1} nested, c = 8 the
// centre; corners = (R diag(l, h, w) / 2) signs + location, divide by z + 1e-6
__device__ __forceinline__ void box_project_corner(const double* __restrict__ xs, const double* __restrict__ k, double sn, double cs,
                                                   int c, double& u, double& v) {
    const double dx = xs[2] / 2, dy = xs[3] / 2, dz = xs[4] / 2;  // dimension = (h, w, l) = (x3, x4, x2): half extents (l, h, w) / 2
    const double sx = c == 8 ? 0.0 : ((c & 4) ? -1.0 : 1.0), sy = c == 8 ? 0.0 : ((c & 2) ? -1.0 : 1.0), sz = c == 8 ? 0.0 : ((c & 1) ? -1.0 : 1.0);
    const double X = (cs * dx) * sx + (sn * dz) * sz + xs[5];
    const double Y = dy * sy + xs[6];
    const double Z = (-sn * dx) * sx + (cs * dz) * sz + xs[7];
    const double pu = k[0] * X + k[1] * Y + k[2] * Z, pv = k[3] * X + k[4] * Y + k[5] * Z, pw = k[6] * X + k[7] * Y + k[8] * Z;
    u = pu / (pw + 1e-6);
    v = pv / (pw + 1e-6);
}
