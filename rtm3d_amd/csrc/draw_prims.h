// Device helpers shared by the two drawing kernels (draw.hip: records_draw_kernel; draw_tracks.hip: draw_tracks_kernel): the
// tile geometry, the batch descriptor with the host function that fills it (draw_fill_batch), the coordinate rule and the exact
// integer coverage tests of include/rtm3d_hip.h, "drawing".  Integer ranges: draw.hip.
#pragma once
#include "common.h"
#include "box_project.h"
#include "../../include/rtm3d_hip.h"

#define DRAW_MAX_BATCH 64
#define DRAW_TW 64
#define DRAW_TH 16
#define DRAW_THREADS 256
#define DRAW_PRIMS 18                  // per slot in a frame: face, 4 box sides, 12 edges, disc
#define DRAW_BEV_PRIMS 5               // per slot in a panel: 4 outline segments, heading mark
#define DRAW_MAX_SIDE 8192
#define DRAW_MAX_RADIUS 64
#define DRAW_FRAME_LAYERS (RTM3D_DRAW_FACE | RTM3D_DRAW_BOX2D | RTM3D_DRAW_WIREFRAME | RTM3D_DRAW_KEYPOINT)

struct DrawBatch {
    uint8_t* img[DRAW_MAX_BATCH];
    int h[DRAW_MAX_BATCH], w[DRAW_MAX_BATCH];
    int tile0[DRAW_MAX_BATCH + 1];     // first workgroup of frame i; [nb] = first workgroup of the panels
};

// host: the descriptor of the nb frames from b0 on (unused entries empty); `frames` = a frame layer is set, so the frames get
// workgroups.  Returns the workgroups of the frames = the first workgroup of the panels.
static inline int draw_fill_batch(DrawBatch& fb, uint8_t* const* h_imgs, const int* h_hw, int b0, int nb, bool frames) {
    int tiles = 0;
    for (int i = 0; i < nb; ++i) {
        fb.img[i] = h_imgs[b0 + i]; fb.h[i] = h_hw[2 * (b0 + i)]; fb.w[i] = h_hw[2 * (b0 + i) + 1];
        fb.tile0[i] = tiles;
        if (frames) tiles += ((fb.w[i] + DRAW_TW - 1) / DRAW_TW) * ((fb.h[i] + DRAW_TH - 1) / DRAW_TH);
    }
    for (int i = nb; i < DRAW_MAX_BATCH; ++i) { fb.img[i] = nullptr; fb.h[i] = 0; fb.w[i] = 0; fb.tile0[i] = tiles; }
    fb.tile0[nb] = tiles;
    fb.tile0[DRAW_MAX_BATCH] = tiles;
    return tiles;
}

// truncation toward zero of a coordinate whose integer lies in [-8192, 8192]; false for anything else (NaN and infinities too)
__device__ __forceinline__ bool draw_coord(double v, int& o) {
    if (!(v > -(double)(DRAW_MAX_SIDE + 1) && v < (double)(DRAW_MAX_SIDE + 1))) return false;
    o = (int)v;
    return true;
}

// vertex vi of a slot: source 0 the regressed vertex, source 1 corner vi of the solved box through K
__device__ __forceinline__ bool draw_vertex(const float* __restrict__ r, const double* __restrict__ xs, const double* __restrict__ k,
                                            double sn, double cs, int source, int vi, int& x, int& y) {
    double u, v;
    if (source == 0) { u = (double)r[4 + 2 * vi]; v = (double)r[5 + 2 * vi]; }
    else box_project_corner(xs, k, sn, cs, vi, u, v);
    const bool a = draw_coord(u, x), b = draw_coord(v, y);
    return a && b;
}

__device__ __forceinline__ bool seg_covers(int px, int py, int x0, int y0, int x1, int y1, int t2) {
    const int dx = x1 - x0, dy = y1 - y0;
    int vx = px - x0, vy = py - y0;
    const int dd = dx * dx + dy * dy, k = vx * dx + vy * dy;
    if (k <= 0 || k >= dd) {
        if (k > 0) { vx = px - x1; vy = py - y1; }
        return 4ll * (long long)(vx * vx + vy * vy) <= (long long)t2;
    }
    const long long cr = (long long)(2 * (vx * dy - vy * dx));
    return cr * cr <= (long long)t2 * (long long)dd;
}

__device__ __forceinline__ bool tri_covers(int px, int py, int ax, int ay, int bx, int by, int cx, int cy) {
    if ((bx - ax) * (cy - ay) - (by - ay) * (cx - ax) == 0) return false;
    const int e0 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    const int e1 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
    const int e2 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx);
    return (e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0);
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// a panel point: local (lx, lz) of the footprint around (X, Z), heading (c, sn), through the bird's-eye mapping
__device__ __forceinline__ bool draw_bev_point(double c, double sn, double lx, double lz, double X, double Z, int bev_h, int bev_w, double m,
                                               int& x, int& y) {
    const double wx = (c * lx + sn * lz) + X, wz = (c * lz - sn * lx) + Z;
    const double u = (double)bev_w / 2.0 + wx / m, v = (double)bev_h - wz / m;
    const bool a = draw_coord(u, x), b = draw_coord(v, y);
    return a && b;
}

// the argument checks of rtm3d_records_draw (draw.hip), shared with rtm3d_records_draw_tracks: `max_layers` the largest mask
// accepted, `layer_words` how the message counts them, `panels` whether a panel layer is set.  Non-zero = refused, reason set.
int draw_check_args(int B, int topk, const float* d_rec, uint8_t* const* h_imgs, const int* h_hw, const double* d_K_camera,
                    const rtm3d_draw_params* params, const uint8_t* d_bev, int max_layers, const char* layer_words, bool panels);
