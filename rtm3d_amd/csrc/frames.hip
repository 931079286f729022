// Bookkeeping on both ends of a detect step fed by camera frames (include/rtm3d_hip.h, "camera frames"):
//   rtm3d_frames_adjust_k      the camera's intrinsics -> the intrinsics of the network canvas: ToPercentCoords -> Resize ->
//                              ToAbsoluteCoords (preprocess/transforms.py:146-176), then the letterbox shift of the principal
//                              point (datasets/dataset_reader.py:189-193) - preprocess.resize_K / adjust_K in fp64;
//   rtm3d_records_to_camera    the 2D fields of the detection records back from canvas pixels to the pixels of the camera
//                              frame, and the numbers of a KITTI label line (rtm3d_amd/kitti_results.py) per kept box.
// The per-image geometry travels as a by-value kernel argument in chunks of FRAMES_MAX_BATCH images, like PreBatch of
// preprocess.hip: no copy, no memset.  Compiled with -ffp-contract=off: every result is a fixed sequence of IEEE operations.
#include "common.h"
#include "box_project.h"
#include "../../include/rtm3d_hip.h"

#define FRAMES_MAX_BATCH 64
struct FrameBatch {
    rtm3d_frame_geom g[FRAMES_MAX_BATCH];
};

// one thread per (image, element of K); numpy's order: row 0 /= w, row 1 /= h, row 0 *= w', row 1 *= h' (executed even when
// the sizes are equal), then cx += pad_w, cy += pad_h; row 2 untouched
__global__ __launch_bounds__(256) void frames_adjust_K_kernel(const FrameBatch fb, int nb, const double* __restrict__ K_camera,
                                                             double* __restrict__ K_net) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nb * 9) return;
    const int b = t / 9, e = t - b * 9;
    const rtm3d_frame_geom g = fb.g[b];
    double v = K_camera[t];
    if (e < 3) { v = v / (double)g.w; v = v * (double)g.rw; }
    else if (e < 6) { v = v / (double)g.h; v = v * (double)g.rh; }
    if (e == 2) v = v + (double)g.pad_w;
    if (e == 5) v = v + (double)g.pad_h;
    K_net[t] = v;
}

// One thread per float of a record (32 per slot, so the lanes of a slot share a wave).  In place: a thread rewrites only
// the float it read; the flag [31] that every lane of the slot reads is never rewritten.
//   fields [2:24] of live slots: x -> (x - pad_w) * (w / w'), y -> (y - pad_h) * (h / h') in fp64, rounded once to fp32
//   (x at the even fields: key point, vertices and box all alternate x, y from an even offset);
//   KITTI row of a kept slot (16 fp64): lanes 0..7 project one corner each through the camera's K, the rectangle is an
//   xor-shuffle min / max over those 8 lanes (order-free, so exact), lanes 0..15 store one element each.
__global__ __launch_bounds__(256) void records_to_camera_kernel(const FrameBatch fb, int total, int topk, float* __restrict__ rec,
                                                               const double* __restrict__ K_camera, const double* __restrict__ x,
                                                               const double* __restrict__ fun, const int32_t* __restrict__ status,
                                                               double fun_accept, double* __restrict__ kitti) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;                       // total is a multiple of 32: whole slots leave together
    const int slot = t >> 5, f = t & 31;
    const int img = slot / topk;
    const rtm3d_frame_geom g = fb.g[img];
    const float flag = rec[(size_t)slot * 32 + 31];
    if (flag >= 1.0f && f >= 2 && f < 24) {
        const bool is_x = (f & 1) == 0;
        const double pad = is_x ? (double)g.pad_w : (double)g.pad_h;
        const double scale = is_x ? (double)g.w / (double)g.rw : (double)g.h / (double)g.rh;
        rec[t] = (float)(((double)rec[t] - pad) * scale);
    }
    if (!kitti) return;
    // a row only where the RECORD says kept (flag 2; rtm3d_records_nms3d turns the flag of a suppressed slot 2 -> 1 and leaves
    // the solver outputs alone) and the solver outputs agree; uniform over the slot's 32 lanes
    const bool kept = flag == 2.0f && status[slot] >= 0 && fun[slot] < fun_accept;
    double out = 0.0;
    if (kept) {
        const double* xs = x + (size_t)slot * 8;
        double sn, cs, u, v;
        const double ry = box_yaw(xs, sn, cs);
        box_project_corner(xs, K_camera + (size_t)img * 9, sn, cs, f & 7, u, v);
        double x1 = u, y1 = v, x2 = u, y2 = v;
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {
            x1 = fmin(x1, __shfl_xor(x1, m)); y1 = fmin(y1, __shfl_xor(y1, m));
            x2 = fmax(x2, __shfl_xor(x2, m)); y2 = fmax(y2, __shfl_xor(y2, m));
        }
        const double xmax = (double)(g.w - 1), ymax = (double)(g.h - 1);
        const double hh = xs[3];
        switch (f) {
        case 0: out = (double)rec[(size_t)slot * 32]; break;                            // class
        case 1: {                                                                        // alpha = ry - atan2(x, z) in [-pi, pi)
            const double pi = 3.141592653589793;
            double a = fmod(ry - atan2(xs[5], xs[7]) + pi, 2 * pi);
            if (a < 0.0) a += 2 * pi;
            out = a - pi;
            break;
        }
        case 2: out = fmin(fmax(x1, 0.0), xmax); break;
        case 3: out = fmin(fmax(y1, 0.0), ymax); break;
        case 4: out = fmin(fmax(x2, 0.0), xmax); break;
        case 5: out = fmin(fmax(y2, 0.0), ymax); break;
        case 6: out = hh; break;                                                         // dimension (h, w, l) = x[3], x[4], x[2]
        case 7: out = xs[4]; break;
        case 8: out = xs[2]; break;
        case 9: out = xs[5]; break;
        case 10: out = xs[6] + hh / 2.0; break;                                          // centre -> bottom face
        case 11: out = xs[7]; break;
        case 12: out = ry; break;
        case 13: out = (double)rec[(size_t)slot * 32 + 1]; break;                        // score
        case 14: out = 2.0; break;
        default: out = 0.0;
        }
    }
    if (f < 16) kitti[(size_t)slot * 16 + f] = out;
}

extern void rt_set_error(const char* fmt, ...);

// every frame of the whole batch, before the first launch: a refusal leaves nothing rewritten
static int check_geom(const char* what, const rtm3d_frame_geom* h_geom, int B) {
    for (int i = 0; i < B; ++i) {
        const rtm3d_frame_geom& g = h_geom[i];
        if (g.h < 1 || g.w < 1 || g.rh < 1 || g.rw < 1) {
            rt_set_error("%s: frame %d has an empty size (%dx%d -> %dx%d)", what, i, g.h, g.w, g.rh, g.rw);
            return 1;
        }
    }
    return 0;
}

static void fill_batch(FrameBatch& fb, const rtm3d_frame_geom* h_geom, int b0, int nb) {
    for (int i = 0; i < nb; ++i) fb.g[i] = h_geom[b0 + i];
}

extern "C" int rtm3d_frames_adjust_k(void* stream, int B, const rtm3d_frame_geom* h_geom, const double* d_K_camera, double* d_K_net) {
    if (B < 1 || !h_geom || !d_K_camera || !d_K_net) { rt_set_error("frames_adjust_K: bad arguments"); return 1; }
    if (check_geom("frames_adjust_K", h_geom, B)) return 1;
    for (int b0 = 0; b0 < B; b0 += FRAMES_MAX_BATCH) {
        const int nb = B - b0 < FRAMES_MAX_BATCH ? B - b0 : FRAMES_MAX_BATCH;
        FrameBatch fb;
        fill_batch(fb, h_geom, b0, nb);
        hipLaunchKernelGGL(frames_adjust_K_kernel, dim3((nb * 9 + 255) / 256), dim3(256), 0, (hipStream_t)stream, fb, nb,
                           d_K_camera + (size_t)b0 * 9, d_K_net + (size_t)b0 * 9);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("frames_adjust_K launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int rtm3d_records_to_camera(void* stream, int B, int topk, const rtm3d_frame_geom* h_geom, float* d_rec,
                                       const double* d_K_camera, const double* d_x, const double* d_fun, const int32_t* d_status,
                                       double fun_accept, double* d_kitti) {
    if (B < 1 || topk < 1 || !h_geom || !d_rec) { rt_set_error("records_to_camera: bad arguments"); return 1; }
    if (d_kitti && (!d_K_camera || !d_x || !d_fun || !d_status)) {
        rt_set_error("records_to_camera: the KITTI rows need the camera intrinsics and the solver outputs"); return 1;
    }
    if (check_geom("records_to_camera", h_geom, B)) return 1;
    for (int b0 = 0; b0 < B; b0 += FRAMES_MAX_BATCH) {
        const int nb = B - b0 < FRAMES_MAX_BATCH ? B - b0 : FRAMES_MAX_BATCH;
        FrameBatch fb;
        fill_batch(fb, h_geom, b0, nb);
        const size_t s0 = (size_t)b0 * topk;                   // first slot of the chunk
        const int total = nb * topk * 32;
        hipLaunchKernelGGL(records_to_camera_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, fb, total, topk,
                           d_rec + s0 * 32, d_kitti ? d_K_camera + (size_t)b0 * 9 : nullptr, d_kitti ? d_x + s0 * 8 : nullptr,
                           d_kitti ? d_fun + s0 : nullptr, d_kitti ? d_status + s0 : nullptr, fun_accept,
                           d_kitti ? d_kitti + s0 * 16 : nullptr);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("records_to_camera launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
