// Lens undistortion (include/rtm3d_hip.h, "lens undistortion"): rectifying maps built on the device and the bilinear remap of
// packed uint8 (h, w, 3) frames through them.  One launch per chunk of FRAME_CHUNK frames (frame_chunks.h; LENS_BUILD_BATCH maps), the
// descriptors travel by value (no copy, no memset, no synchronisation).
//
// Remap, thread mapping (rtm3d_frames_remap_plan returns the same numbers): a destination row is cut into runs of LENS_PX
// pixels; run t = blockIdx.x * LENS_THREADS + threadIdx.x of frame blockIdx.y covers pixels 4 * (t % runs_per_row) .. + 3 of
// row t / runs_per_row.  Consecutive lanes hold consecutive runs of a row: a wave reads 2 KB of map and writes 768 B of output
// in whole cache lines, and the 2 x 2 neighbourhoods it gathers lie next to each other wherever the map is smooth.
//
// The 32 map bytes of a full run are two 16-byte loads when the run's first entry is so aligned (always for an even wo on a
// 16-byte aligned map), dword loads otherwise.  A pixel whose four samples all lie inside the source reads each of its two
// source rows as the six consecutive bytes of two neighbouring pixels (a 4- and a 2-byte load at the bytes' own address: the
// device reads global memory at any alignment) - exactly those bytes, so no read leaves the source; a pixel at the border
// reads the samples that are inside and have a weight, byte by byte.  The 12 output bytes of a full run leave through
// store_rgb_run<4> (rgb_runs.h, shared with frames_convert.hip): as aligned dwords - shifted by the destination's
// misalignment, with a byte-wise head and tail - and a partial run (the row's last) byte by byte: exactly ho * wo * 3 bytes
// are written.
//
// Builder: one thread per destination pixel, fp64 in the header's operation order (this file is compiled with
// -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rtm3d_hip.h"
#include "frame_chunks.h"
#include "rgb_runs.h"

#define LENS_PX 4
#define LENS_THREADS 256
#define LENS_BUILD_BATCH 8
#define LENS_MAX_SIDE 16384

struct LensFrame {                       // 40 B
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* map;
    int h, w, ho, wo;
};
struct LensBatch { LensFrame f[FRAME_CHUNK]; uint32_t fill; };          // 1.3 KB of kernel arguments; fill = c0 | c1 << 8 | c2 << 16

// the 4 / 2 bytes at any address, low byte first
__device__ __forceinline__ uint32_t load4(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t load2(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

// one destination pixel as c0 | c1 << 8 | c2 << 16
__device__ __forceinline__ uint32_t remap_pixel(const LensFrame& f, int sx, int sy, uint32_t fill) {
    if (sx == INT32_MIN) return fill;
    const int ix = sx >> 5, ax = sx & 31, iy = sy >> 5, ay = sy & 31;
    const int w00 = (32 - ax) * (32 - ay), w10 = ax * (32 - ay), w01 = (32 - ax) * ay, w11 = ax * ay;
    uint32_t s00, s10, s01, s11;                                          // the samples' three bytes, as the result's
    if (ix >= 0 && ix < f.w - 1 && iy >= 0 && iy < f.h - 1) {             // all four inside: six bytes of each of two rows
        const uint8_t* p = f.src + ((size_t)iy * f.w + ix) * 3;
        const uint8_t* q = p + (size_t)f.w * 3;
        const uint32_t a = load4(p), b = load2(p + 4), c = load4(q), d = load2(q + 4);
        s00 = a & 0xffffffu; s10 = (a >> 24) | (b << 8);
        s01 = c & 0xffffffu; s11 = (c >> 24) | (d << 8);
    } else {
        s00 = s10 = s01 = s11 = fill;
        const bool x0 = ix >= 0 && ix < f.w, x1 = ix + 1 >= 0 && ix + 1 < f.w;      // (ix + 1 <= 2^26: no overflow)
        const bool y0 = iy >= 0 && iy < f.h, y1 = iy + 1 >= 0 && iy + 1 < f.h;
        if (y0) {
            const uint8_t* p = f.src + (size_t)iy * f.w * 3;
            if (x0 && w00) { const uint8_t* s = p + (size_t)ix * 3; s00 = s[0] | (s[1] << 8) | (s[2] << 16); }
            if (x1 && w10) { const uint8_t* s = p + (size_t)(ix + 1) * 3; s10 = s[0] | (s[1] << 8) | (s[2] << 16); }
        }
        if (y1) {
            const uint8_t* p = f.src + (size_t)(iy + 1) * f.w * 3;
            if (x0 && w01) { const uint8_t* s = p + (size_t)ix * 3; s01 = s[0] | (s[1] << 8) | (s[2] << 16); }
            if (x1 && w11) { const uint8_t* s = p + (size_t)(ix + 1) * 3; s11 = s[0] | (s[1] << 8) | (s[2] << 16); }
        }
    }
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        const int v = w00 * (int)((s00 >> sh) & 255u) + w10 * (int)((s10 >> sh) & 255u) + w01 * (int)((s01 >> sh) & 255u) +
                      w11 * (int)((s11 >> sh) & 255u) + 512;
        out |= (uint32_t)(v >> 10) << sh;                                 // <= 255: the weights sum to 1024
    }
    return out;
}

__global__ __launch_bounds__(LENS_THREADS) void frames_remap_kernel(LensBatch fb) {
    const LensFrame& f = fb.f[blockIdx.y];
    const unsigned per_row = (unsigned)(f.wo + LENS_PX - 1) / LENS_PX;
    const unsigned t = blockIdx.x * LENS_THREADS + threadIdx.x;          // < 2^26 + 256
    if (t >= per_row * (unsigned)f.ho) return;                            // (a frame smaller than the chunk's largest, and the last block)
    const unsigned y = t / per_row;
    const int x0 = (int)(t - y * per_row) * LENS_PX;
    const int n = min(LENS_PX, f.wo - x0);
    const size_t first = (size_t)y * f.wo + x0;
    const int32_t* m = f.map + 2 * first;
    int s[2 * LENS_PX];
    if (n == LENS_PX && ((uintptr_t)m & 15) == 0) {
        const int4 a = ((const int4*)m)[0], b = ((const int4*)m)[1];
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < 2 * LENS_PX; ++i) s[i] = i < 2 * n ? m[i] : INT32_MIN;
    }
    uint32_t px[LENS_PX];
#pragma unroll
    for (int i = 0; i < LENS_PX; ++i) px[i] = i < n ? remap_pixel(f, s[2 * i], s[2 * i + 1], fb.fill) : 0u;
    store_rgb_run<LENS_PX>(f.dst + first * 3, px, n);
}

// ---------------------------------------------------------------------------------------------------- the map builder
struct LensBuild {                       // 312 B
    rtm3d_lens_model m;
    rtm3d_lens_rect r;
    int32_t* map;
};
struct LensBuildBatch { LensBuild b[LENS_BUILD_BATCH]; };                // 2.5 KB of kernel arguments

__global__ __launch_bounds__(LENS_THREADS) void lens_map_build_kernel(LensBuildBatch bb) {
    const LensBuild& B = bb.b[blockIdx.y];
    const unsigned t = blockIdx.x * LENS_THREADS + threadIdx.x;          // < 2^28 + 256
    const int ho = B.r.ho, wo = B.r.wo;
    if (t >= (unsigned)ho * (unsigned)wo) return;
    const int v = (int)(t / (unsigned)wo), u = (int)(t - (unsigned)v * (unsigned)wo);
    const double* Kr = B.r.K;
    const double* R = B.r.R;
    const double* K = B.m.K;
    const double* k = B.m.dist;
    int32_t* out = B.map + 2 * (size_t)t;
    int sx = INT32_MIN, sy = INT32_MIN;
    const double a = ((double)u - Kr[2]) / Kr[0];
    const double b = ((double)v - Kr[5]) / Kr[4];
    const double X = R[0] * a + R[1] * b + R[2];
    const double Y = R[3] * a + R[4] * b + R[5];
    const double Wz = R[6] * a + R[7] * b + R[8];
    if (Wz > 0) {
        const double x = X / Wz, y = Y / Wz;
        double xd, yd;
        if (B.m.kind == RTM3D_LENS_BROWN) {
            const double r2 = x * x + y * y;
            const double num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
            const double den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
            const double cdist = num / den;
            xd = x * cdist + ((2 * k[2]) * x * y + k[3] * (r2 + (2 * x) * x));
            yd = y * cdist + (k[2] * (r2 + (2 * y) * y) + (2 * k[3]) * x * y);
        } else {
            const double r = sqrt(x * x + y * y);
            const double th = atan(r);
            const double t2 = th * th;
            const double td = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
            const double s = r > 1e-8 ? td / r : 1;
            xd = x * s; yd = y * s;
        }
        const double U = K[0] * xd + K[2];
        const double V = K[4] * yd + K[5];
        if (fabs(U) <= 1048576.0 && fabs(V) <= 1048576.0) {               // (false for a NaN or an infinity)
            sx = (int)floor(U * 32.0 + 0.5);
            sy = (int)floor(V * 32.0 + 0.5);
        }
    }
    out[0] = sx; out[1] = sy;
}

// ---------------------------------------------------------------------------------------------------- host
static bool side_ok(int v) { return v >= 1 && v <= LENS_MAX_SIDE; }

// the refusals that concern the maps alone (the plan has nothing else)
static int check_maps(const char* who, int B, const rtm3d_lens_map* h_maps) {
    if (refuse_count(who, B) || refuse_null(who, h_maps)) return 1;
    for (int b = 0; b < B; ++b) {
        const rtm3d_lens_map& m = h_maps[b];
        if (!m.d_map) { rt_set_error("%s: frame %d: the map is a NULL pointer", who, b); return 1; }
        if ((uintptr_t)m.d_map & 3) { rt_set_error("%s: frame %d: the map's address is no multiple of 4", who, b); return 1; }
        if (!side_ok(m.ho) || !side_ok(m.wo)) {
            rt_set_error("%s: frame %d: a map of %d x %d; a side must lie in 1..%d", who, b, m.ho, m.wo, LENS_MAX_SIDE); return 1;
        }
        if (refuse_reserved(who, b, m.reserved)) return 1;
    }
    return 0;
}

static rtm3d_remap_plan plan_chunk(const FrameChunk c, const rtm3d_lens_map* h_maps) {
    rtm3d_remap_plan P;
    P.first = c.b0; P.count = c.nb;
    P.px_per_thread = LENS_PX; P.threads = LENS_THREADS;
    P.runs = 0;
    for (int i = 0; i < c.nb; ++i) {
        const rtm3d_lens_map& m = h_maps[c.b0 + i];
        const int runs = ((m.wo + LENS_PX - 1) / LENS_PX) * m.ho;       // <= 4096 * 16384
        if (runs > P.runs) P.runs = runs;
    }
    P.grid_x = (P.runs + LENS_THREADS - 1) / LENS_THREADS;
    P.grid_y = c.nb;
    return P;
}

extern "C" int rtm3d_frames_remap_plan(int B, const rtm3d_lens_map* h_maps, rtm3d_remap_plan* out) {
    if (refuse_null("frames_remap_plan", out) || check_maps("frames_remap_plan", B, h_maps)) return 1;
    for (const FrameChunk c : frame_chunks(B)) out[c.k] = plan_chunk(c, h_maps);
    return 0;
}

extern "C" int rtm3d_frames_remap_check(int B, const uint8_t* const* h_src, const int* h_hw, const rtm3d_lens_map* h_maps,
                                        uint8_t* const* h_dst, const uint8_t fill[3]) {
    const char* who = "frames_remap";
    if (!h_src || !h_hw || !h_dst || !fill) { rt_set_error("%s: null pointer", who); return 1; }
    if (check_maps(who, B, h_maps)) return 1;
    for (int b = 0; b < B; ++b) {
        const int h = h_hw[2 * b], w = h_hw[2 * b + 1];
        if (!h_src[b]) { rt_set_error("%s: frame %d: the source is a NULL pointer", who, b); return 1; }
        if (refuse_null_dst(who, b, h_dst[b]) || refuse_side(who, b, h, w, 1, LENS_MAX_SIDE)) return 1;
        const uintptr_t s0 = (uintptr_t)h_src[b], s1 = s0 + (size_t)h * w * 3;
        const uintptr_t d0 = (uintptr_t)h_dst[b], d1 = d0 + (size_t)h_maps[b].ho * h_maps[b].wo * 3;
        if (d0 < s1 && s0 < d1) { rt_set_error("%s: frame %d: the destination overlaps its source", who, b); return 1; }
    }
    return 0;
}

extern "C" int rtm3d_frames_remap(void* stream, int B, const uint8_t* const* h_src, const int* h_hw, const rtm3d_lens_map* h_maps,
                                  uint8_t* const* h_dst, const uint8_t fill[3]) {
    if (rtm3d_frames_remap_check(B, h_src, h_hw, h_maps, h_dst, fill)) return 1;      // the whole batch, before the first launch
    for (const FrameChunk c : frame_chunks(B)) {
        const rtm3d_remap_plan plan = plan_chunk(c, h_maps);                           // the numbers of rtm3d_frames_remap_plan
        LensBatch fb;
        fb.fill = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16);
        for (int i = 0; i < FRAME_CHUNK; ++i) {
            LensFrame& f = fb.f[i];
            if (i >= c.nb) { f = LensFrame{nullptr, nullptr, nullptr, 0, 0, 0, 0}; continue; }
            const int b = c.b0 + i;
            f.src = h_src[b]; f.dst = h_dst[b]; f.map = h_maps[b].d_map;
            f.h = h_hw[2 * b]; f.w = h_hw[2 * b + 1];
            f.ho = h_maps[b].ho; f.wo = h_maps[b].wo;
        }
        hipLaunchKernelGGL(frames_remap_kernel, dim3((unsigned)plan.grid_x, (unsigned)plan.grid_y), dim3(LENS_THREADS), 0,
                           (hipStream_t)stream, fb);
    }
    return launch_ok("frames_remap");
}

// no skew, bottom row 0 0 1, positive focal lengths
static const char* bad_k(const double* K) {
    if (K[1] != 0 || K[3] != 0) return "an entry [1] or [3] that is not 0 (skew is not modelled)";
    if (K[6] != 0 || K[7] != 0 || K[8] != 1) return "a bottom row that is not 0 0 1";
    if (!(K[0] > 0) || !(K[4] > 0)) return "fx or fy that is not > 0";
    return nullptr;
}

extern "C" int rtm3d_lens_map_build(void* stream, int n, const rtm3d_lens_model* h_models, const rtm3d_lens_rect* h_rect,
                                    int32_t* const* h_maps) {
    const char* who = "lens_map_build";
    if (n < 1) { rt_set_error("%s: n = %d", who, n); return 1; }
    if (!h_models || !h_rect || !h_maps) { rt_set_error("%s: null pointer", who); return 1; }
    for (int i = 0; i < n; ++i) {
        const rtm3d_lens_model& m = h_models[i];
        const rtm3d_lens_rect& r = h_rect[i];
        if (m.kind != RTM3D_LENS_BROWN && m.kind != RTM3D_LENS_FISHEYE) { rt_set_error("%s: map %d: unknown lens kind %d", who, i, m.kind); return 1; }
        if (!side_ok(m.h) || !side_ok(m.w)) {
            rt_set_error("%s: map %d: a lens of %d x %d; a side must lie in 1..%d", who, i, m.h, m.w, LENS_MAX_SIDE); return 1;
        }
        if (!side_ok(r.ho) || !side_ok(r.wo)) {
            rt_set_error("%s: map %d: a map of %d x %d; a side must lie in 1..%d", who, i, r.ho, r.wo, LENS_MAX_SIDE); return 1;
        }
        if (const char* why = bad_k(m.K)) { rt_set_error("%s: map %d: K has %s", who, i, why); return 1; }
        if (const char* why = bad_k(r.K)) { rt_set_error("%s: map %d: the rectified K has %s", who, i, why); return 1; }
        if (m.kind == RTM3D_LENS_FISHEYE && (m.dist[4] != 0 || m.dist[5] != 0 || m.dist[6] != 0 || m.dist[7] != 0)) {
            rt_set_error("%s: map %d: a fisheye lens has four coefficients, dist[4:8] must be 0", who, i); return 1;
        }
        if (!h_maps[i]) { rt_set_error("%s: map %d: the map is a NULL pointer", who, i); return 1; }
        if ((uintptr_t)h_maps[i] & 3) { rt_set_error("%s: map %d: the map's address is no multiple of 4", who, i); return 1; }
    }
    for (int i0 = 0; i0 < n; i0 += LENS_BUILD_BATCH) {
        const int nb = n - i0 < LENS_BUILD_BATCH ? n - i0 : LENS_BUILD_BATCH;
        LensBuildBatch bb;
        memset(&bb, 0, sizeof bb);                                        // (an unused entry has 0 x 0 pixels)
        int px = 0;
        for (int i = 0; i < nb; ++i) {
            bb.b[i].m = h_models[i0 + i]; bb.b[i].r = h_rect[i0 + i]; bb.b[i].map = h_maps[i0 + i];
            const int p = h_rect[i0 + i].ho * h_rect[i0 + i].wo;           // <= 2^28
            if (p > px) px = p;
        }
        hipLaunchKernelGGL(lens_map_build_kernel, dim3((unsigned)((px + LENS_THREADS - 1) / LENS_THREADS), (unsigned)nb), dim3(LENS_THREADS),
                           0, (hipStream_t)stream, bb);
    }
    return launch_ok(who);
}
