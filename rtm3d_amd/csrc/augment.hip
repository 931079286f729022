// Training augmentation (include/rtm3d_hip.h, "training augmentation"): B packed uint8 (h, w, 3) frames -> the network canvas in
// one pass - brightness / contrast and Philox noise on the source bytes, one bilinear resample through the composed Resize,
// RandomAffine and RandomMirror map, mean-colour letterbox, normalisation tables.  Per chunk of FRAME_CHUNK frames (frame_chunks.h) one interior
// launch (the placed rectangles and their channel sums) and one border launch (the pad colour); the descriptors travel by value
// (2.8 KB of kernel arguments), no copy, no synchronisation.  Integer code on the device: no float arithmetic, no float atomics.
//
// Thread mapping (rtm3d_frames_augment_plan returns the same numbers): a canvas row is cut into runs of AUG_PX pixels that begin
// at X = 4 * k - shift; interior thread t of frame blockIdx.y takes run t % runs_per_row of rectangle row t / runs_per_row and
// makes the pixels of the run that lie inside the rectangle.  Consecutive lanes hold consecutive runs of a row: a wave writes
// whole cache lines (2 KB of NHWC4, 1 KB per fp32 plane, 768 B of packed RGB) and the 2 x 2 neighbourhoods it gathers lie next
// to each other.  A pixel whose four taps lie inside the source reads each of its two source rows as the six consecutive bytes
// of two neighbouring pixels (lens.hip's gather); at the source's last row / column the taps that carry a weight, byte by byte.
// A full run leaves as 2 x 16 B (mode 1: shift makes the run's first pixel an even one of the tensor row), 16 B per plane (mode
// 0, where W and the base allow it) or through store_rgb_run<4> (mode 2); a run cut by the rectangle's edge pixel by pixel.
// Channel sums: registers -> wave butterfly -> LDS -> one 64-bit atomic per workgroup and channel.
//
// The host functions (noise table, geometry, plan, check) touch no device; the geometry is fp64 in the header's operation order
// (this file is compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rtm3d_hip.h"
#include "frame_chunks.h"
#include "philox.h"
#include "rgb_runs.h"

#define AUG_PX 4
#define AUG_THREADS 256
#define AUG_MAX_SIDE 16384
#define AUG_BORDER_GRID 512

struct AugFrame {                        // 88 B
    const uint8_t* src;
    rtm3d_augment_frame f;
};
struct AugBatch { AugFrame f[FRAME_CHUNK]; };                             // 2.8 KB of kernel arguments

// the 4 / 2 bytes at any address, low byte first
__device__ __forceinline__ uint32_t aug_load4(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t aug_load2(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
__device__ __forceinline__ uint32_t aug_load3(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }
__device__ __forceinline__ int aug_clamp255(int v) { return min(max(v, 0), 255); }

// brightness / contrast of the three bytes of s
__device__ __forceinline__ uint32_t aug_photo(uint32_t s, int alpha_q, int beta_q) {
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t v = (int64_t)((s >> (8 * c)) & 255u);
        o |= (uint32_t)aug_clamp255((int)((v * alpha_q + beta_q) >> 16)) << (8 * c);
    }
    return o;
}

// the noise of source pixel p added to the three bytes of s
__device__ __forceinline__ uint32_t aug_noise(uint32_t s, uint32_t p, uint32_t k0, uint32_t k1, int sigma_q, const int16_t* T_s) {
    uint32_t r[4];
    philox4x32_10(p, 0u, 0u, 0u, k0, k1, r);
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int n = ((int)T_s[r[c] >> 20] * sigma_q + 32768) >> 16;
        o |= (uint32_t)aug_clamp255((int)((s >> (8 * c)) & 255u) + n) << (8 * c);
    }
    return o;
}

// one rectangle pixel as c0 | c1 << 8 | c2 << 16; qx = x * ax + bx, qy = y * ay + by
__device__ __forceinline__ uint32_t aug_pixel(const AugFrame& F, int64_t qx, int64_t qy, const int16_t* T_s, uint32_t fill) {
    const rtm3d_augment_frame& f = F.f;
    const int h = f.h, w = f.w;
    const int64_t sx64 = qx >> 16, sy64 = qy >> 16;
    if (sx64 <= -32 || sx64 >= 32 * (int64_t)w || sy64 <= -32 || sy64 >= 32 * (int64_t)h) return fill;
    const int sx = (int)min(max(sx64, (int64_t)0), (int64_t)32 * (w - 1));
    const int sy = (int)min(max(sy64, (int64_t)0), (int64_t)32 * (h - 1));
    const int ix = sx >> 5, fx = sx & 31, iy = sy >> 5, fy = sy & 31;   // 0 <= ix <= w - 1, 0 <= iy <= h - 1
    const int w00 = (32 - fx) * (32 - fy), w10 = fx * (32 - fy), w01 = (32 - fx) * fy, w11 = fx * fy;
    const uint32_t p00 = (uint32_t)iy * (uint32_t)w + (uint32_t)ix;     // < 2^28
    const uint8_t* p = F.src + (size_t)p00 * 3;
    uint32_t s00, s10 = 0, s01 = 0, s11 = 0;
    if (ix < w - 1 && iy < h - 1) {                                      // all four inside: six bytes of each of two rows
        const uint8_t* q = p + (size_t)w * 3;
        const uint32_t a = aug_load4(p), b = aug_load2(p + 4), c = aug_load4(q), d = aug_load2(q + 4);
        s00 = a & 0xffffffu; s10 = (a >> 24) | (b << 8);
        s01 = c & 0xffffffu; s11 = (c >> 24) | (d << 8);
    } else {                                                             // the last row / column: fx == 0 / fy == 0 there
        const bool x1 = ix + 1 < w, y1 = iy + 1 < h;
        s00 = aug_load3(p);
        if (x1 && w10) s10 = aug_load3(p + 3);
        if (y1 && w01) s01 = aug_load3(p + (size_t)w * 3);
        if (x1 && y1 && w11) s11 = aug_load3(p + (size_t)w * 3 + 3);
    }
    if (f.alpha_q != 65536 || f.beta_q != 0) {
        s00 = aug_photo(s00, f.alpha_q, f.beta_q); s10 = aug_photo(s10, f.alpha_q, f.beta_q);
        s01 = aug_photo(s01, f.alpha_q, f.beta_q); s11 = aug_photo(s11, f.alpha_q, f.beta_q);
    }
    if (f.sigma_q != 0) {                                                // (a tap without a weight draws nothing)
        s00 = aug_noise(s00, p00, f.seed_lo, f.seed_hi, f.sigma_q, T_s);
        if (w10) s10 = aug_noise(s10, p00 + 1u, f.seed_lo, f.seed_hi, f.sigma_q, T_s);
        if (w01) s01 = aug_noise(s01, p00 + (uint32_t)w, f.seed_lo, f.seed_hi, f.sigma_q, T_s);
        if (w11) s11 = aug_noise(s11, p00 + (uint32_t)w + 1u, f.seed_lo, f.seed_hi, f.sigma_q, T_s);
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

// ---- the stores of n <= 4 pixels that begin at canvas pixel (X, Y) of frame b; full = a whole run
// MODE 0: fp32 NCHW through lut_s [3][256]
__device__ __forceinline__ void aug_store_f32(float* out, int b, int Y, int X, int H, int W, const float* lut_s, const uint32_t (&px)[AUG_PX],
                                              int n) {
    const size_t plane = (size_t)H * W;
    float* o = out + (size_t)b * 3 * plane + (size_t)Y * W + X;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* oc = o + c * plane;
        const float v0 = lut_s[c * 256 + ((px[0] >> (8 * c)) & 255u)], v1 = lut_s[c * 256 + ((px[1] >> (8 * c)) & 255u)];
        const float v2 = lut_s[c * 256 + ((px[2] >> (8 * c)) & 255u)], v3 = lut_s[c * 256 + ((px[3] >> (8 * c)) & 255u)];
        if (n == AUG_PX && ((uintptr_t)oc & 15) == 0) {
            *(float4*)oc = make_float4(v0, v1, v2, v3);
        } else {
            if (n > 0) oc[0] = v0;
            if (n > 1) oc[1] = v1;
            if (n > 2) oc[2] = v2;
            if (n > 3) oc[3] = v3;
        }
    }
}

// MODE 1: fp16 NHWC4 with border P through lut_s [3][256] (bit patterns), 4th channel 0
__device__ __forceinline__ uint2 aug_half4(const uint16_t* lut_s, uint32_t px) {
    return make_uint2((uint32_t)lut_s[px & 255u] | ((uint32_t)lut_s[256 + ((px >> 8) & 255u)] << 16), (uint32_t)lut_s[512 + ((px >> 16) & 255u)]);
}
__device__ __forceinline__ void aug_store_f16(uint16_t* out, int b, int Y, int X, int H, int W, int P, const uint16_t* lut_s,
                                              const uint32_t (&px)[AUG_PX], int n) {
    uint2* o = (uint2*)(out + (((size_t)b * (H + 2 * P) + Y + P) * (W + 2 * P) + X + P) * 4);
    const uint2 v0 = aug_half4(lut_s, px[0]), v1 = aug_half4(lut_s, px[1]), v2 = aug_half4(lut_s, px[2]), v3 = aug_half4(lut_s, px[3]);
    if (n == AUG_PX && ((uintptr_t)o & 15) == 0) {
        ((uint4*)o)[0] = make_uint4(v0.x, v0.y, v1.x, v1.y);
        ((uint4*)o)[1] = make_uint4(v2.x, v2.y, v3.x, v3.y);
    } else {
        if (n > 0) o[0] = v0;
        if (n > 1) o[1] = v1;
        if (n > 2) o[2] = v2;
        if (n > 3) o[3] = v3;
    }
}

template <int MODE>
__device__ __forceinline__ void aug_store(void* out, int b, int Y, int X, int H, int W, int P, const void* lut_s, const uint32_t (&px)[AUG_PX],
                                          int n) {
    if (MODE == 0) aug_store_f32((float*)out, b, Y, X, H, W, (const float*)lut_s, px, n);
    else if (MODE == 1) aug_store_f16((uint16_t*)out, b, Y, X, H, W, P, (const uint16_t*)lut_s, px, n);
    else store_rgb_run<AUG_PX>((uint8_t*)out + (((size_t)b * H + Y) * W + X) * 3, px, n);
}

// the normalisation table of the mode into LDS (mode 2: none)
template <int MODE>
__device__ __forceinline__ void aug_stage_lut(uint32_t* lut_s, const float* __restrict__ lut, const uint16_t* __restrict__ lut16) {
    if (MODE == 0) for (int i = threadIdx.x; i < 768; i += AUG_THREADS) ((float*)lut_s)[i] = lut[i];
    if (MODE == 1) for (int i = threadIdx.x; i < 768; i += AUG_THREADS) ((uint16_t*)lut_s)[i] = lut16[i];
}

template <int MODE>
__global__ __launch_bounds__(AUG_THREADS) void augment_interior_kernel(const AugBatch ab, void* __restrict__ out, int first, int H, int W, int P,
                                                                      int shift, const int16_t* __restrict__ T, const float* __restrict__ lut,
                                                                      const uint16_t* __restrict__ lut16, unsigned long long* __restrict__ sums) {
    __shared__ int16_t T_s[4096];
    __shared__ uint32_t lut_s[768];
    __shared__ unsigned int red[3][AUG_THREADS / 64];
    const AugFrame& F = ab.f[blockIdx.y];
    const rtm3d_augment_frame& f = F.f;
    const int b = first + (int)blockIdx.y;
    if (f.sigma_q != 0) for (int i = threadIdx.x; i < 4096; i += AUG_THREADS) T_s[i] = T[i];
    aug_stage_lut<MODE>(lut_s, lut, lut16);
    __syncthreads();
    const int k_lo = (f.x0 + shift) >> 2, k_hi = (f.x0 + f.rw - 1 + shift) >> 2;
    const unsigned per_row = (unsigned)(k_hi - k_lo + 1);
    const unsigned t = blockIdx.x * AUG_THREADS + threadIdx.x;           // < 2^26 + 256
    unsigned int s0 = 0, s1 = 0, s2 = 0;
    if (t < per_row * (unsigned)f.rh) {                                   // (a frame smaller than the chunk's largest, and the last block)
        const unsigned row = t / per_row;
        const int xrun = (k_lo + (int)(t - row * per_row)) * AUG_PX - shift;
        const int lo = max(xrun, f.x0), hi = min(xrun + AUG_PX, f.x0 + f.rw);
        const int n = hi - lo;                                            // 1..4
        const uint32_t fill = (uint32_t)f.fill[0] | ((uint32_t)f.fill[1] << 8) | ((uint32_t)f.fill[2] << 16);
        const int64_t qy = (int64_t)row * f.ay + f.by;
        int64_t qx = (int64_t)(lo - f.x0) * f.ax + f.bx;
        uint32_t px[AUG_PX];
#pragma unroll
        for (int i = 0; i < AUG_PX; ++i) {
            px[i] = i < n ? aug_pixel(F, qx, qy, T_s, fill) : 0u;
            qx += f.ax;
            s0 += px[i] & 255u; s1 += (px[i] >> 8) & 255u; s2 += px[i] >> 16;
        }
        aug_store<MODE>(out, b, f.y0 + (int)row, lo, H, W, P, lut_s, px, n);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off); s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s0; red[1][threadIdx.x >> 6] = s1; red[2][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long v = 0;
        for (int i = 0; i < AUG_THREADS / 64; ++i) v += red[threadIdx.x][i];
        atomicAdd(&sums[(size_t)b * 3 + threadIdx.x], v);
    }
}

// border: every run of the canvas, the pixels outside the rectangle in the rectangle's truncated mean colour
template <int MODE>
__global__ __launch_bounds__(AUG_THREADS) void augment_border_kernel(const AugBatch ab, void* __restrict__ out, int first, int H, int W, int P,
                                                                    int shift, int runs_per_row, const float* __restrict__ lut,
                                                                    const uint16_t* __restrict__ lut16,
                                                                    const unsigned long long* __restrict__ sums) {
    __shared__ uint32_t lut_s[768];
    const rtm3d_augment_frame& f = ab.f[blockIdx.y].f;
    const int b = first + (int)blockIdx.y;
    aug_stage_lut<MODE>(lut_s, lut, lut16);
    __syncthreads();
    const unsigned long long npix = (unsigned long long)f.rw * (unsigned long long)f.rh;
    const uint32_t m = (uint32_t)(sums[(size_t)b * 3] / npix) | ((uint32_t)(sums[(size_t)b * 3 + 1] / npix) << 8) |
                       ((uint32_t)(sums[(size_t)b * 3 + 2] / npix) << 16);
    const uint32_t px[AUG_PX] = {m, m, m, m};
    const int x1 = f.x0 + f.rw, y1 = f.y0 + f.rh;
    const unsigned total = (unsigned)H * (unsigned)runs_per_row;          // <= 16384 * 4097
    for (unsigned r = blockIdx.x * AUG_THREADS + threadIdx.x; r < total; r += gridDim.x * AUG_THREADS) {
        const int Y = (int)(r / (unsigned)runs_per_row);
        const int xrun = (int)(r - (unsigned)Y * (unsigned)runs_per_row) * AUG_PX - shift;
        const int lo = max(xrun, 0), hi = min(xrun + AUG_PX, W);
        const bool rowin = Y >= f.y0 && Y < y1;
        if (rowin && lo >= f.x0 && hi <= x1) continue;                    // the rectangle's own
        if (!rowin || hi <= f.x0 || lo >= x1) {                           // none of the rectangle's: the run as it is
            aug_store<MODE>(out, b, Y, lo, H, W, P, lut_s, px, hi - lo);
        } else {                                                          // cut by a vertical edge (a narrow rectangle: by both)
            for (int X = lo; X < hi; ++X)
                if (X < f.x0 || X >= x1) aug_store<MODE>(out, b, Y, X, H, W, P, lut_s, px, 1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host
// Phi^-1(p), 0 < p < 1: Newton steps on Phi(x) - p from the inflection point, on the side where Phi is convex (p < 1/2: the
// iterates fall monotonically onto the root), the other half by symmetry.  Phi through erfc, which keeps its relative accuracy
// in the tail.
static double inv_normal_cdf(double p) {
    if (p > 0.5) return -inv_normal_cdf(1.0 - p);
    if (p == 0.5) return 0.0;
    double x = 0.0;
    for (int it = 0; it < 200; ++it) {
        const double F = 0.5 * erfc(-x * 0.70710678118654752440) - p;
        const double d = 0.39894228040143267794 * exp(-0.5 * x * x);
        const double step = F / d;
        x -= step;
        if (fabs(step) <= 1e-15 * fabs(x)) break;
    }
    return x;
}

extern "C" int rtm3d_augment_noise_table(int16_t out[4096]) {
    if (!out) { rt_set_error("augment_noise_table: null pointer"); return 1; }
    for (int k = 0; k < 2048; ++k) {                                     // (k + 0.5) / 4096 is exact, and so is its complement
        const double v = 1024.0 * inv_normal_cdf(((double)k + 0.5) / 4096.0);
        const int16_t q = (int16_t)floor(v + 0.5);                       // (no entry lies near a tie)
        out[k] = q; out[4095 - k] = (int16_t)-q;
    }
    return 0;
}

// one axis of the composed map, the header's operation order
static int geometry_axis(int n_src, int n_rect, double off, double scale, int mirror, int64_t* a_out, int64_t* b_out) {
    const double r = (double)n_src / (double)n_rect;
    const double g = r / scale;
    const double m0 = mirror ? (double)(n_rect - 1) : 0.0;
    const double c = ((m0 - off) / scale + 0.5) * r - 0.5;
    const double a = mirror ? -g : g;
    const double qa = floor(a * 2097152.0 + 0.5), qb = floor(c * 2097152.0 + 0.5);
    if (!(fabs(qa) < 4611686018427387904.0) || !(fabs(qb) < 4611686018427387904.0)) return 1;      // (false for a NaN)
    *a_out = (int64_t)qa; *b_out = (int64_t)qb + 32768;
    return 0;
}

extern "C" int rtm3d_augment_geometry(const rtm3d_frame_geom* geom, double scale, double off_x, double off_y, int flip,
                                      rtm3d_augment_frame* out) {
    const char* who = "augment_geometry";
    if (!geom || !out) { rt_set_error("%s: null pointer", who); return 1; }
    if (geom->h < 1 || geom->w < 1 || geom->rh < 1 || geom->rw < 1) {
        rt_set_error("%s: a frame of %d x %d resized to %d x %d", who, geom->h, geom->w, geom->rh, geom->rw); return 1;
    }
    if (!(scale > 0) || !(scale <= 1.7976931348623157e308)) { rt_set_error("%s: scale %g is not finite and > 0", who, scale); return 1; }
    if (!(fabs(off_x) <= 1.7976931348623157e308) || !(fabs(off_y) <= 1.7976931348623157e308)) {
        rt_set_error("%s: offset (%g, %g) is not finite", who, off_x, off_y); return 1;
    }
    int64_t ax, bx, ay, by;
    if (geometry_axis(geom->w, geom->rw, off_x, scale, flip != 0, &ax, &bx) || geometry_axis(geom->h, geom->rh, off_y, scale, 0, &ay, &by)) {
        rt_set_error("%s: scale %g, offset (%g, %g): a coefficient beyond 2^62", who, scale, off_x, off_y); return 1;
    }
    out->h = geom->h; out->w = geom->w;
    out->x0 = geom->pad_w; out->y0 = geom->pad_h; out->rw = geom->rw; out->rh = geom->rh;
    out->ax = ax; out->bx = bx; out->ay = ay; out->by = by;
    return 0;
}

static bool side_ok(int v) { return v >= 1 && v <= AUG_MAX_SIDE; }
static bool below(int64_t v, int bits) { return v > -((int64_t)1 << bits) && v < ((int64_t)1 << bits); }

// what concerns the descriptors and the canvas alone (the plan has nothing else)
static int check_frames(const char* who, int B, const rtm3d_augment_frame* h_frames, int out_mode, int H, int W, int out_border) {
    if (refuse_count(who, B) || refuse_null(who, h_frames)) return 1;
    if (out_mode < 0 || out_mode > 2) { rt_set_error("%s: out_mode %d is none of 0 (fp32 NCHW), 1 (fp16 NHWC4), 2 (packed uint8)", who, out_mode); return 1; }
    if (!side_ok(H) || !side_ok(W)) { rt_set_error("%s: a canvas of %d x %d; a side must lie in 1..%d", who, H, W, AUG_MAX_SIDE); return 1; }
    if (out_mode == 1 && (out_border < 0 || out_border > AUG_MAX_SIDE)) { rt_set_error("%s: out_border %d", who, out_border); return 1; }
    for (int b = 0; b < B; ++b) {
        const rtm3d_augment_frame& f = h_frames[b];
        if (refuse_side(who, b, f.h, f.w, 1, AUG_MAX_SIDE)) return 1;
        if (f.rw < 1 || f.rh < 1 || f.x0 < 0 || f.y0 < 0 || f.rw > W || f.rh > H || f.x0 > W - f.rw || f.y0 > H - f.rh) {
            rt_set_error("%s: frame %d: the rectangle %d x %d at (%d, %d) leaves the %d x %d canvas", who, b, f.rh, f.rw, f.y0, f.x0, H, W);
            return 1;
        }
        if (f.sigma_q < 0 || f.sigma_q > 65535) { rt_set_error("%s: frame %d: sigma_q %d outside 0..65535", who, b, f.sigma_q); return 1; }
        if (f.alpha_q > (1 << 24) || f.alpha_q < -(1 << 24)) { rt_set_error("%s: frame %d: |alpha_q| = |%d| > 2^24", who, b, f.alpha_q); return 1; }
        if (f.beta_q > INT32_MAX - (1 << 24) + 1 || f.beta_q < -(INT32_MAX - (1 << 24) + 1)) {
            rt_set_error("%s: frame %d: |beta_q| = |%d| > 2^31 - 2^24", who, b, f.beta_q); return 1;
        }
        if (!below(f.ax, 40) || !below(f.ay, 40)) {
            rt_set_error("%s: frame %d: |ax| or |ay| (%lld, %lld) at or above 2^40", who, b, (long long)f.ax, (long long)f.ay); return 1;
        }
        if (!below(f.bx, 56) || !below(f.by, 56)) {
            rt_set_error("%s: frame %d: |bx| or |by| (%lld, %lld) at or above 2^56", who, b, (long long)f.bx, (long long)f.by); return 1;
        }
        if (refuse_reserved(who, b, f.reserved)) return 1;
    }
    return 0;
}

static int runs_between(int lo, int hi, int shift) { return ((hi - 1 + shift) >> 2) - ((lo + shift) >> 2) + 1; }   // runs that meet lo .. hi - 1

static rtm3d_augment_plan plan_chunk(const FrameChunk c, const rtm3d_augment_frame* h_frames, int out_mode, int H, int W, int out_border) {
    rtm3d_augment_plan P;
    P.first = c.b0; P.count = c.nb;
    P.px_per_thread = AUG_PX; P.threads = AUG_THREADS;
    P.shift = out_mode == 1 ? (out_border & 3) : 0;
    P.runs = 0;
    bool border = false;
    for (int i = 0; i < c.nb; ++i) {
        const rtm3d_augment_frame& f = h_frames[c.b0 + i];
        const int runs = runs_between(f.x0, f.x0 + f.rw, P.shift) * f.rh;         // <= 4097 * 16384
        if (runs > P.runs) P.runs = runs;
        if (f.rw != W || f.rh != H) border = true;
    }
    P.grid_x = (P.runs + AUG_THREADS - 1) / AUG_THREADS;
    P.grid_y = c.nb;
    P.border_runs_per_row = runs_between(0, W, P.shift);
    const int all = (P.border_runs_per_row * H + AUG_THREADS - 1) / AUG_THREADS;
    P.border_grid_x = !border ? 0 : (all > AUG_BORDER_GRID ? AUG_BORDER_GRID : all);
    return P;
}

extern "C" int rtm3d_frames_augment_plan(int B, const rtm3d_augment_frame* h_frames, int out_mode, int H, int W, int out_border,
                                         rtm3d_augment_plan* out) {
    if (refuse_null("frames_augment_plan", out) || check_frames("frames_augment_plan", B, h_frames, out_mode, H, W, out_border)) return 1;
    for (const FrameChunk c : frame_chunks(B)) out[c.k] = plan_chunk(c, h_frames, out_mode, H, W, out_border);
    return 0;
}

extern "C" int rtm3d_frames_augment_check(int B, const uint8_t* const* h_src, const rtm3d_augment_frame* h_frames, const void* d_out,
                                          int out_mode, int H, int W, int out_border, const int16_t* d_noise_table, const float* d_lut,
                                          const void* d_lut16, const unsigned long long* d_sums) {
    const char* who = "frames_augment";
    if (refuse_null(who, h_src) || check_frames(who, B, h_frames, out_mode, H, W, out_border)) return 1;
    if (!d_out) { rt_set_error("%s: the destination is a NULL pointer", who); return 1; }
    if (!d_noise_table) { rt_set_error("%s: the noise table is a NULL pointer", who); return 1; }
    if ((uintptr_t)d_noise_table & 1) { rt_set_error("%s: the noise table's address is odd", who); return 1; }
    if (!d_sums) { rt_set_error("%s: the channel sums are a NULL pointer", who); return 1; }
    if ((uintptr_t)d_sums & 7) { rt_set_error("%s: the channel sums' address is no multiple of 8", who); return 1; }
    if (out_mode == 0 && !d_lut) { rt_set_error("%s: the fp32 normalisation table is a NULL pointer", who); return 1; }
    if (out_mode == 1 && !d_lut16) { rt_set_error("%s: the fp16 normalisation table is a NULL pointer", who); return 1; }
    if (out_mode == 0 && ((uintptr_t)d_out & 3)) { rt_set_error("%s: the fp32 destination's address is no multiple of 4", who); return 1; }
    if (out_mode == 1 && ((uintptr_t)d_out & 7)) { rt_set_error("%s: the fp16 NHWC4 destination's address is no multiple of 8", who); return 1; }
    const uintptr_t d0 = (uintptr_t)d_out, d1 = d0 + (size_t)B * H * W * 3;
    for (int b = 0; b < B; ++b) {
        if (!h_src[b]) { rt_set_error("%s: frame %d: the source is a NULL pointer", who, b); return 1; }
        const uintptr_t s0 = (uintptr_t)h_src[b], s1 = s0 + (size_t)h_frames[b].h * h_frames[b].w * 3;
        if (out_mode == 2 && d0 < s1 && s0 < d1) { rt_set_error("%s: frame %d: the destination overlaps this source", who, b); return 1; }
    }
    return 0;
}

template <int MODE>
static void launch_chunk(hipStream_t s, const rtm3d_augment_plan& P, const AugBatch& ab, void* d_out, int H, int W, int out_border,
                         const int16_t* d_T, const float* d_lut, const void* d_lut16, unsigned long long* d_sums) {
    hipLaunchKernelGGL(augment_interior_kernel<MODE>, dim3((unsigned)P.grid_x, (unsigned)P.grid_y), dim3(AUG_THREADS), 0, s, ab, d_out, P.first,
                       H, W, out_border, P.shift, d_T, d_lut, (const uint16_t*)d_lut16, d_sums);
    if (P.border_grid_x > 0)
        hipLaunchKernelGGL(augment_border_kernel<MODE>, dim3((unsigned)P.border_grid_x, (unsigned)P.grid_y), dim3(AUG_THREADS), 0, s, ab, d_out,
                           P.first, H, W, out_border, P.shift, P.border_runs_per_row, d_lut, (const uint16_t*)d_lut16, d_sums);
}

extern "C" int rtm3d_frames_augment(void* stream, int B, const uint8_t* const* h_src, const rtm3d_augment_frame* h_frames, void* d_out,
                                    int out_mode, int H, int W, int out_border, const int16_t* d_noise_table, const float* d_lut,
                                    const void* d_lut16, unsigned long long* d_sums) {
    // the whole batch, before the first memset or launch
    if (rtm3d_frames_augment_check(B, h_src, h_frames, d_out, out_mode, H, W, out_border, d_noise_table, d_lut, d_lut16, d_sums)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_sums, 0, (size_t)B * 3 * sizeof(unsigned long long), s) != hipSuccess) { rt_set_error("frames_augment: memset failed"); return 1; }
    for (const FrameChunk c : frame_chunks(B)) {
        const rtm3d_augment_plan plan = plan_chunk(c, h_frames, out_mode, H, W, out_border);       // the numbers of rtm3d_frames_augment_plan
        AugBatch ab;
        memset(&ab, 0, sizeof ab);                                                     // (an unused entry is never indexed: grid_y = nb)
        for (int i = 0; i < c.nb; ++i) { ab.f[i].src = h_src[c.b0 + i]; ab.f[i].f = h_frames[c.b0 + i]; }
        if (out_mode == 0) launch_chunk<0>(s, plan, ab, d_out, H, W, out_border, d_noise_table, d_lut, d_lut16, d_sums);
        else if (out_mode == 1) launch_chunk<1>(s, plan, ab, d_out, H, W, out_border, d_noise_table, d_lut, d_lut16, d_sums);
        else launch_chunk<2>(s, plan, ab, d_out, H, W, out_border, d_noise_table, d_lut, d_lut16, d_sums);
    }
    return launch_ok("frames_augment");
}
