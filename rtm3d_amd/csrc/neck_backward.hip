// Neck fusion backward (include/rtm3d_hip.h, "neck fusion backward"): from dz, the gradient of the fused map, to the gradients of
// the fusion_up transposed convs' weights and of their inputs kfpn_h3 / h4 / h5.  Every product is an fp16 x fp16 MFMA product
// (16x16x32) with fp32 accumulation, no float atomic anywhere: two runs on equal inputs leave equal bytes.
//
//   nb_softmax_stats    per (operand, image, run of consecutive pixels, channel): the max m and the sum Z of exp(u - m) of the run
//   nb_softmax_combine  adds the runs in index order -> m, Z per (operand, image, channel)
//   nb_softmax_grad     du[p][c] = fp16(T dz[p][c] exp(u[p][c] - m) / Z) on the interior of a map with border 1
//   nb_deconv_wgrad     part[slice][tap][ci][co] = sum_p X[p][ci] dY[2 p + tap - 1][co]: per tap a GEMM whose K dimension is the pixels
//                       of a slice.  The tile shape and the LDS image are the head backward's (head_backward.hip, "THE LDS IMAGE"):
//                       [32 pixels][128 channels], 16-byte chunks XOR'd by the row's key, read back with ds_read_b64_tr_b16.
//                       X is gathered at stride 1, dY at stride 2 plus the tap offset.
//   nb_deconv_reduce    adds the slices in index order, applies 1 / (S T), writes torch's (ci, co, 4, 4) order, counts non-finite
//   nb_deconv_dgrad     dX[p][ci] = fp16(sum_{tap, co} dY[2 p + tap - 1][co] Wf[ci][co][tap]): operands straight from global memory in
//                       fragment order (8 consecutive co per lane), no LDS - the head dgrad's schedule with 16 taps
//
// The softmax kernels are memory-bound: a lane moves 16 bytes (8 channels), the 32 lanes of a half wave cover the 256 channels of
// a pixel, so a wave's access is two whole 512-byte pixels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rtm3d_hip.h"

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define LDS_AS __attribute__((address_space(3)))

#define NB_PIX 32                          // pixels of a wgrad tile = the K of one MFMA (the head backward's tile: its slices are reused)
#define NB_THREADS 256
#define NB_C 256                           // channels of every map of the fusion
#define NB_TAPS 16
#define NB_DG_PT 4                         // 16-pixel tiles per wave of the dgrad
#define NB_RUNS 32                         // at most this many runs of consecutive pixels per (operand, image)
#define NB_GRAD_PIX 32                     // pixels of a softmax-grad workgroup

struct NbMap {                             // rtm3d_hb_map plus the strides the kernels use
    const f16* d;
    long long img;                         // elements per image
    int row;                               // elements per padded row
    int C, P, coff;
};

__device__ __forceinline__ long long nb_at(const NbMap& m, int b, int y, int x) {
    return b * m.img + (long long)(y + m.P) * m.row + (long long)(x + m.P) * m.C + m.coff;
}

// ------------------------------------------------------------------------------------------------ softmax
struct NbSoftmaxArgs {
    NbMap dz, u[3], du[3];
    int B, H, W, n_ops;
    int run, runs;                         // pixels per run, runs per image
    float T;
    float* part;                           // [op][b][run][2][256]: m, Z of the run
    float* fin;                            // [op][b][2][256]: m, Z
};

// a workgroup: one run of one image of one operand; thread: 8 channels (chunk) of the pixels run0 + prow, + 8, ...  Each thread keeps
// a running (m, Z) per channel, pixel after pixel; the 8 threads of a channel are then combined in prow order.
__global__ __launch_bounds__(NB_THREADS) void nb_softmax_stats(const NbSoftmaxArgs a) {
    __shared__ float sm[8][NB_C], sz[8][NB_C];
    const int tid = threadIdx.x, chunk = tid & 31, prow = tid >> 5;
    const int r = blockIdx.x, b = blockIdx.y, op = blockIdx.z;
    const NbMap u = a.u[op];
    const int HW = a.H * a.W;
    const int p0 = r * a.run, p1 = min(p0 + a.run, HW);
    float m[8], z[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { m[k] = -INFINITY; z[k] = 0.f; }
    for (int p = p0 + prow; p < p1; p += 8) {
        const int y = p / a.W, x = p - y * a.W;
        const f16x8 v = *(const f16x8*)(u.d + nb_at(u, b, y, x) + chunk * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float f = (float)v[k];
            const float mn = fmaxf(m[k], f);
            z[k] = z[k] * expf(m[k] - mn) + expf(f - mn);             // (m = -inf: z = 0 and exp(-inf) = 0)
            m[k] = mn;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { sm[prow][chunk * 8 + k] = m[k]; sz[prow][chunk * 8 + k] = z[k]; }
    __syncthreads();
    const int c = tid;
    float M = -INFINITY, Z = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) M = fmaxf(M, sm[k][c]);
#pragma unroll
    for (int k = 0; k < 8; ++k) Z += sz[k][c] * expf(sm[k][c] - M);   // (a prow without a pixel: 0 * exp(-inf) = 0; a run is never empty)
    float* out = a.part + (((long long)op * a.B + b) * a.runs + r) * 2 * NB_C;
    out[c] = M;
    out[NB_C + c] = Z;
}

__global__ __launch_bounds__(NB_THREADS) void nb_softmax_combine(const NbSoftmaxArgs a) {
    const int c = threadIdx.x, b = blockIdx.x, op = blockIdx.y;
    const float* in = a.part + ((long long)op * a.B + b) * a.runs * 2 * NB_C;
    float M = -INFINITY, Z = 0.f;
    for (int r = 0; r < a.runs; ++r) M = fmaxf(M, in[(long long)r * 2 * NB_C + c]);
    for (int r = 0; r < a.runs; ++r) Z += in[(long long)r * 2 * NB_C + NB_C + c] * expf(in[(long long)r * 2 * NB_C + c] - M);
    float* out = a.fin + ((long long)op * a.B + b) * 2 * NB_C;
    out[c] = M;
    out[NB_C + c] = Z;
}

__global__ __launch_bounds__(NB_THREADS) void nb_softmax_grad(const NbSoftmaxArgs a) {
    const int tid = threadIdx.x, chunk = tid & 31, prow = tid >> 5;
    const int b = blockIdx.y, op = blockIdx.z;
    const NbMap u = a.u[op], du = a.du[op];
    const int HW = a.H * a.W;
    const float* fin = a.fin + ((long long)op * a.B + b) * 2 * NB_C + chunk * 8;
    float m[8], z[8];
#pragma unroll
    for (int k = 0; k < 8; k += 4) {
        const f32x4 mv = *(const f32x4*)(fin + k), zv = *(const f32x4*)(fin + NB_C + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) { m[k + e] = mv[e]; z[k + e] = zv[e]; }
    }
#pragma unroll
    for (int i = 0; i < NB_GRAD_PIX / 8; ++i) {
        const int p = blockIdx.x * NB_GRAD_PIX + i * 8 + prow;
        if (p >= HW) continue;
        const int y = p / a.W, x = p - y * a.W;
        const f16x8 uv = *(const f16x8*)(u.d + nb_at(u, b, y, x) + chunk * 8);
        const f16x8 gv = *(const f16x8*)(a.dz.d + nb_at(a.dz, b, y, x) + chunk * 8);
        f16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (f16)((a.T * (float)gv[k]) * (expf((float)uv[k] - m[k]) / z[k]));
        *(f16x8*)((f16*)du.d + nb_at(du, b, y, x) + chunk * 8) = o;
    }
}

// ------------------------------------------------------------------------------------------------ wgrad
struct NbWgradArgs {
    NbMap x, dy;                           // x: Hi x Wi; dy: 2 Hi x 2 Wi, zero border >= 1
    int B, H, W;                           // Hi, Wi
    int tiles_per_slice;
    long long npix;
    float* part;                           // [slice][tap][ci][co]
};

__device__ __forceinline__ uint32_t nb_lds_off(int row, int chunk) {                 // bytes; chunk: 16-byte chunk of the tile's 128 channels
    return (uint32_t)(row * 256 + ((chunk ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4));
}

// 2 x 2 waves, each 4 x 4 MFMA tiles of 16 (ci) x 16 (co): a 128 x 128 tile of one tap's dW
__global__ __launch_bounds__(NB_THREADS) void nb_deconv_wgrad(const NbWgradArgs a) {
    constexpr int MT = 4, NT = 4, PER = NB_PIX * 128 / 8 / NB_THREADS;             // 16-byte pieces of a tile per thread: 2
    __shared__ __attribute__((aligned(16))) f16 lds_x[NB_PIX * 128];
    __shared__ __attribute__((aligned(16))) f16 lds_dy[NB_PIX * 128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ci0 = (blockIdx.x >> 1) * 128, co0 = (blockIdx.x & 1) * 128;
    const int tap = blockIdx.y, slice = blockIdx.z;
    const int ky = tap >> 2, kx = tap & 3;
    const long long HW = (long long)a.H * a.W;
    const f16* xb = a.x.d + ci0;
    const f16* dyb = a.dy.d + co0;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // transposed-read addresses: lane 4q + p of a 16-lane group names row q, elements 4p .. 4p + 3 of the 16-channel block
    const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
    const uint32_t x_base = (uint32_t)(uintptr_t)(LDS_AS f16*)lds_x, dy_base = (uint32_t)(uintptr_t)(LDS_AS f16*)lds_dy;

    const long long tile0 = (long long)slice * a.tiles_per_slice;
    long long tile1 = tile0 + a.tiles_per_slice;
    const long long ntiles = (a.npix + NB_PIX - 1) / NB_PIX;
    if (tile1 > ntiles) tile1 = ntiles;

    f16x8 rx[PER], rdy[PER];
    auto fetch = [&](long long tile) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int piece = i * NB_THREADS + tid;
            const int px = piece >> 4, c = piece & 15;
            const long long n = tile * NB_PIX + px;
            f16x8 vx = {0, 0, 0, 0, 0, 0, 0, 0}, vy = {0, 0, 0, 0, 0, 0, 0, 0};
            if (n < a.npix) {                                          // (pixels beyond B Hi Wi: staged as zeros)
                const long long b = n / HW, r = n - b * HW;
                const int y = (int)(r / a.W), x = (int)(r - (long long)y * a.W);
                vx = *(const f16x8*)(xb + nb_at(a.x, (int)b, y, x) + c * 8);
                vy = *(const f16x8*)(dyb + nb_at(a.dy, (int)b, 2 * y + ky - 1, 2 * x + kx - 1) + c * 8);
            }
            rx[i] = vx; rdy[i] = vy;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int piece = i * NB_THREADS + tid;
            *(LDS_AS f16x8*)(uintptr_t)(x_base + nb_lds_off(piece >> 4, piece & 15)) = rx[i];
            *(LDS_AS f16x8*)(uintptr_t)(dy_base + nb_lds_off(piece >> 4, piece & 15)) = rdy[i];
        }
    };

    if (tile0 < tile1) fetch(tile0);
    for (long long tile = tile0; tile < tile1; ++tile) {              // (uniform trip count: every lane of every wave takes every barrier)
        store();
        __syncthreads();
        if (tile + 1 < tile1) fetch(tile + 1);                        // in flight while this tile is multiplied
        f16x8 af[MT], bf[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int chunk = ((wm * MT + i) * 16 + 4 * p4) >> 3;      // 16-byte chunk of the lane's 4 elements; + 8 bytes for the odd half
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(x_base + nb_lds_off(8 * grp + q, chunk) + 8 * (p4 & 1)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(x_base + nb_lds_off(8 * grp + 4 + q, chunk) + 8 * (p4 & 1)));
            const f16x4 l4 = __builtin_bit_cast(f16x4, lo), h4 = __builtin_bit_cast(f16x4, hi);
            af[i] = (f16x8){l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int chunk = ((wn * NT + j) * 16 + 4 * p4) >> 3;
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(dy_base + nb_lds_off(8 * grp + q, chunk) + 8 * (p4 & 1)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(dy_base + nb_lds_off(8 * grp + 4 + q, chunk) + 8 * (p4 & 1)));
            const f16x4 l4 = __builtin_bit_cast(f16x4, lo), h4 = __builtin_bit_cast(f16x4, hi);
            bf[j] = (f16x8){l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        __syncthreads();                                              // the images are free for the next tile
    }

    // D[row = ci = 4 (lane >> 4) + e][col = co = lane & 15]
    float* out = a.part + ((long long)slice * NB_TAPS + tap) * NB_C * NB_C;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ci = ci0 + (wm * MT + i) * 16 + 4 * grp + e, co = co0 + (wn * NT + j) * 16 + (lane & 15);
                out[(long long)ci * NB_C + co] = acc[i][j][e];
            }
}

struct NbReduceArgs {
    const float* part;                     // [slice][tap][ci][co]
    float* dw;                             // (ci, co, 4, 4)
    int slices;
    float inv_scale;                       // 1 / (S T)
    unsigned* nonfinite;
};

// one thread per (ci, co): 16 taps, each the sum of its slices in slice order; 64 contiguous bytes out
__global__ __launch_bounds__(NB_THREADS) void nb_deconv_reduce(const NbReduceArgs a) {
    const int i = blockIdx.x * NB_THREADS + threadIdx.x;             // ci * 256 + co
    unsigned bad = 0;
    f32x4 o[4];
#pragma unroll
    for (int tap = 0; tap < NB_TAPS; ++tap) {
        const float* p = a.part + (long long)tap * NB_C * NB_C + i;
        float v = 0.f;
        for (int sl = 0; sl < a.slices; ++sl) v += p[(long long)sl * NB_TAPS * NB_C * NB_C];
        v = v * a.inv_scale;               // (a power of two: exact)
        if (!(fabsf(v) <= 3.4028234663852886e38f)) ++bad;
        o[tap >> 2][tap & 3] = v;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) *(f32x4*)(a.dw + (long long)i * NB_TAPS + 4 * k) = o[k];
    if (bad) atomicAdd(a.nonfinite, bad);  // an integer counter: the order does not show
}

// ------------------------------------------------------------------------------------------------ dgrad
struct NbDgradArgs {
    NbMap dy, out;                         // dy: 2 Hi x 2 Wi, zero border >= 1; out: Hi x Wi
    const f16* wr;                         // [tap][ci 256][co 256]
    int B, H, W;                           // Hi, Wi
    long long npix;
};

// a workgroup: 32 NB_DG_PT pixels x 256 ci; wave w: NB_DG_PT 16-pixel tiles from pixel 16 NB_DG_PT (w >> 1), ci 128 (w & 1) ..;
// D[row = ci][col = pixel].  Four pixel tiles per wave: every weight fragment loaded serves four MFMAs.
__global__ __launch_bounds__(NB_THREADS) void nb_deconv_dgrad(const NbDgradArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const long long HW = (long long)a.H * a.W;
    const int ci_w = 128 * (wave & 1);
    long long pix[NB_DG_PT];
    int py[NB_DG_PT], pxx[NB_DG_PT], pb[NB_DG_PT];
#pragma unroll
    for (int t = 0; t < NB_DG_PT; ++t) {
        long long n = (long long)blockIdx.x * (32 * NB_DG_PT) + 16 * NB_DG_PT * (wave >> 1) + 16 * t + col;
        pix[t] = n;
        if (n >= a.npix) n = a.npix - 1;                                // a copy of the last pixel: computed, never stored
        const long long b = n / HW, r = n - b * HW;
        pb[t] = (int)b; py[t] = (int)(r / a.W); pxx[t] = (int)(r - (long long)py[t] * a.W);
    }
    f32x4 acc[8][NB_DG_PT];
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int t = 0; t < NB_DG_PT; ++t) acc[c][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f16* dyb = a.dy.d + 8 * kq;
    const f16* wb = a.wr + (long long)(ci_w + col) * NB_C + 8 * kq;
    for (int tap = 0; tap < NB_TAPS; ++tap) {
        const int ky = tap >> 2, kx = tap & 3;
        const f16* yp[NB_DG_PT];
#pragma unroll
        for (int t = 0; t < NB_DG_PT; ++t) yp[t] = dyb + nb_at(a.dy, pb[t], 2 * py[t] + ky - 1, 2 * pxx[t] + kx - 1);
        const f16* wt = wb + (long long)tap * NB_C * NB_C;
        for (int ks = 0; ks < NB_C / 32; ++ks) {
            f16x8 bf[NB_DG_PT], af[8];
#pragma unroll
            for (int t = 0; t < NB_DG_PT; ++t) bf[t] = *(const f16x8*)(yp[t] + ks * 32);
#pragma unroll
            for (int c = 0; c < 8; ++c) af[c] = *(const f16x8*)(wt + (long long)c * 16 * NB_C + ks * 32);
#pragma unroll
            for (int c = 0; c < 8; ++c)
#pragma unroll
                for (int t = 0; t < NB_DG_PT; ++t) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[c], bf[t], acc[c][t], 0, 0, 0);
        }
    }
    // lane: pixel `col` of tile t, channels ci_w + 16 c + 4 kq .. + 3
#pragma unroll
    for (int t = 0; t < NB_DG_PT; ++t) {
        if (pix[t] >= a.npix) continue;
        const long long at_o = nb_at(a.out, pb[t], py[t], pxx[t]);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            f16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (f16)acc[c][t][e];
            *(f16x4*)((f16*)a.out.d + at_o + ci_w + 16 * c + 4 * kq) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host
extern void rt_set_error(const char* fmt, ...);

#define NB_MAX_DIM 16384
#define NB_MAX_PIX (1LL << 31)

static bool nb_pow2(float v) {
    int ex = 0;
    return v > 0.f && v <= 3.4028234663852886e38f && frexpf(v, &ex) == 0.5f;
}

static int nb_scales(const char* who, float grad_scale, float fusion_scale) {
    if (!nb_pow2(grad_scale)) { rt_set_error("%s: grad_scale = %g is no power of two", who, (double)grad_scale); return RTM3D_NB_E_SCALE; }
    if (!nb_pow2(fusion_scale)) { rt_set_error("%s: fusion_scale = %g is no power of two", who, (double)fusion_scale); return RTM3D_NB_E_SCALE; }
    const float st = grad_scale * fusion_scale;
    if (!nb_pow2(st) || !nb_pow2(1.0f / st)) {
        rt_set_error("%s: grad_scale * fusion_scale = %g * %g leaves the fp32 range", who, (double)grad_scale, (double)fusion_scale); return RTM3D_NB_E_SCALE;
    }
    return 0;
}

static int nb_shape(const char* who, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || B > NB_MAX_DIM || H > NB_MAX_DIM || W > NB_MAX_DIM || (long long)B * H * W >= NB_MAX_PIX) {
        rt_set_error("%s: B, H, W = %d, %d, %d: each must be 1 .. %d and B * H * W below 2^31", who, B, H, W, NB_MAX_DIM); return RTM3D_NB_E_SHAPE;
    }
    return 0;
}

extern "C" int rtm3d_neck_backward_check(int B, int H, int W, int levels, float grad_scale, float fusion_scale) {
    const char* who = "neck_backward_check";
    if (int rc = nb_shape(who, B, H, W)) return rc;
    if (levels < 1 || levels > 3) { rt_set_error("%s: %d fusion levels, the chain takes 1 .. 3", who, levels); return RTM3D_NB_E_LEVELS; }
    if ((H & ((1 << levels) - 1)) || (W & ((1 << levels) - 1))) {
        rt_set_error("%s: the map is %d x %d, %d levels need multiples of %d", who, H, W, levels, 1 << levels); return RTM3D_NB_E_MULTIPLE;
    }
    return nb_scales(who, grad_scale, fusion_scale);
}

static void nb_runs(int HW, int* run, int* runs) {                      // at most NB_RUNS runs of a multiple of 8 pixels
    int r = (HW + NB_RUNS - 1) / NB_RUNS;
    r = (r + 7) & ~7;
    *run = r;
    *runs = (HW + r - 1) / r;
}

static size_t nb_softmax_bytes(int B, int levels) { return (size_t)levels * B * (NB_RUNS + 1) * 2 * NB_C * sizeof(float); }
static size_t nb_wgrad_bytes(int n_slices) { return (size_t)n_slices * NB_TAPS * NB_C * NB_C * sizeof(float); }

extern "C" size_t rtm3d_neck_backward_workspace_bytes(int B, int levels, int n_slices) {
    if (B < 1 || B > NB_MAX_DIM || levels < 1 || levels > 3 || n_slices < 1 || n_slices > RTM3D_HB_MAX_SLICES) return 0;
    const size_t s = nb_softmax_bytes(B, levels), w = nb_wgrad_bytes(n_slices);
    return s > w ? s : w;
}

// a map of 256 channels as the kernels read it; H, W: the map's own interior
static int nb_map(const char* who, const char* name, const rtm3d_hb_map* m, int H, int W, int need_border, NbMap* o) {
    if (!m || !m->d) { rt_set_error("%s: %s is a NULL pointer", who, name); return RTM3D_NB_E_NULL; }
    if ((uintptr_t)m->d & 15) { rt_set_error("%s: the address of %s is no multiple of 16", who, name); return RTM3D_NB_E_ALIGN; }
    if (m->C < NB_C || (m->C & 7) || m->coff < 0 || (m->coff & 7) || (long long)m->coff + NB_C > m->C) {
        rt_set_error("%s: %s: %d channels at offset %d do not fit %d channels in steps of 8", who, name, NB_C, m->coff, m->C); return RTM3D_NB_E_CHANNELS;
    }
    if (m->P < need_border || m->P > 64) { rt_set_error("%s: %s has a border of %d pixels, its reader's taps need %d (at most 64)", who, name, m->P, need_border); return RTM3D_NB_E_BORDER; }
    o->d = (const f16*)m->d;
    o->C = m->C; o->P = m->P; o->coff = m->coff;
    o->row = (W + 2 * m->P) * m->C;
    o->img = (long long)(H + 2 * m->P) * o->row;
    return 0;
}

static int nb_launched(const char* who) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("%s launch: %s", who, hipGetErrorString(e)); return RTM3D_NB_E_LAUNCH; }
    return 0;
}

extern "C" int rtm3d_neck_softmax_grad(void* stream, int B, int H, int W, int n_ops, const rtm3d_hb_map* dz, const rtm3d_hb_map* u,
                                       const rtm3d_hb_map* du, float fusion_scale, void* d_ws, size_t ws_bytes) {
    const char* who = "neck_softmax_grad";
    if (!dz || !u || !du || !d_ws) { rt_set_error("%s: null pointer", who); return RTM3D_NB_E_NULL; }
    if (int rc = nb_shape(who, B, H, W)) return rc;
    if (n_ops < 1 || n_ops > 3) { rt_set_error("%s: %d operands, the fusion takes 1 .. 3", who, n_ops); return RTM3D_NB_E_LEVELS; }
    if (int rc = nb_scales(who, 1.0f, fusion_scale)) return rc;
    NbSoftmaxArgs a;
    if (int rc = nb_map(who, "dz", dz, H, W, 0, &a.dz)) return rc;
    for (int i = 0; i < 3; ++i) {
        if (i >= n_ops) { a.u[i] = a.u[0]; a.du[i] = a.du[0]; continue; }
        if (int rc = nb_map(who, "u", u + i, H, W, 0, &a.u[i])) return rc;
        if (int rc = nb_map(who, "du", du + i, H, W, 1, &a.du[i])) return rc;
    }
    if ((uintptr_t)d_ws & 15) { rt_set_error("%s: the workspace is misaligned", who); return RTM3D_NB_E_ALIGN; }
    if (ws_bytes < nb_softmax_bytes(B, n_ops)) {
        rt_set_error("%s: the workspace has %zu bytes, the statistics of %d operands need %zu", who, ws_bytes, n_ops, nb_softmax_bytes(B, n_ops));
        return RTM3D_NB_E_WORKSPACE;
    }
    a.B = B; a.H = H; a.W = W; a.n_ops = n_ops; a.T = fusion_scale;
    nb_runs(H * W, &a.run, &a.runs);
    a.part = (float*)d_ws;
    a.fin = a.part + (size_t)n_ops * B * NB_RUNS * 2 * NB_C;
    hipLaunchKernelGGL(nb_softmax_stats, dim3(a.runs, B, n_ops), dim3(NB_THREADS), 0, (hipStream_t)stream, a);
    if (int rc = nb_launched(who)) return rc;
    hipLaunchKernelGGL(nb_softmax_combine, dim3(B, n_ops), dim3(NB_THREADS), 0, (hipStream_t)stream, a);
    if (int rc = nb_launched(who)) return rc;
    hipLaunchKernelGGL(nb_softmax_grad, dim3((H * W + NB_GRAD_PIX - 1) / NB_GRAD_PIX, B, n_ops), dim3(NB_THREADS), 0, (hipStream_t)stream, a);
    return nb_launched(who);
}

extern "C" int rtm3d_neck_deconv_wgrad(void* stream, int B, int Hi, int Wi, const rtm3d_hb_map* x, const rtm3d_hb_map* dy, float grad_scale,
                                       float fusion_scale, float* d_dw, int want_slices, void* d_ws, size_t ws_bytes, unsigned* d_nonfinite) {
    const char* who = "neck_deconv_wgrad";
    if (!x || !dy || !d_ws || !d_nonfinite) { rt_set_error("%s: null pointer", who); return RTM3D_NB_E_NULL; }
    if (int rc = nb_shape(who, B, Hi, Wi)) return rc;
    if (int rc = nb_shape(who, B, 2 * Hi, 2 * Wi)) return rc;
    if (int rc = nb_scales(who, grad_scale, fusion_scale)) return rc;
    NbWgradArgs w;
    if (int rc = nb_map(who, "X", x, Hi, Wi, 0, &w.x)) return rc;
    if (int rc = nb_map(who, "dY", dy, 2 * Hi, 2 * Wi, 1, &w.dy)) return rc;
    if (((uintptr_t)d_ws & 15) || ((uintptr_t)d_dw & 15) || ((uintptr_t)d_nonfinite & 3)) {
        rt_set_error("%s: the workspace, the gradient or the counter is misaligned", who); return RTM3D_NB_E_ALIGN;
    }
    const long long npix = (long long)B * Hi * Wi;
    int slices = 0, tps = 0;
    if (rtm3d_head_backward_slices(npix, want_slices, &slices, &tps)) return RTM3D_NB_E_SLICES;      // (the message is the callee's)
    if (ws_bytes < nb_wgrad_bytes(slices)) {
        rt_set_error("%s: the workspace has %zu bytes, %d slices need %zu", who, ws_bytes, slices, nb_wgrad_bytes(slices)); return RTM3D_NB_E_WORKSPACE;
    }
    if (!d_dw) return 0;
    w.B = B; w.H = Hi; w.W = Wi; w.tiles_per_slice = tps; w.npix = npix; w.part = (float*)d_ws;
    hipLaunchKernelGGL(nb_deconv_wgrad, dim3(4, NB_TAPS, slices), dim3(NB_THREADS), 0, (hipStream_t)stream, w);
    if (int rc = nb_launched(who)) return rc;
    NbReduceArgs r;
    r.part = w.part; r.dw = d_dw; r.slices = slices; r.inv_scale = 1.0f / (grad_scale * fusion_scale); r.nonfinite = d_nonfinite;
    hipLaunchKernelGGL(nb_deconv_reduce, dim3(NB_C * NB_C / NB_THREADS), dim3(NB_THREADS), 0, (hipStream_t)stream, r);
    return nb_launched(who);
}

extern "C" int rtm3d_neck_deconv_dgrad(void* stream, int B, int Hi, int Wi, const rtm3d_hb_map* dy, const void* d_wr, const rtm3d_hb_map* dx) {
    const char* who = "neck_deconv_dgrad";
    if (!dy || !d_wr || !dx) { rt_set_error("%s: null pointer", who); return RTM3D_NB_E_NULL; }
    if (int rc = nb_shape(who, B, Hi, Wi)) return rc;
    if (int rc = nb_shape(who, B, 2 * Hi, 2 * Wi)) return rc;
    if ((uintptr_t)d_wr & 15) { rt_set_error("%s: the address of the weights is no multiple of 16", who); return RTM3D_NB_E_ALIGN; }
    NbDgradArgs a;
    if (int rc = nb_map(who, "dY", dy, 2 * Hi, 2 * Wi, 1, &a.dy)) return rc;
    if (int rc = nb_map(who, "dX", dx, Hi, Wi, 0, &a.out)) return rc;
    a.wr = (const f16*)d_wr; a.B = B; a.H = Hi; a.W = Wi; a.npix = (long long)B * Hi * Wi;
    hipLaunchKernelGGL(nb_deconv_dgrad, dim3((unsigned)((a.npix + 32 * NB_DG_PT - 1) / (32 * NB_DG_PT))), dim3(NB_THREADS), 0, (hipStream_t)stream, a);
    return nb_launched(who);
}
