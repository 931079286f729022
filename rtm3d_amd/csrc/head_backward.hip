// Head backward (include/rtm3d_hip.h, "head backward"): from the gradients of the logit maps to the gradients of the head convs'
// weights and biases and of the activations behind them.  Five kernels, every product an fp16 x fp16 MFMA product (16x16x32)
// with fp32 accumulation, no float atomic anywhere: a reduction over pixels is cut into slices, each slice writes a partial, and
// a second pass adds the partials in slice order - two runs on equal inputs leave equal bytes.
//
//   hb_go_kernel       fp32 NCHW dL/dlogit of the G heads -> one fp16 NHWC map, 16 channels per head, scaled by S
//   hb_wgrad_kernel    dW[tap][co][ci] = sum_p dY[p][co] X[p + dil tap][ci]: per (group, tap) a GEMM whose K dimension is the pixels.
//                      Both operands are channel-contiguous in memory and pixel-contiguous in the MFMA: a workgroup stages
//                      [32 pixels][channels] tiles of both in LDS and reads them back with ds_read_b64_tr_b16.
//   hb_colsum_kernel   db[c] = sum_p dY[p][c], over up to 1024 pixel slices of its own
//   hb_reduce_kernel   adds the slices in index order, applies 1/S and the BatchNorm scale s[co], writes torch's (cout, cin, 3, 3)
//                      order in fp32 and counts non-finite results
//   hb_dgrad_kernel    dX[p][ci] = [X > 0] sum_{tap, co} dY[p - dil tap][co] Wf[co][ci][tap]: operands straight from global memory in
//                      fragment order (8 consecutive channels per lane), no LDS
//
// THE LDS IMAGE of the wgrad.  A tile is [32 pixels][128 channels] fp16 with 256-byte rows (wider operands: one image per 128
// channels).  16-byte chunk ch (0 .. 15) of row r lies at 256 r + 16 (ch ^ key(r)), key(r) = ((r & 3) << 2) | ((r >> 2) & 3).  The
// A / B operand of mfma_f32_16x16x32_f16 wants, in lane l, channel l & 15 of the 16-channel tile and pixels 8 (l >> 4) .. + 7: two
// transposed reads per lane, read s taking rows 8 (l >> 4) + 4 s + q (q = 0 .. 3).  The LDS serves a transposed read per 32-lane
// half: rows {4 s + q} and {8 + 4 s + q} (or 16 more), two chunks each.  Their keys are 4 q + s and 4 q + 2 + s: the XOR sends the
// 8 rows x 2 chunks to 16 different chunks of the 256-byte bank row, so no two of them share a bank.  The staging stores are
// 16 bytes per lane, consecutive lanes on consecutive chunks of a row: the XOR permutes chunks inside a row, no conflict either.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rtm3d_hip.h"

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define LDS_AS __attribute__((address_space(3)))

#define HB_PIX 32                          // pixels of a wgrad tile = the K of one MFMA
#define HB_THREADS 256
#define HB_DG_PT 4                         // 16-pixel tiles per wave of the dgrad
#define HB_COLSUM_CH 256                   // channels of a colsum workgroup
#define HB_COLSUM_SLICES 1024              // pixel slices of the column sums (their own: see hb_colsum_kernel)

struct HbMap {                             // rtm3d_hb_map plus the strides the kernels use
    const f16* d;
    long long img;                         // elements per image
    int row;                               // elements per padded row
    int C, P, coff, gstride;
};

// ------------------------------------------------------------------------------------------------ go
struct HbGoArgs {
    const float* d[4];
    int K[4];
    int B, H, W, G;
    float S;
    HbMap go;
};

__global__ __launch_bounds__(HB_THREADS) void hb_go_kernel(const HbGoArgs a) {
    const long long n = (long long)blockIdx.x * HB_THREADS + threadIdx.x;          // (pixel, head)
    const long long N = (long long)a.B * a.H * a.W;
    if (n >= N * a.G) return;
    const int g = (int)(n % a.G);
    const long long p = n / a.G;
    const int x = (int)(p % a.W), y = (int)((p / a.W) % a.H), b = (int)(p / ((long long)a.W * a.H));
    const int K = a.K[g];
    const float* src = a.d[g] + ((long long)b * K * a.H + y) * a.W + x;
    f16x8 v[2];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k >> 3][k & 7] = k < K ? (f16)(a.S * src[(long long)k * a.H * a.W]) : (f16)0.0f;
    f16* dst = (f16*)a.go.d + b * a.go.img + (long long)(y + a.go.P) * a.go.row + (long long)(x + a.go.P) * a.go.C + a.go.coff + g * a.go.gstride;
    *(f16x8*)dst = v[0];
    *(f16x8*)(dst + 8) = v[1];
}

// ------------------------------------------------------------------------------------------------ wgrad
struct HbWgradArgs {
    HbMap dy, x;
    int B, H, W, G, dil, cout;             // cout: channels of dY per group (16 or 256) = rows of a partial
    int tiles_per_slice;
    long long npix;
    float* part;                           // [slice][g][tap][cout][256]
};

__device__ __forceinline__ uint32_t hb_lds_off(int row, int chunk) {                 // bytes; chunk: 16-byte chunk of the operand's channels
    return (uint32_t)((chunk >> 4) * (HB_PIX * 256) + row * 256 + (((chunk & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4));
}

// WM x WN waves, each MT x NT MFMA tiles of 16 (co) x 16 (ci)
template <int WM, int WN, int MT, int NT>
__global__ __launch_bounds__(HB_THREADS) void hb_wgrad_kernel(const HbWgradArgs a) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int CO_T = WM * MT * 16, CI_T = WN * NT * 16;
    constexpr int CO_IMG = (CO_T + 127) / 128, CI_IMG = (CI_T + 127) / 128;
    constexpr int DY_PIECES = HB_PIX * CO_T / 8, X_PIECES = HB_PIX * CI_T / 8;
    constexpr int DY_PER = (DY_PIECES + HB_THREADS - 1) / HB_THREADS, X_PER = X_PIECES / HB_THREADS;
    static_assert(X_PIECES % HB_THREADS == 0, "whole passes over the X tile");
    __shared__ __attribute__((aligned(16))) f16 lds_dy[CO_IMG * HB_PIX * 128];
    __shared__ __attribute__((aligned(16))) f16 lds_x[CI_IMG * HB_PIX * 128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int n_ci_tiles = 256 / CI_T;
    const int co0 = (blockIdx.x / n_ci_tiles) * CO_T, ci0 = (blockIdx.x % n_ci_tiles) * CI_T;
    const int tap = blockIdx.y % 9, g = blockIdx.y / 9, slice = blockIdx.z;
    const int dy_t = (tap / 3 - 1) * a.dil, dx_t = (tap % 3 - 1) * a.dil;
    const long long HW = (long long)a.H * a.W;
    const f16* dyb = a.dy.d + a.dy.coff + g * a.dy.gstride + co0;
    const f16* xb = a.x.d + a.x.coff + g * a.x.gstride + ci0;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // transposed-read addresses: lane 4q + p of a 16-lane group names row q, elements 4p .. 4p + 3 of the 16-channel block
    const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
    const uint32_t dy_base = (uint32_t)(uintptr_t)(LDS_AS f16*)lds_dy, x_base = (uint32_t)(uintptr_t)(LDS_AS f16*)lds_x;

    const long long tile0 = (long long)slice * a.tiles_per_slice;
    long long tile1 = tile0 + a.tiles_per_slice;
    const long long ntiles = (a.npix + HB_PIX - 1) / HB_PIX;
    if (tile1 > ntiles) tile1 = ntiles;

    f16x8 rdy[DY_PER], rx[X_PER];
    auto fetch = [&](long long tile) {
#pragma unroll
        for (int i = 0; i < DY_PER; ++i) {
            const int piece = i * HB_THREADS + tid;
            const int px = piece / (CO_T / 8), c = piece % (CO_T / 8);
            const long long n = tile * HB_PIX + px;
            f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (piece < DY_PIECES && n < a.npix) {
                const long long b = n / HW, r = n - b * HW;
                const int y = (int)(r / a.W), x = (int)(r - (long long)y * a.W);
                v = *(const f16x8*)(dyb + b * a.dy.img + (long long)(y + a.dy.P) * a.dy.row + (long long)(x + a.dy.P) * a.dy.C + c * 8);
            }
            rdy[i] = v;
        }
#pragma unroll
        for (int i = 0; i < X_PER; ++i) {
            const int piece = i * HB_THREADS + tid;
            const int px = piece / (CI_T / 8), c = piece % (CI_T / 8);
            const long long n = tile * HB_PIX + px;
            f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (n < a.npix) {
                const long long b = n / HW, r = n - b * HW;
                const int y = (int)(r / a.W), x = (int)(r - (long long)y * a.W);
                v = *(const f16x8*)(xb + b * a.x.img + (long long)(y + dy_t + a.x.P) * a.x.row + (long long)(x + dx_t + a.x.P) * a.x.C + c * 8);
            }
            rx[i] = v;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < DY_PER; ++i) {
            const int piece = i * HB_THREADS + tid;
            if (piece < DY_PIECES) *(LDS_AS f16x8*)(uintptr_t)(dy_base + hb_lds_off(piece / (CO_T / 8), piece % (CO_T / 8))) = rdy[i];
        }
#pragma unroll
        for (int i = 0; i < X_PER; ++i) {
            const int piece = i * HB_THREADS + tid;
            *(LDS_AS f16x8*)(uintptr_t)(x_base + hb_lds_off(piece / (CI_T / 8), piece % (CI_T / 8))) = rx[i];
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
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(dy_base + hb_lds_off(8 * grp + q, chunk) + 8 * (p4 & 1)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(dy_base + hb_lds_off(8 * grp + 4 + q, chunk) + 8 * (p4 & 1)));
            const f16x4 l4 = __builtin_bit_cast(f16x4, lo), h4 = __builtin_bit_cast(f16x4, hi);
            af[i] = (f16x8){l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int chunk = ((wn * NT + j) * 16 + 4 * p4) >> 3;
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(x_base + hb_lds_off(8 * grp + q, chunk) + 8 * (p4 & 1)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(x_base + hb_lds_off(8 * grp + 4 + q, chunk) + 8 * (p4 & 1)));
            const f16x4 l4 = __builtin_bit_cast(f16x4, lo), h4 = __builtin_bit_cast(f16x4, hi);
            bf[j] = (f16x8){l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        __syncthreads();                                              // the images are free for the next tile
    }

    // D[row = co = 4 (lane >> 4) + e][col = ci = lane & 15]
    float* out = a.part + (((long long)slice * a.G + g) * 9 + tap) * a.cout * 256;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = co0 + (wm * MT + i) * 16 + 4 * grp + e, ci = ci0 + (wn * NT + j) * 16 + (lane & 15);
                out[(long long)co * 256 + ci] = acc[i][j][e];
            }
}

// ------------------------------------------------------------------------------------------------ column sums
struct HbColsumArgs {
    HbMap dy;
    int B, H, W, nch;                      // nch channels from dy.coff on (all groups)
    int pix_per_slice;
    long long npix;
    float* part;                           // [slice][nch]
};

// One lane per channel, one workgroup per (256 channels, slice of consecutive pixels); the slices are the colsum's own, at most
// HB_COLSUM_SLICES of ceil(npix / HB_COLSUM_SLICES) pixels: the rule's fixed order is pixel order inside a slice, then slice order.
__global__ __launch_bounds__(HB_COLSUM_CH) void hb_colsum_kernel(const HbColsumArgs a) {
    const int c = blockIdx.x * HB_COLSUM_CH + threadIdx.x, slice = blockIdx.y;
    if (c >= a.nch) return;
    const long long n0 = (long long)slice * a.pix_per_slice;
    long long n1 = n0 + a.pix_per_slice;
    if (n1 > a.npix) n1 = a.npix;
    const long long HW = (long long)a.H * a.W;
    const long long b0 = n0 / HW, r0 = n0 - b0 * HW;
    int y = (int)(r0 / a.W), x = (int)(r0 - (long long)y * a.W);
    const f16* p = a.dy.d + b0 * a.dy.img + (long long)(y + a.dy.P) * a.dy.row + (long long)(x + a.dy.P) * a.dy.C + a.dy.coff + c;
    const long long row_skip = (long long)2 * a.dy.P * a.dy.C;                          // from the last pixel of a row to the first of the next
    const long long img_skip = (long long)2 * a.dy.P * a.dy.row;                        // and of an image to the next image
    float s = 0.f;
    for (long long n = n0; n < n1; ++n) {
        s += (float)*p;
        p += a.dy.C;
        if (++x == a.W) {
            x = 0; p += row_skip;
            if (++y == a.H) { y = 0; p += img_skip; }
        }
    }
    a.part[(long long)slice * a.nch + c] = s;
}

// ------------------------------------------------------------------------------------------------ reduce
struct HbReduceArgs {
    const float* wpart;                    // [slice][g][tap][cout][256]
    const float* bpart;                    // [slice][G][cout]
    const float* s[4];                     // BatchNorm scale per output channel, or NULL
    float* dw[4];                          // (cout_valid, 256, 3, 3) or NULL
    float* db[4];                          // (cout_valid) or NULL
    int cout_valid[4];
    int G, cout, slices, bslices;
    float inv_scale;
    unsigned* nonfinite;
};

__global__ __launch_bounds__(HB_THREADS) void hb_reduce_kernel(const HbReduceArgs a) {
    const int g = blockIdx.y;
    const int nw = a.dw[g] ? a.cout_valid[g] * 256 * 9 : 0, nb = a.db[g] ? a.cout_valid[g] : 0;
    const int i = blockIdx.x * HB_THREADS + threadIdx.x;
    if (i >= nw + nb) return;
    float v = 0.f;
    int co;
    if (i < nw) {
        const int tap = i % 9, ci = (i / 9) % 256;
        co = i / (9 * 256);
        const long long stride = (long long)a.G * 9 * a.cout * 256;
        const float* p = a.wpart + (((long long)g * 9 + tap) * a.cout + co) * 256 + ci;
        for (int sl = 0; sl < a.slices; ++sl) v += p[sl * stride];
    } else {
        co = i - nw;
        const float* p = a.bpart + g * a.cout + co;
        for (int sl = 0; sl < a.bslices; ++sl) v += p[(long long)sl * a.G * a.cout];
    }
    v = v * a.inv_scale;                   // (a power of two: exact)
    if (a.s[g]) v = a.s[g][co] * v;
    if (!(fabsf(v) <= 3.4028234663852886e38f)) atomicAdd(a.nonfinite, 1u);       // an integer counter: the order does not show
    if (i < nw) a.dw[g][i] = v; else a.db[g][co] = v;
}

// ------------------------------------------------------------------------------------------------ dgrad
struct HbDgradArgs {
    HbMap dy, mask, out;                   // mask.d == NULL: no mask
    const f16* wr;                         // [group][tap][ci 256][kc]
    int B, H, W, nsum, dil, kc;            // kc: channels of dY per group (16 or 256)
    long long npix;
};

// a workgroup: 32 HB_DG_PT pixels x 256 ci; wave w: HB_DG_PT 16-pixel tiles from pixel 16 HB_DG_PT (w >> 1), ci 128 (w & 1) ..;
// D[row = ci][col = pixel].  Four pixel tiles per wave: every weight fragment loaded serves four MFMAs.
__global__ __launch_bounds__(HB_THREADS) void hb_dgrad_kernel(const HbDgradArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gout = blockIdx.y;
    const int col = lane & 15, kq = lane >> 4;
    const long long HW = (long long)a.H * a.W;
    const int ci_w = 128 * (wave & 1);
    long long pix[HB_DG_PT];
    int py[HB_DG_PT], pxx[HB_DG_PT], pb[HB_DG_PT];
#pragma unroll
    for (int t = 0; t < HB_DG_PT; ++t) {
        long long n = (long long)blockIdx.x * (32 * HB_DG_PT) + 16 * HB_DG_PT * (wave >> 1) + 16 * t + col;
        pix[t] = n;
        if (n >= a.npix) n = a.npix - 1;                                // a copy of the last pixel: computed, never stored
        const long long b = n / HW, r = n - b * HW;
        pb[t] = (int)b; py[t] = (int)(r / a.W); pxx[t] = (int)(r - (long long)py[t] * a.W);
    }
    f32x4 acc[8][HB_DG_PT];
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int t = 0; t < HB_DG_PT; ++t) acc[c][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool half_k = a.kc == 16;                                     // 16 channels per tap: lanes with k >= 16 feed zeros
    const bool live = !half_k || kq < 2;
    const int ksteps = half_k ? 1 : a.kc / 32;
    for (int gs = 0; gs < a.nsum; ++gs) {
        const int gi = gout + gs;
        const f16* dyb = a.dy.d + a.dy.coff + gi * a.dy.gstride + 8 * kq;
        const f16* wb = a.wr + (long long)gi * 9 * 256 * a.kc + (long long)(ci_w + col) * a.kc + 8 * kq;
        for (int tap = 0; tap < 9; ++tap) {
            const int oy = (tap / 3 - 1) * a.dil, ox = (tap % 3 - 1) * a.dil;
            const f16* yp[HB_DG_PT];
#pragma unroll
            for (int t = 0; t < HB_DG_PT; ++t)
                yp[t] = dyb + pb[t] * a.dy.img + (long long)(py[t] - oy + a.dy.P) * a.dy.row + (long long)(pxx[t] - ox + a.dy.P) * a.dy.C;
            const f16* wt = wb + (long long)tap * 256 * a.kc;
            for (int ks = 0; ks < ksteps; ++ks) {
                f16x8 bf[HB_DG_PT], af[8];
                const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int t = 0; t < HB_DG_PT; ++t) bf[t] = live ? *(const f16x8*)(yp[t] + ks * 32) : zero;
#pragma unroll
                for (int c = 0; c < 8; ++c) af[c] = live ? *(const f16x8*)(wt + (long long)c * 16 * a.kc + ks * 32) : zero;
#pragma unroll
                for (int c = 0; c < 8; ++c)
#pragma unroll
                    for (int t = 0; t < HB_DG_PT; ++t) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[c], bf[t], acc[c][t], 0, 0, 0);
            }
        }
    }
    // lane: pixel `col` of tile t, channels ci_w + 16 c + 4 kq .. + 3
#pragma unroll
    for (int t = 0; t < HB_DG_PT; ++t) {
        if (pix[t] >= a.npix) continue;
        const long long at_o = pb[t] * a.out.img + (long long)(py[t] + a.out.P) * a.out.row + (long long)(pxx[t] + a.out.P) * a.out.C + a.out.coff + gout * a.out.gstride;
        const long long at_m = a.mask.d ? pb[t] * a.mask.img + (long long)(py[t] + a.mask.P) * a.mask.row + (long long)(pxx[t] + a.mask.P) * a.mask.C + a.mask.coff + gout * a.mask.gstride : 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int ch = ci_w + 16 * c + 4 * kq;
            f16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (f16)acc[c][t][e];
            if (a.mask.d) {
                const f16x4 m = *(const f16x4*)(a.mask.d + at_m + ch);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = m[e] > (f16)0.0f ? v[e] : (f16)0.0f;
            }
            *(f16x4*)((f16*)a.out.d + at_o + ch) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ refresh
// packed[i] = fp16(fp32(w[perm[i]] * s[c])) (kind 0) or fp32((b[perm[i]] - mean[c]) * s[c] + beta[c]) (kind 1), c = scale_of[perm[i]],
// in fp64 as the host fold (plan.fold_bn) forms them; perm[i] < 0: a padding element, zero.
__global__ __launch_bounds__(HB_THREADS) void hb_refresh_kernel(const rtm3d_hb_refresh_job* __restrict__ jobs, const float* __restrict__ arena,
                                                                const int* __restrict__ scale_of, const double* __restrict__ bn) {
#pragma clang fp contract(off)
    const rtm3d_hb_refresh_job j = jobs[blockIdx.y];
    const int* perm = (const int*)j.perm;
    for (long long i = (long long)blockIdx.x * HB_THREADS + threadIdx.x; i < j.n; i += (long long)gridDim.x * HB_THREADS) {
        const int src = perm[i];
        double v = 0.0;
        if (src >= 0) {
            const double* c = bn + 3 * (long long)scale_of[src];
            v = (double)arena[src];
            v = j.kind == 0 ? v * c[0] : (v - c[1]) * c[0] + c[2];
        }
        if (j.kind == 0) ((f16*)j.dst)[i] = (f16)(float)v; else ((float*)j.dst)[i] = (float)v;
    }
}

// ---------------------------------------------------------------------------------------------------- host
extern void rt_set_error(const char* fmt, ...);

#define HB_MAX_DIM 16384
#define HB_MAX_PIX (1LL << 31)

extern "C" int rtm3d_head_backward_slices(long long npix, int want, int* n_slices, int* tiles_per_slice) {
    const char* who = "head_backward_slices";
    if (!n_slices || !tiles_per_slice) { rt_set_error("%s: null pointer", who); return RTM3D_HB_E_NULL; }
    if (npix < 1 || npix >= HB_MAX_PIX) { rt_set_error("%s: %lld pixels, a launch takes 1 .. 2^31 - 1", who, npix); return RTM3D_HB_E_SHAPE; }
    if (want < 1 || want > RTM3D_HB_MAX_SLICES) { rt_set_error("%s: %d slices asked for, a launch takes 1 .. %d", who, want, RTM3D_HB_MAX_SLICES); return RTM3D_HB_E_SLICES; }
    const long long ntiles = (npix + HB_PIX - 1) / HB_PIX;
    const long long tps = (ntiles + want - 1) / want;
    *tiles_per_slice = (int)tps;
    *n_slices = (int)((ntiles + tps - 1) / tps);
    return 0;
}

static int hb_shape(const char* who, int B, int H, int W, int G) {
    if (B < 1 || H < 1 || W < 1 || B > HB_MAX_DIM || H > HB_MAX_DIM || W > HB_MAX_DIM || (long long)B * H * W >= HB_MAX_PIX) {
        rt_set_error("%s: B, H, W = %d, %d, %d: each must be 1 .. %d and B * H * W below 2^31", who, B, H, W, HB_MAX_DIM); return RTM3D_HB_E_SHAPE;
    }
    if (G != 1 && G != 2 && G != 4) { rt_set_error("%s: %d head branches, the kernels take 1, 2 or 4", who, G); return RTM3D_HB_E_GROUPS; }
    return 0;
}

extern "C" size_t rtm3d_head_backward_workspace_bytes(int G, int n_slices) {
    if ((G != 1 && G != 2 && G != 4) || n_slices < 1 || n_slices > RTM3D_HB_MAX_SLICES) return 0;
    return ((size_t)n_slices * G * 9 * 256 * 256 + (size_t)HB_COLSUM_SLICES * G * 256) * sizeof(float);
}

extern "C" int rtm3d_head_backward_check(int B, int H, int W, int G, const int* K, int num_conv, float grad_scale) {
    const char* who = "head_backward_check";
    if (!K) { rt_set_error("%s: null pointer", who); return RTM3D_HB_E_NULL; }
    if (int rc = hb_shape(who, B, H, W, G)) return rc;
    for (int g = 0; g < G; ++g)
        if (K[g] < 1 || K[g] > 16) { rt_set_error("%s: head %d has %d output channels, the final-conv kernels take 1 .. 16", who, g, K[g]); return RTM3D_HB_E_CHANNELS; }
    if (num_conv < 1) { rt_set_error("%s: HEADER_NUM_CONV = %d, must be >= 1", who, num_conv); return RTM3D_HB_E_NUM_CONV; }
    int ex = 0;
    if (!(grad_scale > 0.f) || !(grad_scale <= 3.4028234663852886e38f) || frexpf(grad_scale, &ex) != 0.5f) {
        rt_set_error("%s: grad_scale = %g is no power of two", who, (double)grad_scale); return RTM3D_HB_E_SCALE;
    }
    return 0;
}

// a map as the kernels read it; refuses what would make a 16-byte access misaligned or leave the tensor
static int hb_map(const char* who, const char* name, const rtm3d_hb_map* m, int B, int H, int W, int G, int width, int need_border, HbMap* o,
                  bool shared_ok = false) {      // shared_ok: gstride 0, every branch reads the same channels (z)
    if (!m || !m->d) { rt_set_error("%s: %s is a NULL pointer", who, name); return RTM3D_HB_E_NULL; }
    if ((uintptr_t)m->d & 15) { rt_set_error("%s: the address of %s is no multiple of 16", who, name); return RTM3D_HB_E_ALIGN; }
    if (m->C < 8 || (m->C & 7) || m->coff < 0 || (m->coff & 7) || m->gstride < 0 || (m->gstride & 7) || (G > 1 && m->gstride < width && !(shared_ok && m->gstride == 0)) ||
        (long long)m->coff + (long long)(G - 1) * m->gstride + width > m->C) {
        rt_set_error("%s: %s: %d groups of %d channels at offset %d, stride %d do not fit %d channels in steps of 8", who, name, G, width, m->coff, m->gstride, m->C);
        return RTM3D_HB_E_CHANNELS;
    }
    if (m->P < need_border || m->P > 64) { rt_set_error("%s: %s has a border of %d pixels, its reader's taps need %d (at most 64)", who, name, m->P, need_border); return RTM3D_HB_E_BORDER; }
    o->d = (const f16*)m->d;
    o->C = m->C; o->P = m->P; o->coff = m->coff; o->gstride = m->gstride;
    o->row = (W + 2 * m->P) * m->C;
    o->img = (long long)(H + 2 * m->P) * o->row;
    (void)B;
    return 0;
}

static int hb_launched(const char* who) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("%s launch: %s", who, hipGetErrorString(e)); return RTM3D_HB_E_LAUNCH; }
    return 0;
}

extern "C" int rtm3d_head_go(void* stream, int B, int H, int W, int G, const int* K, const float* const* d_dlogit, float grad_scale,
                             const rtm3d_hb_map* go) {
    const char* who = "head_go";
    if (!K || !d_dlogit) { rt_set_error("%s: null pointer", who); return RTM3D_HB_E_NULL; }
    if (int rc = rtm3d_head_backward_check(B, H, W, G, K, 1, grad_scale)) return rc;
    HbGoArgs a;
    if (int rc = hb_map(who, "go", go, B, H, W, G, 16, 0, &a.go)) return rc;
    for (int g = 0; g < 4; ++g) {
        a.d[g] = g < G ? d_dlogit[g] : nullptr; a.K[g] = g < G ? K[g] : 0;
        if (g < G && (!a.d[g] || ((uintptr_t)a.d[g] & 3))) { rt_set_error("%s: the gradient of logit map %d is NULL or misaligned", who, g); return a.d[g] ? RTM3D_HB_E_ALIGN : RTM3D_HB_E_NULL; }
    }
    a.B = B; a.H = H; a.W = W; a.G = G; a.S = grad_scale;
    const long long n = (long long)B * H * W * G;
    hipLaunchKernelGGL(hb_go_kernel, dim3((unsigned)((n + HB_THREADS - 1) / HB_THREADS)), dim3(HB_THREADS), 0, (hipStream_t)stream, a);
    return hb_launched(who);
}

extern "C" int rtm3d_head_wgrad(void* stream, int B, int H, int W, int G, int dil, int cout, const int* cout_valid, const rtm3d_hb_map* dy,
                                const rtm3d_hb_map* x, float grad_scale, const float* const* d_s, float* const* d_dw, float* const* d_db,
                                int want_slices, void* d_ws, size_t ws_bytes, unsigned* d_nonfinite) {
    const char* who = "head_wgrad";
    if (!cout_valid || !d_dw || !d_db || !d_ws || !d_nonfinite) { rt_set_error("%s: null pointer", who); return RTM3D_HB_E_NULL; }
    if (int rc = hb_shape(who, B, H, W, G)) return rc;
    if (cout != 16 && cout != 256) { rt_set_error("%s: %d gradient channels per branch, the kernels take 16 (final conv) or 256", who, cout); return RTM3D_HB_E_CHANNELS; }
    if (dil < 1 || dil > 64) { rt_set_error("%s: dilation %d", who, dil); return RTM3D_HB_E_BORDER; }
    int ex = 0;
    if (!(grad_scale > 0.f) || !(grad_scale <= 3.4028234663852886e38f) || frexpf(grad_scale, &ex) != 0.5f) {
        rt_set_error("%s: grad_scale = %g is no power of two", who, (double)grad_scale); return RTM3D_HB_E_SCALE;
    }
    HbWgradArgs w;
    if (int rc = hb_map(who, "dY", dy, B, H, W, G, cout, 0, &w.dy)) return rc;
    if (int rc = hb_map(who, "X", x, B, H, W, G, 256, dil, &w.x, true)) return rc;
    if (G > 1 && dy->gstride != cout) { rt_set_error("%s: dY: the branches' %d channels must be adjacent, their stride is %d", who, cout, dy->gstride); return RTM3D_HB_E_CHANNELS; }
    HbReduceArgs r;
    bool any_w = false, any_b = false;
    for (int g = 0; g < 4; ++g) {
        r.s[g] = g < G && d_s ? d_s[g] : nullptr; r.dw[g] = g < G ? d_dw[g] : nullptr; r.db[g] = g < G ? d_db[g] : nullptr;
        r.cout_valid[g] = g < G ? cout_valid[g] : 0;
        if (g < G && (cout_valid[g] < 1 || cout_valid[g] > cout)) { rt_set_error("%s: branch %d has %d of %d output channels", who, g, cout_valid[g], cout); return RTM3D_HB_E_CHANNELS; }
        if (((uintptr_t)r.s[g] | (uintptr_t)r.dw[g] | (uintptr_t)r.db[g]) & 3) { rt_set_error("%s: a scale or gradient pointer of branch %d is misaligned", who, g); return RTM3D_HB_E_ALIGN; }
        any_w |= r.dw[g] != nullptr; any_b |= r.db[g] != nullptr;
    }
    if (((uintptr_t)d_ws & 15) || ((uintptr_t)d_nonfinite & 3)) { rt_set_error("%s: the workspace or the counter is misaligned", who); return RTM3D_HB_E_ALIGN; }
    const long long npix = (long long)B * H * W;
    int slices = 0, tps = 0;
    if (int rc = rtm3d_head_backward_slices(npix, want_slices, &slices, &tps)) return rc;
    if (ws_bytes < rtm3d_head_backward_workspace_bytes(G, slices)) {
        rt_set_error("%s: the workspace has %zu bytes, %d slices of %d branches need %zu", who, ws_bytes, slices, G, rtm3d_head_backward_workspace_bytes(G, slices));
        return RTM3D_HB_E_WORKSPACE;
    }
    if (!any_w && !any_b) return 0;
    float* wpart = (float*)d_ws;
    float* bpart = wpart + (size_t)slices * G * 9 * 256 * 256;             // (behind the largest weight partials)
    w.B = B; w.H = H; w.W = W; w.G = G; w.dil = dil; w.cout = cout; w.tiles_per_slice = tps; w.npix = npix; w.part = wpart;
    if (any_w) {
        if (cout == 256) hipLaunchKernelGGL((hb_wgrad_kernel<2, 2, 4, 4>), dim3(4, 9 * G, slices), dim3(HB_THREADS), 0, (hipStream_t)stream, w);
        else hipLaunchKernelGGL((hb_wgrad_kernel<1, 4, 1, 4>), dim3(1, 9 * G, slices), dim3(HB_THREADS), 0, (hipStream_t)stream, w);
        if (int rc = hb_launched(who)) return rc;
    }
    const int pps = (int)((npix + HB_COLSUM_SLICES - 1) / HB_COLSUM_SLICES), bslices = (int)((npix + pps - 1) / pps);
    const int nch = G * cout;                                              // (the groups' channels are adjacent: checked above)
    if (any_b) {
        HbColsumArgs c;
        c.dy = w.dy; c.B = B; c.H = H; c.W = W; c.nch = nch; c.pix_per_slice = pps; c.npix = npix; c.part = bpart;
        hipLaunchKernelGGL(hb_colsum_kernel, dim3((nch + HB_COLSUM_CH - 1) / HB_COLSUM_CH, bslices), dim3(HB_COLSUM_CH), 0, (hipStream_t)stream, c);
        if (int rc = hb_launched(who)) return rc;
    }
    r.wpart = wpart; r.bpart = bpart; r.G = G; r.cout = cout; r.slices = slices; r.bslices = bslices;
    r.inv_scale = 1.0f / grad_scale; r.nonfinite = d_nonfinite;
    const int per = cout * 256 * 9 + cout;
    hipLaunchKernelGGL(hb_reduce_kernel, dim3((per + HB_THREADS - 1) / HB_THREADS, G), dim3(HB_THREADS), 0, (hipStream_t)stream, r);
    return hb_launched(who);
}

extern "C" int rtm3d_head_dgrad(void* stream, int B, int H, int W, int n_out, int n_sum, int dil, int kc, const rtm3d_hb_map* dy,
                                const void* d_wr, const rtm3d_hb_map* mask, const rtm3d_hb_map* out) {
    const char* who = "head_dgrad";
    if (!d_wr) { rt_set_error("%s: null pointer", who); return RTM3D_HB_E_NULL; }
    if (int rc = hb_shape(who, B, H, W, n_out)) return rc;
    if (int rc = hb_shape(who, B, H, W, n_sum)) return rc;
    if (n_out > 1 && n_sum > 1) { rt_set_error("%s: %d outputs each summing %d branches", who, n_out, n_sum); return RTM3D_HB_E_GROUPS; }
    if (kc != 16 && kc != 256) { rt_set_error("%s: %d gradient channels per branch, the kernels take 16 (final conv) or 256", who, kc); return RTM3D_HB_E_CHANNELS; }
    if (dil < 1 || dil > 64) { rt_set_error("%s: dilation %d", who, dil); return RTM3D_HB_E_BORDER; }
    if ((uintptr_t)d_wr & 15) { rt_set_error("%s: the address of the weights is no multiple of 16", who); return RTM3D_HB_E_ALIGN; }
    HbDgradArgs a;
    const int ng = n_out > n_sum ? n_out : n_sum;
    if (int rc = hb_map(who, "dY", dy, B, H, W, ng, kc, dil, &a.dy)) return rc;
    if (int rc = hb_map(who, "dX", out, B, H, W, n_out, 256, 0, &a.out)) return rc;
    a.mask.d = nullptr;
    if (mask && mask->d) { if (int rc = hb_map(who, "X", mask, B, H, W, n_out, 256, 0, &a.mask)) return rc; }
    a.wr = (const f16*)d_wr; a.B = B; a.H = H; a.W = W; a.nsum = n_sum; a.dil = dil; a.kc = kc; a.npix = (long long)B * H * W;
    hipLaunchKernelGGL(hb_dgrad_kernel, dim3((unsigned)((a.npix + 32 * HB_DG_PT - 1) / (32 * HB_DG_PT)), n_out), dim3(HB_THREADS), 0, (hipStream_t)stream, a);
    return hb_launched(who);
}

extern "C" int rtm3d_head_refresh_check(int n_jobs, const rtm3d_hb_refresh_job* jobs) {
    const char* who = "head_refresh_check";
    if (!jobs) { rt_set_error("%s: null pointer", who); return RTM3D_HB_E_NULL; }
    if (n_jobs < 1 || n_jobs > RTM3D_HB_MAX_JOBS) { rt_set_error("%s: %d jobs, a launch takes 1 .. %d", who, n_jobs, RTM3D_HB_MAX_JOBS); return RTM3D_HB_E_SLICES; }
    for (int i = 0; i < n_jobs; ++i) {
        const rtm3d_hb_refresh_job& j = jobs[i];
        if (!j.dst || !j.perm) { rt_set_error("%s: job %d: NULL pointer", who, i); return RTM3D_HB_E_NULL; }
        if (j.kind != 0 && j.kind != 1) { rt_set_error("%s: job %d: kind %d is neither 0 (fp16 weights) nor 1 (fp32 biases)", who, i, j.kind); return RTM3D_HB_E_CHANNELS; }
        if (j.n < 1 || j.n >= HB_MAX_PIX) { rt_set_error("%s: job %d: %lld elements", who, i, j.n); return RTM3D_HB_E_SHAPE; }
        if (((uintptr_t)j.dst & (j.kind == 0 ? 1 : 3)) || ((uintptr_t)j.perm & 3)) { rt_set_error("%s: job %d: misaligned pointer", who, i); return RTM3D_HB_E_ALIGN; }
    }
    return 0;
}

extern "C" int rtm3d_head_refresh(void* stream, int n_jobs, const rtm3d_hb_refresh_job* h_jobs, const rtm3d_hb_refresh_job* d_jobs,
                                  const float* d_arena, const int* d_scale_of, const double* d_bn) {
    const char* who = "head_refresh";
    if (!d_jobs || !d_arena || !d_scale_of || !d_bn) { rt_set_error("%s: null pointer", who); return RTM3D_HB_E_NULL; }
    if (int rc = rtm3d_head_refresh_check(n_jobs, h_jobs)) return rc;
    if (((uintptr_t)d_jobs & 7) || ((uintptr_t)d_arena & 3) || ((uintptr_t)d_scale_of & 3) || ((uintptr_t)d_bn & 7)) { rt_set_error("%s: misaligned pointer", who); return RTM3D_HB_E_ALIGN; }
    long long most = 0;
    for (int i = 0; i < n_jobs; ++i) most = h_jobs[i].n > most ? h_jobs[i].n : most;
    long long gx = (most + HB_THREADS - 1) / HB_THREADS;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(hb_refresh_kernel, dim3((unsigned)gx, n_jobs), dim3(HB_THREADS), 0, (hipStream_t)stream, d_jobs, d_arena, d_scale_of, d_bn);
    return hb_launched(who);
}
