// Neck FPN backward (include/rtm3d_hip.h, "neck FPN backward"): the 1x1 convs of the FPN half of the neck - kfpn_head5 and the three
// composed proj + head convs (Cin -> 256) - and the sum of the two gradient paths that meet at kfpn_h*.  The transposed convs kfpn_up*
// between them are neck_backward.hip's rtm3d_neck_deconv_wgrad / _dgrad as they are.  Every product is an fp16 x fp16 MFMA product
// (16x16x32) with fp32 accumulation, no float atomic anywhere: two runs on equal inputs leave equal bytes.
//
//   fb_wgrad_kernel    part[slice][co][ci] = sum_p dY[p][co] X[p][ci]: a GEMM whose K dimension is the pixels of a slice.  The tile
//                      shape and the LDS image are the head backward's (head_backward.hip, "THE LDS IMAGE"): [32 pixels][128 channels],
//                      16-byte chunks XOR'd by the row's key, read back with ds_read_b64_tr_b16.  A workgroup: 128 co x 128 ci; X
//                      is staged as zeros beyond the last pixel and beyond channel Cin, so every transposed read runs with a full EXEC.
//   fb_colsum_kernel   bpart[run][co] = sum_p dY[p][co] over a run of consecutive pixels (the header's 1024-run rule)
//   fb_reduce_kernel   adds the slices / runs in index order, applies inv, writes torch's (256, Cin, 1, 1) order, counts non-finite
//   fb_dgrad_kernel    dX[p][ci] = fp16(mul sum_co dY[p][co] Af[co][ci]): operands straight from global memory in fragment order
//                      (8 consecutive co per lane), no LDS - the head dgrad's schedule with one tap and Cin output channels
//   fb_add_kernel      g[p][c] = fp16(fp32(E[p][c]) + fp32(F[p][c]) r), 16 bytes per lane
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rtm3d_hip.h"

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define LDS_AS __attribute__((address_space(3)))

#define FB_PIX 32                          // pixels of a wgrad tile = the K of one MFMA (the head backward's tile: its slices are reused)
#define FB_THREADS 256
#define FB_CO 256                          // channels of dY
#define FB_TILE 128                        // co and ci of a wgrad workgroup
#define FB_DG_PT 4                         // 16-pixel tiles per wave of the dgrad
#define FB_COLSUM_RUNS 1024                // pixel runs of the bias sums

struct FbMap {                             // rtm3d_hb_map plus the strides the kernels use
    const f16* d;
    long long img;                         // elements per image
    int row;                               // elements per padded row
    int C, P, coff;
};

__device__ __forceinline__ long long fb_at(const FbMap& m, long long n, long long HW, int W) {      // pixel n of B H W -> element offset
    const long long b = n / HW, r = n - b * HW;
    const int y = (int)(r / W), x = (int)(r - (long long)y * W);
    return b * m.img + (long long)(y + m.P) * m.row + (long long)(x + m.P) * m.C + m.coff;
}

// ------------------------------------------------------------------------------------------------ wgrad
struct FbWgradArgs {
    FbMap dy, x;
    int H, W, Cin;
    int tiles_per_slice;
    long long npix;
    float* part;                           // [slice][256][Cin]
};

__device__ __forceinline__ uint32_t fb_lds_off(int row, int chunk) {                 // bytes; chunk 0 .. 15: 16-byte chunk of the 128 channels
    return (uint32_t)(row * 256 + ((chunk ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4));
}

// 2 x 2 waves, each 4 x 4 MFMA tiles of 16 (co) x 16 (ci)
__global__ __launch_bounds__(FB_THREADS) void fb_wgrad_kernel(const FbWgradArgs a) {
    constexpr int PIECES = FB_PIX * FB_TILE / 8, PER = PIECES / FB_THREADS;          // 16-byte pieces of an image; per thread: 2
    __shared__ __attribute__((aligned(16))) f16 lds_dy[FB_PIX * FB_TILE];
    __shared__ __attribute__((aligned(16))) f16 lds_x[FB_PIX * FB_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int co0 = (blockIdx.x & 1) * FB_TILE, ci0 = (blockIdx.x >> 1) * FB_TILE;
    const int slice = blockIdx.z;
    const long long HW = (long long)a.H * a.W;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // transposed-read addresses: lane 4q + p of a 16-lane group names row q, elements 4p .. 4p + 3 of the 16-channel block
    const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
    const uint32_t dy_base = (uint32_t)(uintptr_t)(LDS_AS f16*)lds_dy, x_base = (uint32_t)(uintptr_t)(LDS_AS f16*)lds_x;

    const long long tile0 = (long long)slice * a.tiles_per_slice;
    long long tile1 = tile0 + a.tiles_per_slice;
    const long long ntiles = (a.npix + FB_PIX - 1) / FB_PIX;
    if (tile1 > ntiles) tile1 = ntiles;

    f16x8 rdy[PER], rx[PER];
    auto fetch = [&](long long tile) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int piece = i * FB_THREADS + tid;
            const int px = piece >> 4, c = piece & 15;
            const long long n = tile * FB_PIX + px;
            const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
            f16x8 vy = zero, vx = zero;
            if (n < a.npix) {                                           // beyond the last pixel: zeros
                vy = *(const f16x8*)(a.dy.d + fb_at(a.dy, n, HW, a.W) + co0 + c * 8);
                if (ci0 + c * 8 < a.Cin) vx = *(const f16x8*)(a.x.d + fb_at(a.x, n, HW, a.W) + ci0 + c * 8);      // beyond channel Cin: zeros
            }
            rdy[i] = vy; rx[i] = vx;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int piece = i * FB_THREADS + tid;
            *(LDS_AS f16x8*)(uintptr_t)(dy_base + fb_lds_off(piece >> 4, piece & 15)) = rdy[i];
            *(LDS_AS f16x8*)(uintptr_t)(x_base + fb_lds_off(piece >> 4, piece & 15)) = rx[i];
        }
    };

    if (tile0 < tile1) fetch(tile0);
    for (long long tile = tile0; tile < tile1; ++tile) {              // (uniform trip count: every lane of every wave takes every barrier)
        store();
        __syncthreads();
        if (tile + 1 < tile1) fetch(tile + 1);                        // in flight while this tile is multiplied
        f16x8 af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int chunk = ((wm * 4 + i) * 16 + 4 * p4) >> 3;       // 16-byte chunk of the lane's 4 elements; + 8 bytes for the odd half
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(dy_base + fb_lds_off(8 * grp + q, chunk) + 8 * (p4 & 1)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(dy_base + fb_lds_off(8 * grp + 4 + q, chunk) + 8 * (p4 & 1)));
            const f16x4 l4 = __builtin_bit_cast(f16x4, lo), h4 = __builtin_bit_cast(f16x4, hi);
            af[i] = (f16x8){l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int chunk = ((wn * 4 + j) * 16 + 4 * p4) >> 3;
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(x_base + fb_lds_off(8 * grp + q, chunk) + 8 * (p4 & 1)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(uintptr_t)(x_base + fb_lds_off(8 * grp + 4 + q, chunk) + 8 * (p4 & 1)));
            const f16x4 l4 = __builtin_bit_cast(f16x4, lo), h4 = __builtin_bit_cast(f16x4, hi);
            bf[j] = (f16x8){l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        __syncthreads();                                              // the images are free for the next tile
    }

    // D[row = co = 4 (lane >> 4) + e][col = ci = lane & 15]
    float* out = a.part + (long long)slice * FB_CO * a.Cin;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ci = ci0 + (wn * 4 + j) * 16 + (lane & 15);
            if (ci >= a.Cin) continue;                                  // (the zero-staged channels of the last ci tile)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = co0 + (wm * 4 + i) * 16 + 4 * grp + e;
                out[(long long)co * a.Cin + ci] = acc[i][j][e];
            }
        }
}

// ------------------------------------------------------------------------------------------------ bias sums
struct FbColsumArgs {
    FbMap dy;
    int H, W;
    int pix_per_run;
    long long npix;
    float* part;                           // [run][256]
};

// one lane per channel, one workgroup per run of consecutive pixels: pixel order inside a run (hb_colsum_kernel's walk)
__global__ __launch_bounds__(FB_CO) void fb_colsum_kernel(const FbColsumArgs a) {
    const int c = threadIdx.x, run = blockIdx.x;
    const long long n0 = (long long)run * a.pix_per_run;
    long long n1 = n0 + a.pix_per_run;
    if (n1 > a.npix) n1 = a.npix;
    const long long HW = (long long)a.H * a.W;
    const long long b0 = n0 / HW, r0 = n0 - b0 * HW;
    int y = (int)(r0 / a.W), x = (int)(r0 - (long long)y * a.W);
    const f16* p = a.dy.d + b0 * a.dy.img + (long long)(y + a.dy.P) * a.dy.row + (long long)(x + a.dy.P) * a.dy.C + a.dy.coff + c;
    const long long row_skip = (long long)2 * a.dy.P * a.dy.C;                          // from the last pixel of a row to the first of the next
    const long long img_skip = (long long)2 * a.dy.P * a.dy.row;                        // and of an image to the next image
    float s = 0.f;
    for (long long n = n0; n < n1; n += 16) {                           // sixteen loads in flight, added in pixel order all the same
        f16 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (n + u >= n1) break;
            v[u] = *p;
            p += a.dy.C;
            if (++x == a.W) {
                x = 0; p += row_skip;
                if (++y == a.H) { y = 0; p += img_skip; }
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (n + u < n1) s += (float)v[u];
    }
    a.part[(long long)run * FB_CO + c] = s;
}

// ------------------------------------------------------------------------------------------------ reduce
struct FbReduceArgs {
    const float* wpart;                    // [slice][256][Cin]
    const float* bpart;                    // [run][256]
    float* dw;                             // (256, Cin, 1, 1) or NULL
    float* db;                             // (256) or NULL
    int Cin, slices, runs;
    float inv;
    unsigned* nonfinite;
};

__global__ __launch_bounds__(FB_THREADS) void fb_reduce_kernel(const FbReduceArgs a) {
    const int nw = a.dw ? FB_CO * a.Cin : 0, nb = a.db ? FB_CO : 0;
    const int i = blockIdx.x * FB_THREADS + threadIdx.x;
    if (i >= nw + nb) return;
    // index order, sixteen loads in flight: a thread that waited for each of 1024 bias runs in turn took longer than the GEMM
    const float* p = i < nw ? a.wpart + i : a.bpart + (i - nw);
    const long long stride = i < nw ? (long long)FB_CO * a.Cin : FB_CO;
    const int n = i < nw ? a.slices : a.runs;
    float v = 0.f;
    for (int s0 = 0; s0 < n; s0 += 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (s0 + u < n) t[u] = p[(s0 + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (s0 + u < n) v += t[u];
    }
    v = v * a.inv;                         // (a power of two: exact)
    if (!(fabsf(v) <= 3.4028234663852886e38f)) atomicAdd(a.nonfinite, 1u);       // an integer counter: the order does not show
    if (i < nw) a.dw[i] = v; else a.db[i - nw] = v;
}

// ------------------------------------------------------------------------------------------------ dgrad
struct FbDgradArgs {
    FbMap dy, out;
    const f16* wr;                         // [ci = Cin][co = 256]
    int H, W, Cin;
    float mul;
    long long npix;
};

// a workgroup: 32 FB_DG_PT pixels x all Cin channels, 256 at a time; wave w: FB_DG_PT 16-pixel tiles from pixel 16 FB_DG_PT (w >> 1),
// ci 128 (w & 1) .. of the block of 256; D[row = ci][col = pixel].  Cin is a multiple of 64: a wave's last block may hold 4 or 0
// tiles of 16 ci (wave-uniform), whose operands are neither loaded nor multiplied.
__global__ __launch_bounds__(FB_THREADS) void fb_dgrad_kernel(const FbDgradArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const long long HW = (long long)a.H * a.W;
    long long pix[FB_DG_PT];
    const f16* yp[FB_DG_PT];
    long long at_o[FB_DG_PT];
#pragma unroll
    for (int t = 0; t < FB_DG_PT; ++t) {
        long long n = (long long)blockIdx.x * (32 * FB_DG_PT) + 16 * FB_DG_PT * (wave >> 1) + 16 * t + col;
        pix[t] = n;
        if (n >= a.npix) n = a.npix - 1;                                // a copy of the last pixel: computed, never stored
        yp[t] = a.dy.d + fb_at(a.dy, n, HW, a.W) + 8 * kq;
        at_o[t] = fb_at(a.out, n, HW, a.W);
    }
    for (int cb = 0; cb < a.Cin; cb += 256) {
        const int ci_w = cb + 128 * (wave & 1);
        int nc = (a.Cin - ci_w) / 16;                                   // live 16-ci tiles of this wave: 8, 4 or none
        nc = nc < 0 ? 0 : (nc > 8 ? 8 : nc);
        f32x4 acc[8][FB_DG_PT];
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int t = 0; t < FB_DG_PT; ++t) acc[c][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const f16* wb = a.wr + (long long)(ci_w + col) * FB_CO + 8 * kq;
        for (int ks = 0; ks < FB_CO / 32; ++ks) {
            f16x8 bf[FB_DG_PT], af[8];
#pragma unroll
            for (int t = 0; t < FB_DG_PT; ++t) bf[t] = *(const f16x8*)(yp[t] + ks * 32);
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < nc) af[c] = *(const f16x8*)(wb + (long long)c * 16 * FB_CO + ks * 32);
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < nc)
#pragma unroll
                    for (int t = 0; t < FB_DG_PT; ++t) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[c], bf[t], acc[c][t], 0, 0, 0);
        }
        // lane: pixel `col` of tile t, channels ci_w + 16 c + 4 kq .. + 3
#pragma unroll
        for (int t = 0; t < FB_DG_PT; ++t) {
            if (pix[t] >= a.npix) continue;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (c >= nc) continue;
                f16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (f16)(acc[c][t][e] * a.mul);
                *(f16x4*)((f16*)a.out.d + at_o[t] + ci_w + 16 * c + 4 * kq) = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ add
struct FbAddArgs {
    FbMap e, f, g;
    int H, W;
    float r;
    long long npix;
};

// a thread: 8 channels of a pixel; the 32 lanes of a half wave cover the 256 channels of a pixel
__global__ __launch_bounds__(FB_THREADS) void fb_add_kernel(const FbAddArgs a) {
    const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
    const long long n = i >> 5;
    if (n >= a.npix) return;
    const int c = (int)(i & 31) * 8;
    const long long HW = (long long)a.H * a.W;
    const f16x8 e = *(const f16x8*)(a.e.d + fb_at(a.e, n, HW, a.W) + c);
    const f16x8 f = *(const f16x8*)(a.f.d + fb_at(a.f, n, HW, a.W) + c);
    f16x8 g;
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = (f16)((float)e[k] + (float)f[k] * a.r);
    *(f16x8*)((f16*)a.g.d + fb_at(a.g, n, HW, a.W) + c) = g;
}

// ---------------------------------------------------------------------------------------------------- host
extern void rt_set_error(const char* fmt, ...);

#define FB_MAX_DIM 16384
#define FB_MAX_PIX (1LL << 31)

static bool fb_pow2(float v) {
    int ex = 0;
    return v > 0.f && v <= 3.4028234663852886e38f && frexpf(v, &ex) == 0.5f;
}

static int fb_shape(const char* who, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || B > FB_MAX_DIM || H > FB_MAX_DIM || W > FB_MAX_DIM || (long long)B * H * W >= FB_MAX_PIX) {
        rt_set_error("%s: B, H, W = %d, %d, %d: each must be 1 .. %d and B * H * W below 2^31", who, B, H, W, FB_MAX_DIM); return RTM3D_FB_E_SHAPE;
    }
    return 0;
}

static int fb_cin(const char* who, int Cin) {
    if (Cin < 64 || Cin > 1024 || (Cin & 63)) { rt_set_error("%s: Cin = %d, the kernels take multiples of 64 in 64 .. 1024", who, Cin); return RTM3D_FB_E_CIN; }
    return 0;
}

static int fb_factor(const char* who, const char* name, float v) {
    if (!fb_pow2(v) || !fb_pow2(1.0f / v)) { rt_set_error("%s: %s = %g is no power of two whose reciprocal is an fp32 number", who, name, (double)v); return RTM3D_FB_E_SCALE; }
    return 0;
}

extern "C" int rtm3d_fpn_backward_check(int B, int H, int W, int Cin, float factor) {
    const char* who = "fpn_backward_check";
    if (int rc = fb_shape(who, B, H, W)) return rc;
    if (int rc = fb_cin(who, Cin)) return rc;
    return fb_factor(who, "the factor", factor);
}

static size_t fb_wgrad_bytes(int Cin, int n_slices) { return ((size_t)n_slices * FB_CO * Cin + (size_t)FB_COLSUM_RUNS * FB_CO) * sizeof(float); }

extern "C" size_t rtm3d_fpn_backward_workspace_bytes(int Cin, int n_slices) {
    if (Cin < 64 || Cin > 1024 || (Cin & 63) || n_slices < 1 || n_slices > RTM3D_HB_MAX_SLICES) return 0;
    return fb_wgrad_bytes(Cin, n_slices);
}

// `width` channels of a map from coff on, as the kernels read them; H, W: the map's interior
static int fb_map(const char* who, const char* name, const rtm3d_hb_map* m, int H, int W, int width, FbMap* o) {
    if (!m || !m->d) { rt_set_error("%s: %s is a NULL pointer", who, name); return RTM3D_FB_E_NULL; }
    if ((uintptr_t)m->d & 15) { rt_set_error("%s: the address of %s is no multiple of 16", who, name); return RTM3D_FB_E_ALIGN; }
    if (m->C < width || (m->C & 7) || m->coff < 0 || (m->coff & 7) || (long long)m->coff + width > m->C) {
        rt_set_error("%s: %s: %d channels at offset %d do not fit %d channels in steps of 8", who, name, width, m->coff, m->C); return RTM3D_FB_E_CHANNELS;
    }
    if (m->P < 0 || m->P > 64) { rt_set_error("%s: %s has a border of %d pixels, a map takes 0 .. 64", who, name, m->P); return RTM3D_FB_E_BORDER; }
    o->d = (const f16*)m->d;
    o->C = m->C; o->P = m->P; o->coff = m->coff;
    o->row = (W + 2 * m->P) * m->C;
    o->img = (long long)(H + 2 * m->P) * o->row;
    return 0;
}

static int fb_launched(const char* who) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("%s launch: %s", who, hipGetErrorString(e)); return RTM3D_FB_E_LAUNCH; }
    return 0;
}

extern "C" int rtm3d_fpn_conv1x1_wgrad(void* stream, int B, int H, int W, int Cin, const rtm3d_hb_map* x, const rtm3d_hb_map* dy, float inv,
                                       float* d_dA, float* d_db, int want_slices, void* d_ws, size_t ws_bytes, unsigned* d_nonfinite) {
    const char* who = "fpn_conv1x1_wgrad";
    if (!x || !dy || !d_ws || !d_nonfinite) { rt_set_error("%s: null pointer", who); return RTM3D_FB_E_NULL; }
    if (int rc = fb_shape(who, B, H, W)) return rc;
    if (int rc = fb_cin(who, Cin)) return rc;
    if (int rc = fb_factor(who, "inv", inv)) return rc;
    FbWgradArgs w;
    if (int rc = fb_map(who, "X", x, H, W, Cin, &w.x)) return rc;
    if (int rc = fb_map(who, "dY", dy, H, W, FB_CO, &w.dy)) return rc;
    if (((uintptr_t)d_ws & 15) || ((uintptr_t)d_dA & 15) || ((uintptr_t)d_db & 3) || ((uintptr_t)d_nonfinite & 3)) {
        rt_set_error("%s: the workspace, a gradient or the counter is misaligned", who); return RTM3D_FB_E_ALIGN;
    }
    const long long npix = (long long)B * H * W;
    int slices = 0, tps = 0;
    if (rtm3d_head_backward_slices(npix, want_slices, &slices, &tps)) return RTM3D_FB_E_SLICES;      // (the message is the callee's)
    if (ws_bytes < fb_wgrad_bytes(Cin, slices)) {
        rt_set_error("%s: the workspace has %zu bytes, %d slices of %d channels need %zu", who, ws_bytes, slices, Cin, fb_wgrad_bytes(Cin, slices));
        return RTM3D_FB_E_WORKSPACE;
    }
    if (!d_dA && !d_db) return 0;
    float* wpart = (float*)d_ws;
    float* bpart = wpart + (size_t)slices * FB_CO * Cin;
    w.H = H; w.W = W; w.Cin = Cin; w.tiles_per_slice = tps; w.npix = npix; w.part = wpart;
    if (d_dA) {
        hipLaunchKernelGGL(fb_wgrad_kernel, dim3(2 * ((Cin + FB_TILE - 1) / FB_TILE), 1, slices), dim3(FB_THREADS), 0, (hipStream_t)stream, w);
        if (int rc = fb_launched(who)) return rc;
    }
    const int ppr = (int)((npix + FB_COLSUM_RUNS - 1) / FB_COLSUM_RUNS), runs = (int)((npix + ppr - 1) / ppr);
    if (d_db) {
        FbColsumArgs c;
        c.dy = w.dy; c.H = H; c.W = W; c.pix_per_run = ppr; c.npix = npix; c.part = bpart;
        hipLaunchKernelGGL(fb_colsum_kernel, dim3(runs), dim3(FB_CO), 0, (hipStream_t)stream, c);
        if (int rc = fb_launched(who)) return rc;
    }
    FbReduceArgs r;
    r.wpart = wpart; r.bpart = bpart; r.dw = d_dA; r.db = d_db; r.Cin = Cin; r.slices = slices; r.runs = runs; r.inv = inv; r.nonfinite = d_nonfinite;
    const int per = FB_CO * Cin + FB_CO;
    hipLaunchKernelGGL(fb_reduce_kernel, dim3((per + FB_THREADS - 1) / FB_THREADS), dim3(FB_THREADS), 0, (hipStream_t)stream, r);
    return fb_launched(who);
}

extern "C" int rtm3d_fpn_conv1x1_dgrad(void* stream, int B, int H, int W, int Cin, const rtm3d_hb_map* dy, const void* d_wr, float mul,
                                       const rtm3d_hb_map* dx) {
    const char* who = "fpn_conv1x1_dgrad";
    if (!dy || !d_wr || !dx) { rt_set_error("%s: null pointer", who); return RTM3D_FB_E_NULL; }
    if (int rc = fb_shape(who, B, H, W)) return rc;
    if (int rc = fb_cin(who, Cin)) return rc;
    if (int rc = fb_factor(who, "mul", mul)) return rc;
    if ((uintptr_t)d_wr & 15) { rt_set_error("%s: the address of the weights is no multiple of 16", who); return RTM3D_FB_E_ALIGN; }
    FbDgradArgs a;
    if (int rc = fb_map(who, "dY", dy, H, W, FB_CO, &a.dy)) return rc;
    if (int rc = fb_map(who, "dX", dx, H, W, Cin, &a.out)) return rc;
    a.wr = (const f16*)d_wr; a.H = H; a.W = W; a.Cin = Cin; a.mul = mul; a.npix = (long long)B * H * W;
    hipLaunchKernelGGL(fb_dgrad_kernel, dim3((unsigned)((a.npix + 32 * FB_DG_PT - 1) / (32 * FB_DG_PT))), dim3(FB_THREADS), 0, (hipStream_t)stream, a);
    return fb_launched(who);
}

extern "C" int rtm3d_fpn_grad_add(void* stream, int B, int H, int W, const rtm3d_hb_map* e, const rtm3d_hb_map* f, float r, const rtm3d_hb_map* g) {
    const char* who = "fpn_grad_add";
    if (!e || !f || !g) { rt_set_error("%s: null pointer", who); return RTM3D_FB_E_NULL; }
    if (int rc = fb_shape(who, B, H, W)) return rc;
    if (int rc = fb_factor(who, "r", r)) return rc;
    FbAddArgs a;
    if (int rc = fb_map(who, "E", e, H, W, FB_CO, &a.e)) return rc;
    if (int rc = fb_map(who, "F", f, H, W, FB_CO, &a.f)) return rc;
    if (int rc = fb_map(who, "g", g, H, W, FB_CO, &a.g)) return rc;
    a.H = H; a.W = W; a.r = r; a.npix = (long long)B * H * W;
    hipLaunchKernelGGL(fb_add_kernel, dim3((unsigned)((a.npix * 32 + FB_THREADS - 1) / FB_THREADS)), dim3(FB_THREADS), 0, (hipStream_t)stream, a);
    return fb_launched(who);
}
