// MXFP8 head convolutions (opt-in: Model(head_precision='mxfp8')): block-scaled e4m3 operands on
// v_mfma_scale_f32_32x32x64_f8f6f4, twice the fp16 MFMA rate per clock, half the bytes per MAC.
//
// Storage ("MX8 tensor", runtime.hip): padded NHWC OCP e4m3fn bytes [B][Hp][Wp][C] plus an E8M0 scale plane
// [B][Hp][Wp][C/32] (one power-of-two scale per 32 channels of a pixel; value = e4m3 * 2^(scale - 127)).  The zero border
// (scale 127 = 1.0) is written once at creation, like the fp16 tensors'.
//
// Quantisation rule (OCP MX v1.0), identical on the host (rtm3d_amd/mx8.py):
//   shared_exp = floor(log2(amax of the 32 values)) - 8, clamped to [-127, 127]; an all-zero block gets 127 (2^0);
//   element = round-to-nearest-even e4m3(x / 2^shared_exp), saturated to +-448.
//   Non-finite values: amax is an fmaxf, so a NaN never reaches a scale (an all-NaN block gets 127, an infinity gives 247); a
//   NaN element, like an infinity, becomes sign | 0x7e.  Code 0x7f / 0xff is never written.
//
// conv_mx8_kernel: implicit GEMM, 256 pixels x 256 output channels per workgroup, 8 waves (2 pixel halves x 4 channel
// quarters, 4 x 2 MFMA tiles of 32 x 32 each), K-step = (tap, 64-channel chunk) = ONE scaled MFMA per tile.  Weights and
// pixels are staged by global_load_lds into one __shared__ array (two buffers), the four scale bytes per row and step through
// registers.  Operand maps of the scaled MFMA (measured on the MI355X with one-hot e4m3 data, pinned by tests/test_gpu_mx8.py
// with exact integer data): lane l (h = l >> 5) holds row l & 31 of A (output channel) / column l & 31 of B (pixel); its bytes
// 0-15 are K elements [16 h, 16 h + 16) and bytes 16-31 are [32 + 16 h, 32 + 16 h + 16), so scale block 0 (K 0-31) is spread
// over lanes r and r + 32, and block 1 likewise.  Byte 0 of lane r's scale operand scales block 0 of row r, byte 0 of lane
// r + 32's scales block 1.  C/D: pixel = lane & 31, channel = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), so the 32 channels of a
// pixel that share one output scale live in lanes l, l ^ 32.
#include "common.h"

#define LDS_AS __attribute__((address_space(3)))
#define GLB_AS __attribute__((address_space(1)))

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- quantisation (device half of rtm3d_amd/mx8.py)
// E8M0 byte of a block with largest magnitude `amax` (>= 0, never NaN: the callers take it with fmaxf; +inf gives 247)
__device__ __forceinline__ int mx8_scale_byte(float amax) {
    const uint32_t bits = __float_as_uint(amax);
    const int e = (int)((bits >> 23) & 0xff);
    if (amax == 0.f) return 127;
    if (e == 0) return 0;                              // subnormal amax: floor(log2) - 8 < -127, clamped
    int s = e - 127 - 8;
    s = s < -127 ? -127 : (s > 127 ? 127 : s);
    return s + 127;
}
// 2^(127 - sbyte): the exact multiplier that takes a value to its block's e4m3 domain
__device__ __forceinline__ float mx8_inv_scale(int sbyte) {
    const int s = sbyte - 127;                         // [-127, 127]
    // 2^-s in two exact steps (2^127 is the largest power of two a float holds; 2^-127 is subnormal)
    const int a = -s / 2, b = -s - a;
    return __uint_as_float((uint32_t)(a + 127) << 23) * __uint_as_float((uint32_t)(b + 127) << 23);
}
// round-to-nearest-even OCP e4m3fn of v (already divided by the block scale), saturated to +-448
__device__ __forceinline__ uint32_t mx8_e4m3(float v) {
    const uint32_t sign = (__float_as_uint(v) >> 31) << 7;
    const float a = fabsf(v);
    if (!(a < 448.f)) return sign | 0x7e;               // also rounds (448, 464] to 448 and saturates above
    int e = (int)((__float_as_uint(a) >> 23) & 0xff) - 127;
    e = e < -6 ? -6 : e;                               // e4m3 subnormals share exponent -6 (quantum 2^-9)
    const float q = rintf(a * __uint_as_float((uint32_t)(127 + 3 - e) << 23));   // exact scaling, RNE
    return sign | (uint32_t)(((e + 7) << 3) + (int)q - 8);
}


// one thread per (pixel, 32-channel block)
__global__ __launch_bounds__(256) void quant_mx8_kernel(const QuantMx8Args a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)a.B * a.H * a.W * a.nblk;
    if (i >= total) return;
    const int blk = (int)(i % a.nblk);
    const long long px = i / a.nblk;
    const int x = (int)(px % a.W);
    const long long ny = px / a.W;
    const int y = (int)(ny % a.H), n = (int)(ny / a.H);
    const size_t ip = ((size_t)n * a.in_Hp + y + a.in_P) * a.in_Wp + x + a.in_P;
    const size_t op = ((size_t)n * a.out_Hp + y + a.out_P) * a.out_Wp + x + a.out_P;
    const f16x8* src = (const f16x8*)(a.in + ip * a.in_C + a.in_coff + blk * 32);
    float v[32];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f16x8 h = src[j];
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[j * 8 + k] = (float)h[k]; amax = fmaxf(amax, fabsf(v[j * 8 + k])); }
    }
    const int sb = mx8_scale_byte(amax);
    const float inv = mx8_inv_scale(sb);
    u32x4 w[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) word |= mx8_e4m3(v[j * 4 + k] * inv) << (8 * k);
        w[j >> 2][j & 3] = word;
    }
    u32x4* dst = (u32x4*)(a.out + op * a.out_C + a.out_coff + blk * 32);
    dst[0] = w[0]; dst[1] = w[1];
    a.out_s[op * (a.out_C / 32) + (a.out_coff / 32) + blk] = (uint8_t)sb;
}

hipError_t launch_quant_mx8(const QuantMx8Args& a, hipStream_t s) {
    const long long total = (long long)a.B * a.H * a.W * a.nblk;
    hipLaunchKernelGGL(quant_mx8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- convolution
#define MX_ROWS 256                       // pixels (and output channels) per tile
#define MX_TILE_BYTES (MX_ROWS * 64)      // one K-step of one operand: 256 rows x 64 e4m3
#define MX_BUF_BYTES (2 * MX_TILE_BYTES)  // X then W

// the 16-byte piece `p` of tile row `r` lives at piece p ^ swz(r): rows 4 apart differ in bank group, so the 32 lanes of a
// fragment read (rows r..r+31, pieces 2h, 2h+1) spread over all banks
__device__ __forceinline__ int mx_swz(int r) { return (r >> 2) & 3; }

__global__ __launch_bounds__(512) void conv_mx8_kernel(const ConvMx8Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * MX_BUF_BYTES];
    __shared__ uint16_t sxs[2][MX_ROWS], sws[2][MX_ROWS];       // per row: the scale bytes of the step's two 32-channel blocks
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave & 1, wc = wave >> 1;                    // pixel half, channel quarter

    const int item = xcd_contiguous_index(blockIdx.x, a.MT * a.NT);   // the NT channel tiles of a pixel tile on one XCD
    const int mtile = item / a.NT, ntile = item - mtile * a.NT;
    const int g = blockIdx.y;
    const int T = a.ksteps;
    const int in_sC = a.in_C >> 5;

    // padded input pixel index of tile row r (partial tiles repeat the last pixel; the epilogue stores only m < M)
    auto pix_of = [&](int r) -> uint32_t {
        int m = mtile * MX_ROWS + r;
        m = m < a.M ? m : a.M - 1;
        const int n = m / a.HmWm, rem = m - n * a.HmWm;
        const int y = rem / a.Wm, x = rem - y * a.Wm;
        return (uint32_t)((n * a.in_Hp + y + a.in_P) * a.in_Wp + x + a.in_P);
    };
    // DMA rows of this thread: i * 128 + tid / 4, piece slot tid & 3
    const int drow = tid >> 2, dslot = tid & 3;
    uint32_t xsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = i * 128 + drow;
        xsrc[i] = pix_of(r) * (uint32_t)a.in_C + (uint32_t)a.in_coff[g] + (uint32_t)((dslot ^ mx_swz(r)) * 16);
    }
    // scale rows: threads 0-255 the pixels', 256-511 the weights'
    const int srow = tid & 255;
    const uint32_t spix = pix_of(srow);
    const uint8_t* wtile = a.wgt + ((size_t)(g * a.NT + ntile) * T) * MX_TILE_BYTES;
    const uint8_t* wstile = a.wsc + ((size_t)(g * a.NT + ntile) * T) * (MX_ROWS * 2);

    auto stage = [&](int buf, int k) {
        const int tap = k / a.cpt, q = k - tap * a.cpt;
        const int koff = a.tap_pix[tap] * a.in_C + q * 64;
        uint8_t* dst = lds + buf * MX_BUF_BYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint8_t* src = a.in + (ptrdiff_t)xsrc[i] + koff;
            __builtin_amdgcn_global_load_lds((const GLB_AS void*)src, (LDS_AS void*)(dst + (i * 128 + wave * 16) * 64), 16, 0, 0);
        }
        const uint8_t* ws = wtile + (size_t)k * MX_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = i * 128 + drow;
            __builtin_amdgcn_global_load_lds((const GLB_AS void*)(ws + r * 64 + (dslot ^ mx_swz(r)) * 16),
                                             (LDS_AS void*)(dst + MX_TILE_BYTES + (i * 128 + wave * 16) * 64), 16, 0, 0);
        }
    };
    auto load_scales = [&](int k) -> uint16_t {
        if (tid < 256) {
            const int tap = k / a.cpt, q = k - tap * a.cpt;
            return *(const uint16_t*)(a.in_s + (size_t)(spix + a.tap_pix[tap]) * in_sC + (a.in_coff[g] >> 5) + 2 * q);
        }
        return *(const uint16_t*)(wstile + ((size_t)k * MX_ROWS + srow) * 2);
    };
    auto store_scales = [&](int buf, uint16_t v) {
        if (tid < 256) sxs[buf][srow] = v; else sws[buf][srow] = v;
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][c][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    stage(0, 0);
    store_scales(0, load_scales(0));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int k = 0; k < T; ++k) {
        const int buf = k & 1;
        uint16_t nsc = 0;
        if (k + 1 < T) { stage(buf ^ 1, k + 1); nsc = load_scales(k + 1); }
        const uint8_t* X = lds + buf * MX_BUF_BYTES;
        const uint8_t* Wt = X + MX_TILE_BYTES;
        i32x8 wf[2], xf[4];
        int wsc[2], xsc[4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int r = wc * 64 + c * 32 + fr, s = mx_swz(r);
            const u32x4 lo = *(const u32x4*)(Wt + r * 64 + (fh ^ s) * 16);
            const u32x4 hi = *(const u32x4*)(Wt + r * 64 + ((fh + 2) ^ s) * 16);
            wf[c] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            wsc[c] = (sws[buf][r] >> (8 * fh)) & 0xff;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = wp * 128 + p * 32 + fr, s = mx_swz(r);
            const u32x4 lo = *(const u32x4*)(X + r * 64 + (fh ^ s) * 16);
            const u32x4 hi = *(const u32x4*)(X + r * 64 + ((fh + 2) ^ s) * 16);
            xf[p] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            xsc[p] = (sxs[buf][r] >> (8 * fh)) & 0xff;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                acc[p][c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[c], xf[p], acc[p][c], 0, 0, 0, wsc[c], 0, xsc[p]);
        if (k + 1 < T) store_scales(buf ^ 1, nsc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ---- epilogue: + bias, ReLU, then e4m3 + one scale per 32 channels of a pixel, or fp16
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = mtile * MX_ROWS + wp * 128 + p * 32 + fr;
        const bool live = m < a.M;
        const int mm = live ? m : a.M - 1;
        const int n = mm / a.HmWm, rem = mm - n * a.HmWm;
        const int y = rem / a.Wm, x = rem - y * a.Wm;
        const size_t op = ((size_t)n * a.out_Hp + y + a.out_P) * a.out_Wp + x + a.out_P;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int co0 = ntile * 256 + wc * 64 + c * 32;            // this tile's 32 output channels (within the group)
            float v[16];
            float amax = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                float t = acc[p][c][r] + a.bias[g * a.cout + co];
                if (a.relu) t = fmaxf(t, 0.f);
                v[r] = t;
                amax = fmaxf(amax, fabsf(t));
            }
            const int oc = a.out_coff[g] + co0;
            if (a.out_fp16) {
                f16* o = (f16*)a.out + op * a.out_C + oc + 4 * fh;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (live) *(f16x4*)(o + 8 * j) = (f16x4){(f16)v[4 * j], (f16)v[4 * j + 1], (f16)v[4 * j + 2], (f16)v[4 * j + 3]};
            } else {
                amax = fmaxf(amax, __shfl_xor(amax, 32));               // the other 16 channels of the block: lane ^ 32
                const int sb = mx8_scale_byte(amax);
                const float inv = mx8_inv_scale(sb);
                uint8_t* o = (uint8_t*)a.out + op * a.out_C + oc + 4 * fh;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t word = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) word |= mx8_e4m3(v[4 * j + i] * inv) << (8 * i);
                    if (live) *(uint32_t*)(o + 8 * j) = word;
                }
                if (live && fh == 0) a.out_s[op * (a.out_C >> 5) + (oc >> 5)] = (uint8_t)sb;
            }
        }
    }
}

hipError_t launch_conv_mx8(const ConvMx8Args& a, int groups, hipStream_t s) {
    hipLaunchKernelGGL(conv_mx8_kernel, dim3(a.MT * a.NT, groups), dim3(512), 0, s, a);
    return hipGetLastError();
}
