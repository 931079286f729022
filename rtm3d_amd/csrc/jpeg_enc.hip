// JPEG encoding, device side (include/rtm3d_hip.h, "JPEG encoding"): tightly packed uint8 (h, w, 3) frames become the
// coefficient buffers the host's Huffman encoder (jpeg_host.cpp) reads - RGB -> YCbCr, edge replication, chroma downsampling,
// the 8 x 8 forward DCT and the quantisation in ONE launch per chunk of FRAME_CHUNK frames (frame_chunks.h); the descriptors and the
// two tables (with their division multipliers, jpeg_quant.h) travel by value: no copy, no memset, no synchronisation.  The
// chain rtm3d_frames_jpeg_encode and its two halves are here too.  The buffer is the decoder's (jpeg.hip reads it back).
//
// Mapping (rtm3d_frames_jpeg_fdct_plan returns the same numbers): workgroup blockIdx.x of frame blockIdx.y takes the tile of
// JPE_TW x JPE_TH pixels at (JPE_TW * (t % tiles_x), JPE_TH * (t / tiles_x)) - whole MCUs in every mode, so downsampling
// needs nothing from a neighbouring tile.
//   1. Samples.  Thread (rx, ry) = (tid % 16, tid / 16) reads pixels 8 rx .. + 7 of rows 4 ry .. + 3 of the tile: the 24 bytes of
//      a row of its run as the aligned dwords around them (any source address), adjacent lanes adjacent runs, so a wave reads
//      whole rows of 384 contiguous bytes.  Edges are clamped indices in libjpeg's order, never a padded copy: column
//      min(x, w - 1), row min(y, h - 1) at full resolution, and for 4:2:0 the chroma row is clamped FIRST in the downsampled
//      plane (j' = min(j, ch - 1)) and then its two source rows min(2 j' + k, h - 1) - where those are not the run's own rows
//      (below the picture, h even) they are read again.  Y, and Cb / Cr after the 2 x 1 or 2 x 2 average with libjpeg's
//      alternating bias, go to LDS as 8-byte (subsampled chroma: 4-byte) writes.  The whole tile is filled, so every block
//      under it finds its samples.
//   2. Blocks.  The blocks under the tile are tasks, one per thread and step: 16 x 8 of Y, then those of Cb and Cr (16 x 8,
//      8 x 8 or 8 x 4 each).  A thread reads its block's 8 rows as 8-byte LDS reads, keeps the 64 values in registers - every
//      index a constant after unrolling, pass 1 along the rows, pass 2 down the columns - quantises with one multiplication
//      per coefficient and writes the block's 128 bytes as eight 16-byte stores.  Tasks 0 .. 127 are the Y blocks - two whole
//      waves - and both chroma components share a table, so the table is uniform over a wave and is read through scalar
//      loads from the kernel arguments.  A block of the padded grid outside the component's REAL grid is written as zeros;
//      tile 0 also writes the three tables: the whole buffer is defined.
// LDS row stride.  A thread's 8-byte read of row r of block (bx, by) is at ((8 by + r) * stride + 8 bx); ds_read_b64 is served
// in halves of 32 lanes over 64 banks of 4 bytes.  With 16 blocks in a tile row a half holds bx = 0 .. 15 (32 banks) of two
// by: a stride of 128 would put both on the same banks (8 * 128 = 4 * 256), 144 = 128 + 16 puts the second 128 bytes - 32
// banks - further (8 * 144 = 4 * 256 + 128): conflict-free.  With 8 blocks in a row (subsampled chroma) a half holds bx = 0 .. 7
// (16 banks) of four by, and 72 = 64 + 8 steps 64 bytes per by (8 * 72 = 2 * 256 + 64): conflict-free again.  So the stride
// is the row's width plus an eighth of it, which also keeps every row 8-byte aligned.
// Integer code only, all of it on unsigned values where a sign could shift: the rule's arithmetic >> is made explicit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtm3d_hip.h"
#include "frame_chunks.h"
#include "jpeg_quant.h"

#define JPE_TW 128
#define JPE_TH 64
#define JPE_PX 8
#define JPE_ROWS 4
#define JPE_THREADS 256
#define JPE_MAX_SIDE 16384
#define JPE_YBW (JPE_TW / 8)                             // blocks of Y under a tile
#define JPE_YBH (JPE_TH / 8)
#define JPE_STRIDE(wd) ((wd) + (wd) / 8)                 // LDS bytes of a row of wd samples (see above)
#define JPE_YS JPE_STRIDE(JPE_TW)
#define JPE_CMAX (JPE_YS * JPE_TH)                       // bytes of a chroma tile in LDS: 4:4:4 is the largest
static_assert(JPE_THREADS == (JPE_TW / JPE_PX) * (JPE_TH / JPE_ROWS), "one run of JPE_PX x JPE_ROWS pixels per thread");
static_assert(JPE_TW % 16 == 0 && JPE_TH % 16 == 0 && JPE_ROWS == 4 && JPE_PX == 8, "whole MCUs under a tile; two 4:2:0 chroma rows per run");
static_assert(JPE_YBW * JPE_YBH == 128, "the Y blocks of a tile are two whole waves: the table of a task is uniform over a wave");
static_assert(JPE_YS % 8 == 0 && JPE_STRIDE(JPE_TW / 2) % 8 == 0, "8-byte LDS accesses");

struct JpeFrame {                        // 32 B
    const uint8_t* src;
    int16_t* coef;
    int h, w, mode, pad;
};
struct JpeBatch { JpeFrame f[FRAME_CHUNK]; };            // 1 KB of kernel arguments
struct JpeTables { uint32_t q[2][64], m[2][64]; };       // 1 KB: luma, chroma in natural order; m = jpeg_quant_multiplier(q)

// ---- pixels x0 .. x0 + 7 of the row at `row` (columns clamped to w - 1), each byte0 | byte1 << 8 | byte2 << 16
__device__ __forceinline__ void load_run(const uint8_t* row, int x0, int w, uint32_t (&px)[JPE_PX]) {
    if (x0 + JPE_PX <= w) {
        const uint8_t* p = row + 3 * (size_t)x0;
        const uint32_t a = (uint32_t)((uintptr_t)p & 3);
        const uint32_t* d = (const uint32_t*)(p - a);                      // the aligned dwords that hold the 24 bytes: 6, or 7 when a != 0
        uint32_t v[7];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = d[i];
        v[6] = a ? d[6] : 0u;                                              // (byte p + 23 lies in it exactly when a != 0)
        uint32_t s[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = __builtin_amdgcn_alignbyte(v[i + 1], v[i], a);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            px[4 * g] = s[3 * g] & 0xffffffu;
            px[4 * g + 1] = (s[3 * g] >> 24) | ((s[3 * g + 1] & 0xffffu) << 8);
            px[4 * g + 2] = (s[3 * g + 1] >> 16) | ((s[3 * g + 2] & 0xffu) << 16);
            px[4 * g + 3] = s[3 * g + 2] >> 8;
        }
    } else {
#pragma unroll
        for (int i = 0; i < JPE_PX; ++i) {
            const uint8_t* p = row + 3 * (size_t)min(x0 + i, w - 1);
            px[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
    }
}

// ---- step 1 of the rule; order 0: byte 0 is R
__device__ __forceinline__ void rgb_of(uint32_t px, int order, int& R, int& G, int& B) {
    const int c0 = (int)(px & 255u), c2 = (int)(px >> 16);
    G = (int)((px >> 8) & 255u);
    R = order ? c2 : c0;
    B = order ? c0 : c2;
}
__device__ __forceinline__ uint32_t luma_of(int R, int G, int B) { return (uint32_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16); }
__device__ __forceinline__ uint32_t cb_of(int R, int G, int B) { return (uint32_t)((-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16); }
__device__ __forceinline__ uint32_t cr_of(int R, int G, int B) { return (uint32_t)((32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16); }

__device__ __forceinline__ uint2 pack8(const uint32_t (&v)[8]) {
    return make_uint2(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24), v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24));
}

// ---- one thread's 8 x 4 pixels into the LDS planes.  (x0, y0): its first pixel; (lx0, ly0): the same inside the tile
template <int MODE>
__device__ __forceinline__ void sample_run(const JpeFrame& f, int x0, int y0, int lx0, int ly0, uint8_t* ly, uint8_t* lcb, uint8_t* lcr, int order) {
    constexpr int CS = MODE == RTM3D_JPEG_444 ? JPE_YS : JPE_STRIDE(JPE_TW / 2);
    const size_t pitch = (size_t)f.w * 3;
    const int ch = MODE == RTM3D_JPEG_420 ? (f.h + 1) >> 1 : f.h;
#pragma unroll
    for (int jj = 0; jj < JPE_ROWS / 2; ++jj) {
        uint32_t hb[4], hr[4];                                             // 4:2:0: the horizontal sums of the pair's first row
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = 2 * jj + k, ys = min(y0 + r, f.h - 1);
            uint32_t px[JPE_PX], v[JPE_PX];
            load_run(f.src + (size_t)ys * pitch, x0, f.w, px);
#pragma unroll
            for (int i = 0; i < JPE_PX; ++i) {
                int R, G, B;
                rgb_of(px[i], order, R, G, B);
                v[i] = luma_of(R, G, B);
            }
            *(uint2*)(ly + (ly0 + r) * JPE_YS + lx0) = pack8(v);
            if (MODE == RTM3D_JPEG_GREY) continue;
            if (MODE == RTM3D_JPEG_420) {
                const int crow = min(2 * min((y0 >> 1) + jj, ch - 1) + k, f.h - 1);
                if (crow != ys) load_run(f.src + (size_t)crow * pitch, x0, f.w, px);      // below the picture only
            }
            uint32_t cb[JPE_PX], cr[JPE_PX];
#pragma unroll
            for (int i = 0; i < JPE_PX; ++i) {
                int R, G, B;
                rgb_of(px[i], order, R, G, B);
                cb[i] = cb_of(R, G, B);
                cr[i] = cr_of(R, G, B);
            }
            if (MODE == RTM3D_JPEG_444) {
                *(uint2*)(lcb + (ly0 + r) * CS + lx0) = pack8(cb);
                *(uint2*)(lcr + (ly0 + r) * CS + lx0) = pack8(cr);
            } else if (MODE == RTM3D_JPEG_422) {
                uint32_t ob = 0, orr = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {                              // (x0 / 2 is a multiple of 4: the bias alternates with i)
                    ob |= ((cb[2 * i] + cb[2 * i + 1] + (uint32_t)(i & 1)) >> 1) << (8 * i);
                    orr |= ((cr[2 * i] + cr[2 * i + 1] + (uint32_t)(i & 1)) >> 1) << (8 * i);
                }
                *(uint32_t*)(lcb + (ly0 + r) * CS + (lx0 >> 1)) = ob;
                *(uint32_t*)(lcr + (ly0 + r) * CS + (lx0 >> 1)) = orr;
            } else if (k == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { hb[i] = cb[2 * i] + cb[2 * i + 1]; hr[i] = cr[2 * i] + cr[2 * i + 1]; }
            } else {
                uint32_t ob = 0, orr = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ob |= ((hb[i] + cb[2 * i] + cb[2 * i + 1] + 1u + (uint32_t)(i & 1)) >> 2) << (8 * i);
                    orr |= ((hr[i] + cr[2 * i] + cr[2 * i + 1] + 1u + (uint32_t)(i & 1)) >> 2) << (8 * i);
                }
                *(uint32_t*)(lcb + ((ly0 >> 1) + jj) * CS + (lx0 >> 1)) = ob;
                *(uint32_t*)(lcr + ((ly0 >> 1) + jj) * CS + (lx0 >> 1)) = orr;
            }
        }
    }
}

// ---- the one-dimensional pass of the rule on d0..d7, in place; FIRST: along a row (s = 11), else down a column (s = 15)
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(uint32_t& d0, uint32_t& d1, uint32_t& d2, uint32_t& d3, uint32_t& d4, uint32_t& d5, uint32_t& d6,
                                          uint32_t& d7) {
    constexpr int S = FIRST ? 11 : 15;
    constexpr uint32_t R = 1u << (S - 1);
#define JPE_D(v) (uint32_t)((int32_t)((v) + R) >> S)
    const uint32_t t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d0 = (t10 + t11) << 2; d4 = (t10 - t11) << 2;
    } else {
        d0 = (uint32_t)((int32_t)(t10 + t11 + 2u) >> 2); d4 = (uint32_t)((int32_t)(t10 - t11 + 2u) >> 2);
    }
    uint32_t z1 = (t12 + t13) * 4433u;
    d2 = JPE_D(z1 + t13 * 6270u);
    d6 = JPE_D(z1 - t12 * 15137u);
    z1 = t4 + t7;
    uint32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const uint32_t z5 = (z3 + z4) * 9633u;
    const uint32_t a4 = t4 * 2446u, a5 = t5 * 16819u, a6 = t6 * 25172u, a7 = t7 * 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u;
    z3 = z3 * (0u - 16069u) + z5;
    z4 = z4 * (0u - 3196u) + z5;
    d7 = JPE_D(a4 + z1 + z3); d5 = JPE_D(a5 + z2 + z4); d3 = JPE_D(a6 + z2 + z3); d1 = JPE_D(a7 + z1 + z4);
#undef JPE_D
}

// ---- steps 4 and 5 for one block: 8 rows of 8 samples at in (8-byte aligned), the table T.q[ti] / T.m[ti], 64 int16 to out (16-byte aligned)
__device__ __forceinline__ void fdct_block(const uint8_t* in, int stride, const JpeTables& T, int ti, int16_t* out) {
    uint32_t d[64];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const uint2 s = *(const uint2*)(in + v * stride);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            d[8 * v + i] = ((s.x >> (8 * i)) & 255u) - 128u;
            d[8 * v + 4 + i] = ((s.y >> (8 * i)) & 255u) - 128u;
        }
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) fdct_pass<true>(d[8 * v], d[8 * v + 1], d[8 * v + 2], d[8 * v + 3], d[8 * v + 4], d[8 * v + 5], d[8 * v + 6], d[8 * v + 7]);
#pragma unroll
    for (int u = 0; u < 8; ++u) fdct_pass<false>(d[u], d[8 + u], d[16 + u], d[24 + u], d[32 + u], d[40 + u], d[48 + u], d[56 + u]);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 8 * v + 2 * i;
            const uint32_t lo = (uint32_t)jpeg_quantise((int32_t)d[k], T.q[ti][k], T.m[ti][k]);
            const uint32_t hi = (uint32_t)jpeg_quantise((int32_t)d[k + 1], T.q[ti][k + 1], T.m[ti][k + 1]);
            o[i] = (lo & 0xffffu) | (hi << 16);
        }
        ((uint4*)out)[v] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

__global__ __launch_bounds__(JPE_THREADS) void frames_jpeg_fdct_kernel(JpeBatch fb, JpeTables T, int src_order) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_y[JPE_YS * JPE_TH];
    __shared__ __attribute__((aligned(16))) uint8_t lds_c[2][JPE_CMAX];
    const JpeFrame& f = fb.f[blockIdx.y];
    const int tiles_x = (f.w + JPE_TW - 1) / JPE_TW, tiles_y = (f.h + JPE_TH - 1) / JPE_TH;
    const int t = (int)blockIdx.x;
    if (t >= tiles_x * tiles_y) return;                                    // (a frame smaller than the chunk's largest): the whole workgroup
    const int tyi = t / tiles_x;
    const int tx0 = (t - tyi * tiles_x) * JPE_TW, ty0 = tyi * JPE_TH;
    // the geometry of the mode, uniform over the workgroup
    const int mode = f.mode;
    const int hx = (mode == RTM3D_JPEG_422 || mode == RTM3D_JPEG_420) ? 2 : 1, vy = mode == RTM3D_JPEG_420 ? 2 : 1;
    const int ncomp = mode == RTM3D_JPEG_GREY ? 1 : 3;
    const int mcus_x = (f.w + 8 * hx - 1) / (8 * hx), mcus_y = (f.h + 8 * vy - 1) / (8 * vy);
    const int ybw = mcus_x * hx, ybh = mcus_y * vy;                         // the padded block grid of Y; chroma: mcus_x x mcus_y
    const size_t plane_cb = 192 + (size_t)ybw * ybh * 64, plane_c = (size_t)mcus_x * mcus_y * 64;
    const int cw = (f.w + hx - 1) / hx, ch = (f.h + vy - 1) / vy;          // real chroma size
    if (t == 0 && threadIdx.x < 96) {                                      // the three tables, two entries per thread; zero for a component the frame lacks
        const int k = 2 * (int)threadIdx.x, c = k >> 6;
        const uint32_t v = c < ncomp ? T.q[c ? 1 : 0][k & 63] | (T.q[c ? 1 : 0][(k & 63) + 1] << 16) : 0u;
        ((uint32_t*)f.coef)[threadIdx.x] = v;
    }
    const int lx0 = ((int)threadIdx.x % (JPE_TW / JPE_PX)) * JPE_PX, ly0 = ((int)threadIdx.x / (JPE_TW / JPE_PX)) * JPE_ROWS;
    switch (mode) {
        case RTM3D_JPEG_GREY: sample_run<RTM3D_JPEG_GREY>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], src_order); break;
        case RTM3D_JPEG_444: sample_run<RTM3D_JPEG_444>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], src_order); break;
        case RTM3D_JPEG_422: sample_run<RTM3D_JPEG_422>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], src_order); break;
        default: sample_run<RTM3D_JPEG_420>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], src_order); break;
    }
    __syncthreads();
    const int cbw = JPE_YBW / hx, cbh = JPE_YBH / vy;                      // blocks of a chroma tile
    const int cs = mode == RTM3D_JPEG_444 ? JPE_YS : JPE_STRIDE(JPE_TW / 2);
    const int ntasks = JPE_YBW * JPE_YBH + (ncomp == 3 ? 2 * cbw * cbh : 0);
    for (int task = (int)threadIdx.x; task < ntasks; task += JPE_THREADS) {
        int comp, lbx, lby, gbx, gby, rw, rh, bw, bh, stride;
        if (task < JPE_YBW * JPE_YBH) {
            comp = 0; lby = task / JPE_YBW; lbx = task - lby * JPE_YBW;
            gbx = tx0 / 8 + lbx; gby = ty0 / 8 + lby; rw = f.w; rh = f.h; bw = ybw; bh = ybh; stride = JPE_YS;
        } else {
            int k = task - JPE_YBW * JPE_YBH;
            comp = 1 + (k >= cbw * cbh);
            k -= (comp - 1) * cbw * cbh;
            lby = k / cbw; lbx = k - lby * cbw;
            gbx = tx0 / (8 * hx) + lbx; gby = ty0 / (8 * vy) + lby; rw = cw; rh = ch; bw = mcus_x; bh = mcus_y; stride = cs;
        }
        if (gbx >= bw || gby >= bh) continue;                              // outside the padded grid: no such block
        const size_t plane = comp == 0 ? 192 : plane_cb + (comp - 1) * plane_c;
        int16_t* out = f.coef + plane + ((size_t)gby * bw + gbx) * 64;
        if (gbx * 8 >= rw || gby * 8 >= rh) {                              // a padding block
#pragma unroll
            for (int v = 0; v < 8; ++v) ((uint4*)out)[v] = make_uint4(0u, 0u, 0u, 0u);
            continue;
        }
        const int ti = __builtin_amdgcn_readfirstlane(comp != 0);          // uniform over the wave (see the file header)
        const uint8_t* in = (comp == 0 ? lds_y : lds_c[comp - 1]) + lby * 8 * stride + lbx * 8;
        fdct_block(in, stride, T, ti, out);
    }
}

extern int rt_jpeg_frame_layout(int h, int w, int mode, rtm3d_jpeg_stream_info* out, char* msg, size_t msg_len);
extern int rt_jpeg_encode_bound(int h, int w, int mode, int restart, size_t* bytes, char* msg, size_t msg_len);
extern int rt_jpeg_entropy_encode(const int16_t* h_coef, int h, int w, int mode, int restart, uint8_t* out, size_t capacity, size_t* bytes, char* msg,
                                  size_t msg_len);

// every refusal of the header, for the whole batch; tables may be NULL (the plan has none)
static int check_fdct(const char* who, int B, const rtm3d_jpeg_enc_frame* h_frames, bool plan_only, const uint16_t* q_luma, const uint16_t* q_chroma,
                      int src_order) {
    if (refuse_count(who, B) || refuse_null(who, h_frames) || (!plan_only && (refuse_null(who, q_luma) || refuse_null(who, q_chroma)))) return 1;
    if (refuse_order(who, "src_order", src_order)) return 1;
    if (!plan_only)
        for (int t = 0; t < 2; ++t)
            for (int k = 0; k < 64; ++k) {
                const unsigned q = (t ? q_chroma : q_luma)[k];
                if (q < 1 || q > 255) { rt_set_error("%s: entry %d of the %s table is %u; a baseline table holds 1..255", who, k, t ? "chroma" : "luma", q); return 1; }
            }
    for (int b = 0; b < B; ++b) {
        const rtm3d_jpeg_enc_frame& s = h_frames[b];
        if (refuse_side(who, b, s.h, s.w, 1, JPE_MAX_SIDE)) return 1;
        if (s.mode < RTM3D_JPEG_GREY || s.mode > RTM3D_JPEG_420) { rt_set_error("%s: frame %d has the unknown mode %d", who, b, s.mode); return 1; }
        if (refuse_reserved(who, b, s.reserved)) return 1;
        if (plan_only) continue;
        if (!s.d_src) { rt_set_error("%s: frame %d: the source is a NULL pointer", who, b); return 1; }
        if (!s.d_coef) { rt_set_error("%s: frame %d: the coefficient buffer is a NULL pointer", who, b); return 1; }
        if ((uintptr_t)s.d_coef & 15) { rt_set_error("%s: frame %d: the coefficient buffer is not 16-byte aligned", who, b); return 1; }
    }
    return 0;
}

static rtm3d_jpeg_enc_plan plan_chunk(const FrameChunk c, const rtm3d_jpeg_enc_frame* h_frames) {
    rtm3d_jpeg_enc_plan P;
    P.first = c.b0; P.count = c.nb;
    P.tile_w = JPE_TW; P.tile_h = JPE_TH; P.threads = JPE_THREADS;
    P.lds_stride = JPE_YS; P.lds_stride_sub = JPE_STRIDE(JPE_TW / 2);
    P.tiles = 0;
    for (int i = 0; i < c.nb; ++i) {
        const rtm3d_jpeg_enc_frame& s = h_frames[c.b0 + i];
        const int tiles = ((s.w + JPE_TW - 1) / JPE_TW) * ((s.h + JPE_TH - 1) / JPE_TH);                // <= 128 * 256
        if (tiles > P.tiles) P.tiles = tiles;
    }
    P.grid_x = P.tiles;
    P.grid_y = c.nb;
    return P;
}

extern "C" int rtm3d_frames_jpeg_fdct_plan(int B, const rtm3d_jpeg_enc_frame* h_frames, rtm3d_jpeg_enc_plan* out) {
    if (refuse_null("frames_jpeg_fdct_plan", out) || check_fdct("frames_jpeg_fdct_plan", B, h_frames, true, nullptr, nullptr, 0)) return 1;
    for (const FrameChunk c : frame_chunks(B)) out[c.k] = plan_chunk(c, h_frames);
    return 0;
}

extern "C" int rtm3d_frames_jpeg_fdct_check(int B, const rtm3d_jpeg_enc_frame* h_frames, const uint16_t* q_luma, const uint16_t* q_chroma, int src_order) {
    return check_fdct("frames_jpeg_fdct", B, h_frames, false, q_luma, q_chroma, src_order);
}

// one chunk of a batch that is already checked
static void launch_chunk(hipStream_t stream, const FrameChunk c, const rtm3d_jpeg_enc_frame* h_frames, const JpeTables& T, int src_order) {
    const rtm3d_jpeg_enc_plan plan = plan_chunk(c, h_frames);                          // the numbers of rtm3d_frames_jpeg_fdct_plan
    JpeBatch fb;
    for (int i = 0; i < FRAME_CHUNK; ++i) {
        JpeFrame& f = fb.f[i];
        f = JpeFrame{};                                                                // (h = w = 0: no tiles)
        if (i >= c.nb) continue;
        const rtm3d_jpeg_enc_frame& s = h_frames[c.b0 + i];
        f.src = s.d_src; f.coef = s.d_coef; f.h = s.h; f.w = s.w; f.mode = s.mode;
    }
    hipLaunchKernelGGL(frames_jpeg_fdct_kernel, dim3((unsigned)plan.grid_x, (unsigned)plan.grid_y), dim3(JPE_THREADS), 0, stream, fb, T, src_order);
}

static JpeTables make_tables(const uint16_t* q_luma, const uint16_t* q_chroma) {
    JpeTables T;
    for (int k = 0; k < 64; ++k) {
        T.q[0][k] = q_luma[k]; T.q[1][k] = q_chroma[k];
        T.m[0][k] = jpeg_quant_multiplier(q_luma[k]); T.m[1][k] = jpeg_quant_multiplier(q_chroma[k]);
    }
    return T;
}

extern "C" int rtm3d_frames_jpeg_fdct(void* stream, int B, const rtm3d_jpeg_enc_frame* h_frames, const uint16_t* q_luma, const uint16_t* q_chroma,
                                      int src_order) {
    if (rtm3d_frames_jpeg_fdct_check(B, h_frames, q_luma, q_chroma, src_order)) return 1;   // the whole batch, before the first launch
    const JpeTables T = make_tables(q_luma, q_chroma);
    for (const FrameChunk c : frame_chunks(B)) launch_chunk((hipStream_t)stream, c, h_frames, T, src_order);
    return launch_ok("frames_jpeg_fdct");
}

// ---- the chain.  The layout of a batch in d_coef / h_stage: frame b at the int16 offset at[b], the sum of the coef_count before it
static int chain_layout(const char* who, int B, const int* h_hw, int mode, std::vector<size_t>& at) {
    char msg[200];
    if (refuse_count(who, B) || refuse_null(who, h_hw)) return 1;
    at.assign((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) {
        rtm3d_jpeg_stream_info I;
        if (rt_jpeg_frame_layout(h_hw[2 * b], h_hw[2 * b + 1], mode, &I, msg, sizeof(msg))) { rt_set_error("%s: frame %d: %s", who, b, msg); return 1; }
        at[b + 1] = at[b] + I.coef_count;
    }
    return 0;
}

extern "C" int rtm3d_jpeg_encode_workspace_bytes(int B, const int* h_hw, int mode, size_t* bytes) {
    std::vector<size_t> at;
    if (!bytes) { rt_set_error("jpeg_encode_workspace_bytes: null pointer"); return 1; }
    if (chain_layout("jpeg_encode_workspace_bytes", B, h_hw, mode, at)) return 1;
    *bytes = at[B] * sizeof(int16_t);
    return 0;
}

extern "C" int rtm3d_frames_jpeg_encode_queue(void* stream, int B, const uint8_t* const* h_src, const int* h_hw, int mode, const uint16_t* q_luma,
                                              const uint16_t* q_chroma, int src_order, int16_t* d_coef, int16_t* h_stage, size_t capacity) {
    const char* who = "frames_jpeg_encode";
    std::vector<size_t> at;
    if (chain_layout(who, B, h_hw, mode, at)) return 1;
    if (!h_src || !d_coef || !h_stage) { rt_set_error("%s: null pointer", who); return 1; }
    if (((uintptr_t)d_coef & 127) || ((uintptr_t)h_stage & 1)) { rt_set_error("%s: d_coef must be 128-byte aligned, h_stage 2-byte", who); return 1; }
    if (at[B] * sizeof(int16_t) > capacity) {
        rt_set_error("%s: the coefficient buffers hold %zu bytes, the batch needs %zu (rtm3d_jpeg_encode_workspace_bytes)", who, capacity, at[B] * sizeof(int16_t));
        return 1;
    }
    std::vector<rtm3d_jpeg_enc_frame> frames((size_t)B);
    for (int b = 0; b < B; ++b) {
        frames[b].d_src = h_src[b]; frames[b].d_coef = d_coef + at[b];
        frames[b].h = h_hw[2 * b]; frames[b].w = h_hw[2 * b + 1]; frames[b].mode = mode; frames[b].reserved = 0;
    }
    if (check_fdct(who, B, frames.data(), false, q_luma, q_chroma, src_order)) return 1;   // the whole batch, before the first launch
    const JpeTables T = make_tables(q_luma, q_chroma);
    for (const FrameChunk c : frame_chunks(B)) {
        launch_chunk((hipStream_t)stream, c, frames.data(), T, src_order);
        const size_t lo = at[c.b0], hi = at[c.b0 + c.nb];
        hipError_t e = hipMemcpyAsync(h_stage + lo, d_coef + lo, (hi - lo) * sizeof(int16_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
        if (e != hipSuccess) { rt_set_error("%s copy: %s", who, hipGetErrorString(e)); return 1; }
    }
    return launch_ok(who);
}

extern "C" int rtm3d_frames_jpeg_encode_finish(int B, const int* h_hw, int mode, int restart, const int16_t* h_stage, uint8_t* const* h_out,
                                               const size_t* h_out_capacity, size_t* h_out_bytes, int n_threads) {
    const char* who = "frames_jpeg_encode";
    char msg[200];
    std::vector<size_t> at;
    if (chain_layout(who, B, h_hw, mode, at)) return 1;
    if (!h_stage || !h_out || !h_out_capacity || !h_out_bytes) { rt_set_error("%s: null pointer", who); return 1; }
    if (n_threads < 0 || n_threads > 64) { rt_set_error("%s: n_threads = %d (0: min(B, 8); at most 64)", who, n_threads); return 1; }
    for (int b = 0; b < B; ++b) {                                                      // what needs no encoding, for the whole batch
        size_t bound = 0;
        if (rt_jpeg_encode_bound(h_hw[2 * b], h_hw[2 * b + 1], mode, restart, &bound, msg, sizeof(msg))) { rt_set_error("%s: frame %d: %s", who, b, msg); return 1; }
        if (!h_out[b]) { rt_set_error("%s: frame %d: the output is a NULL pointer", who, b); return 1; }
        if (h_out_capacity[b] < bound) {
            rt_set_error("%s: frame %d: the output holds %zu bytes, a stream of this frame may need %zu (rtm3d_jpeg_encode_bound)", who, b, h_out_capacity[b], bound);
            return 1;
        }
    }
    // frames are handed out one by one; the refusal of the lowest frame is the one reported
    int nt = n_threads ? n_threads : (B < 8 ? B : 8);
    if (nt > B) nt = B;
    std::atomic<int> next(0), failed(B);
    std::vector<std::string> errors((size_t)B);
    auto work = [&]() {
        char m[200];
        for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1)) {
            if (rt_jpeg_entropy_encode(h_stage + at[b], h_hw[2 * b], h_hw[2 * b + 1], mode, restart, h_out[b], h_out_capacity[b], &h_out_bytes[b], m, sizeof(m))) {
                errors[b] = m;
                int cur = failed.load();
                while (b < cur && !failed.compare_exchange_weak(cur, b)) {}
            }
        }
    };
    {
        std::vector<std::thread> pool;
        for (int i = 1; i < nt; ++i) {
            try { pool.emplace_back(work); } catch (...) { break; }                    // (no more threads to be had: the others do the work)
        }
        work();
        for (std::thread& th : pool) th.join();
    }
    if (failed.load() < B) { rt_set_error("%s: frame %d: %s", who, failed.load(), errors[failed.load()].c_str()); return 1; }
    return 0;
}

extern "C" int rtm3d_frames_jpeg_encode(void* stream, int B, const uint8_t* const* h_src, const int* h_hw, int mode, const uint16_t* q_luma,
                                        const uint16_t* q_chroma, int src_order, int restart, int16_t* d_coef, int16_t* h_stage, size_t capacity,
                                        uint8_t* const* h_out, const size_t* h_out_capacity, size_t* h_out_bytes, int n_threads) {
    const char* who = "frames_jpeg_encode";
    char msg[200];
    // what the second half would refuse without encoding is refused before the first launch
    if (refuse_count(who, B)) return 1;
    if (!h_hw || !h_out || !h_out_capacity || !h_out_bytes) { rt_set_error("%s: null pointer", who); return 1; }
    if (n_threads < 0 || n_threads > 64) { rt_set_error("%s: n_threads = %d (0: min(B, 8); at most 64)", who, n_threads); return 1; }
    for (int b = 0; b < B; ++b) {
        size_t bound = 0;
        if (rt_jpeg_encode_bound(h_hw[2 * b], h_hw[2 * b + 1], mode, restart, &bound, msg, sizeof(msg))) { rt_set_error("%s: frame %d: %s", who, b, msg); return 1; }
        if (!h_out[b]) { rt_set_error("%s: frame %d: the output is a NULL pointer", who, b); return 1; }
        if (h_out_capacity[b] < bound) {
            rt_set_error("%s: frame %d: the output holds %zu bytes, a stream of this frame may need %zu (rtm3d_jpeg_encode_bound)", who, b, h_out_capacity[b], bound);
            return 1;
        }
    }
    if (rtm3d_frames_jpeg_encode_queue(stream, B, h_src, h_hw, mode, q_luma, q_chroma, src_order, d_coef, h_stage, capacity)) return 1;
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) { rt_set_error("%s event: %s", who, hipGetErrorString(e)); return 1; }
    e = hipEventRecord(ev, (hipStream_t)stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev);                                  // the one wait: the result is host bytes
    (void)hipEventDestroy(ev);
    if (e != hipSuccess) { rt_set_error("%s event: %s", who, hipGetErrorString(e)); return 1; }
    return rtm3d_frames_jpeg_encode_finish(B, h_hw, mode, restart, h_stage, h_out, h_out_capacity, h_out_bytes, n_threads);
}
