// JPEG frames, device side (include/rtm3d_hip.h, "JPEG frames"): the coefficient buffers the host's Huffman decoder
// (jpeg_host.cpp) wrote become the tightly packed uint8 (h, w, 3) frames every other entry point reads - dequantisation, the
// 8 x 8 inverse DCT, chroma upsampling and YCbCr -> RGB in ONE launch per chunk of FRAME_CHUNK frames (frame_chunks.h); the per-frame
// descriptors travel by value (no copy, no memset, no synchronisation).  The chain rtm3d_frames_jpeg is here too.
//
// Mapping (rtm3d_frames_jpeg_plan returns the same numbers): workgroup blockIdx.x of frame blockIdx.y takes the tile of
// JPG_TW x JPG_TH pixels at (JPG_TW * (t % tiles_x), JPG_TH * (t / tiles_x)).
//   1. Inverse DCT.  The blocks under the tile are tasks, one per thread and step: 16 x 8 of Y, then those of Cb and Cr -
//      16 x 8 each in 4:4:4; in 4:2:2 8 + 2 columns of blocks, in 4:2:0 (8 + 2) x (4 + 2): "fancy" upsampling reads one chroma
//      sample beyond every tile edge, and the block that holds it is computed again here rather than fetched from a
//      neighbour's result (ONE launch, no sample planes in memory; 248 tasks of a 4:2:0 tile on 256 threads, 192 without the
//      halo).  A thread reads its block's 128 bytes and the component's table as eight 16-byte loads each, keeps the 64
//      values in registers - every index a constant after unrolling, pass 1 down the columns in place, pass 2 along the rows -
//      and writes each finished row of 8 samples to LDS as one 8-byte store.  Blocks outside the component's REAL size
//      (ceil(w H_c / Hmax) x ceil(h V_c / Vmax)) are not computed: nothing reads them, the upsampling clamps its neighbour
//      indices into that size.
//   2. Pixels.  Thread (rx, ry) = (tid % 16, tid / 16) writes pixels 8 rx .. + 7 of rows 4 ry .. + 3 of the tile: Y as 8-byte
//      LDS reads, chroma as 8-byte reads (4:4:4) or the 6 neighbours of its 4 samples per row, byte by byte with clamped
//      indices (4 rows of them in 4:2:0, read once for the thread's 4 output rows).
//   3. Store.  The 24 output bytes of a row of a run leave through store_rgb_run<8> (rgb_runs.h): adjacent lanes write
//      adjacent runs, whole cache lines; exactly h * w * 3 bytes are written.
// Integer code only, all of it on unsigned values: the rule's two's-complement wrap is the language's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtm3d_hip.h"
#include "frame_chunks.h"
#include "rgb_runs.h"

#define JPG_TW 128
#define JPG_TH 64
#define JPG_HALO 1                                       // chroma samples beyond a tile edge that the upsampling reads
#define JPG_PX 8
#define JPG_ROWS 4
#define JPG_THREADS 256
#define JPG_MAX_SIDE 16384
#define JPG_YBW (JPG_TW / 8)                             // blocks of Y under a tile
#define JPG_YBH (JPG_TH / 8)
#define JPG_CMAX (JPG_TW * JPG_TH)                       // bytes of a chroma tile in LDS: 4:4:4 is the largest (4:2:2 80 x 64, 4:2:0 80 x 48)
static_assert(JPG_THREADS == (JPG_TW / JPG_PX) * (JPG_TH / JPG_ROWS), "one run of JPG_PX x JPG_ROWS pixels per thread");
static_assert(JPG_TW % 16 == 0 && JPG_TH % 16 == 0 && JPG_ROWS == 4 && JPG_PX == 8, "whole MCUs under a tile; the 4:2:0 rows of a run");
static_assert((JPG_TW / 2 + 16) * (JPG_TH) <= JPG_CMAX && (JPG_TW / 2 + 16) * (JPG_TH / 2 + 16) <= JPG_CMAX, "the chroma tiles with their halo blocks fit");

struct JpgFrame {                        // 32 B
    const int16_t* coef;
    uint8_t* dst;
    int h, w, mode, pad;
};
struct JpgBatch { JpgFrame f[FRAME_CHUNK]; };            // 1 KB of kernel arguments

// ---- the one-dimensional pass of the rule on x0..x7, in place, outputs (v + 2^(S-1)) >> S
template <int S>
__device__ __forceinline__ void idct_pass(uint32_t& x0, uint32_t& x1, uint32_t& x2, uint32_t& x3, uint32_t& x4, uint32_t& x5, uint32_t& x6,
                                          uint32_t& x7) {
    uint32_t z1 = (x2 + x6) * 4433u;
    const uint32_t t2 = z1 - x6 * 15137u, t3 = z1 + x2 * 6270u;
    const uint32_t t0 = (x0 + x4) << 13, t1 = (x0 - x4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = x7, a1 = x5, a2 = x3, a3 = x1;
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u;
    z3 = z3 * (0u - 16069u) + z5;
    z4 = z4 * (0u - 3196u) + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    constexpr uint32_t R = 1u << (S - 1);
#define JPG_OUT(v) (uint32_t)((int32_t)((v) + R) >> S)
    x0 = JPG_OUT(t10 + a3); x1 = JPG_OUT(t11 + a2); x2 = JPG_OUT(t12 + a1); x3 = JPG_OUT(t13 + a0);
    x4 = JPG_OUT(t13 - a0); x5 = JPG_OUT(t12 - a1); x6 = JPG_OUT(t11 - a2); x7 = JPG_OUT(t10 - a3);
#undef JPG_OUT
}

__device__ __forceinline__ uint32_t sample_of(uint32_t v) { return (uint32_t)min(max((int32_t)(v + 128u), 0), 255); }

// ---- steps 1 and 2 for one block: 64 coefficients at c (16-byte aligned), the table at q, 8 rows of 8 samples to out
__device__ __forceinline__ void idct_block(const int16_t* c, const uint16_t* q, uint8_t* out, int stride) {
    uint32_t d[64];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const uint4 cv = ((const uint4*)c)[v], qv = ((const uint4*)q)[v];
        const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            d[8 * v + 2 * i] = (uint32_t)(int32_t)(int16_t)(cw[i] & 0xffffu) * (qw[i] & 0xffffu);
            d[8 * v + 2 * i + 1] = (uint32_t)((int32_t)cw[i] >> 16) * (qw[i] >> 16);
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) idct_pass<11>(d[u], d[8 + u], d[16 + u], d[24 + u], d[32 + u], d[40 + u], d[48 + u], d[56 + u]);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        idct_pass<18>(d[8 * v], d[8 * v + 1], d[8 * v + 2], d[8 * v + 3], d[8 * v + 4], d[8 * v + 5], d[8 * v + 6], d[8 * v + 7]);
        uint2 r;
        r.x = sample_of(d[8 * v]) | (sample_of(d[8 * v + 1]) << 8) | (sample_of(d[8 * v + 2]) << 16) | (sample_of(d[8 * v + 3]) << 24);
        r.y = sample_of(d[8 * v + 4]) | (sample_of(d[8 * v + 5]) << 8) | (sample_of(d[8 * v + 6]) << 16) | (sample_of(d[8 * v + 7]) << 24);
        *(uint2*)(out + v * stride) = r;                               // 8-byte aligned: stride and the block's column are multiples of 8
    }
}

// ---- step 4 for one pixel; cb and cr already less 128
__device__ __forceinline__ uint32_t colour_px(int y, int cb, int cr, int dst_order) {
    const int R = min(max(y + ((91881 * cr + 32768) >> 16), 0), 255);
    const int B = min(max(y + ((116130 * cb + 32768) >> 16), 0), 255);
    const int G = min(max(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
    return dst_order ? (uint32_t)B | ((uint32_t)G << 8) | ((uint32_t)R << 16) : (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
}

#define JPG_BYTE(v, k) (int)((((k) < 4 ? (v).x : (v).y) >> (8 * ((k) & 3))) & 255u)

// ---- one thread's 8 x 4 pixels.  (x0, y0): its first pixel; (lx0, ly0): the same inside the tile; (cx0, cy0): the chroma sample
// at column / row 0 of the chroma tiles in LDS (halo blocks included); cs: bytes of a chroma row in LDS; (cw, ch): real chroma size
template <int MODE>
__device__ __forceinline__ void pixel_run(const JpgFrame& f, int x0, int y0, int lx0, int ly0, const uint8_t* ly, const uint8_t* lcb,
                                          const uint8_t* lcr, int cx0, int cy0, int cs, int cw, int ch, int dst_order) {
    const int n = min(JPG_PX, f.w - x0), nrows = min(JPG_ROWS, f.h - y0);
    int cb[MODE == RTM3D_JPEG_420 ? 4 : 1][6], cr[MODE == RTM3D_JPEG_420 ? 4 : 1][6];
    int col[6];
    if (MODE == RTM3D_JPEG_422 || MODE == RTM3D_JPEG_420) {
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = min(max((x0 >> 1) - 1 + i, 0), cw - 1) - cx0;
    }
    if (MODE == RTM3D_JPEG_420) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (min(max((y0 >> 1) - 1 + r, 0), ch - 1) - cy0) * cs;
#pragma unroll
            for (int i = 0; i < 6; ++i) { cb[r][i] = lcb[row + col[i]]; cr[r][i] = lcr[row + col[i]]; }
        }
    }
#pragma unroll
    for (int j = 0; j < JPG_ROWS; ++j) {
        if (j >= nrows) break;
        const uint2 yv = *(const uint2*)(ly + (ly0 + j) * JPG_TW + lx0);
        uint32_t px[JPG_PX];
        if (MODE == RTM3D_JPEG_GREY) {
#pragma unroll
            for (int i = 0; i < JPG_PX; ++i) px[i] = (uint32_t)JPG_BYTE(yv, i) * 0x010101u;
        } else if (MODE == RTM3D_JPEG_444) {
            const uint2 bv = *(const uint2*)(lcb + (ly0 + j) * cs + lx0), rv = *(const uint2*)(lcr + (ly0 + j) * cs + lx0);
#pragma unroll
            for (int i = 0; i < JPG_PX; ++i) px[i] = colour_px(JPG_BYTE(yv, i), JPG_BYTE(bv, i) - 128, JPG_BYTE(rv, i) - 128, dst_order);
        } else if (MODE == RTM3D_JPEG_422) {
            const int row = (y0 + j - cy0) * cs;
#pragma unroll
            for (int i = 0; i < 6; ++i) { cb[0][i] = lcb[row + col[i]]; cr[0][i] = lcr[row + col[i]]; }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int b0 = (3 * cb[0][t + 1] + cb[0][t] + 1) >> 2, b1 = (3 * cb[0][t + 1] + cb[0][t + 2] + 2) >> 2;
                const int r0 = (3 * cr[0][t + 1] + cr[0][t] + 1) >> 2, r1 = (3 * cr[0][t + 1] + cr[0][t + 2] + 2) >> 2;
                px[2 * t] = colour_px(JPG_BYTE(yv, 2 * t), b0 - 128, r0 - 128, dst_order);
                px[2 * t + 1] = colour_px(JPG_BYTE(yv, 2 * t + 1), b1 - 128, r1 - 128, dst_order);
            }
        } else {
            const int m = 1 + (j >> 1), o = (j & 1) ? m + 1 : m - 1;       // rows of cb / cr: the sample's own, and the nearer neighbour
            int sb[6], sr[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) { sb[i] = 3 * cb[m][i] + cb[o][i]; sr[i] = 3 * cr[m][i] + cr[o][i]; }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int b0 = (3 * sb[t + 1] + sb[t] + 8) >> 4, b1 = (3 * sb[t + 1] + sb[t + 2] + 7) >> 4;
                const int r0 = (3 * sr[t + 1] + sr[t] + 8) >> 4, r1 = (3 * sr[t + 1] + sr[t + 2] + 7) >> 4;
                px[2 * t] = colour_px(JPG_BYTE(yv, 2 * t), b0 - 128, r0 - 128, dst_order);
                px[2 * t + 1] = colour_px(JPG_BYTE(yv, 2 * t + 1), b1 - 128, r1 - 128, dst_order);
            }
        }
        store_rgb_run<JPG_PX>(f.dst + ((size_t)(y0 + j) * f.w + x0) * 3, px, n);
    }
}

__global__ __launch_bounds__(JPG_THREADS) void frames_jpeg_kernel(JpgBatch fb, int dst_order) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_y[JPG_TW * JPG_TH];
    __shared__ __attribute__((aligned(16))) uint8_t lds_c[2][JPG_CMAX];
    const JpgFrame& f = fb.f[blockIdx.y];
    const int tiles_x = (f.w + JPG_TW - 1) / JPG_TW, tiles_y = (f.h + JPG_TH - 1) / JPG_TH;
    const int t = (int)blockIdx.x;
    if (t >= tiles_x * tiles_y) return;                                    // (a frame smaller than the chunk's largest): the whole workgroup
    const int tyi = t / tiles_x;
    const int tx0 = (t - tyi * tiles_x) * JPG_TW, ty0 = tyi * JPG_TH;
    const int nw = min(JPG_TW, f.w - tx0), nh = min(JPG_TH, f.h - ty0);    // the tile's own pixels
    // the geometry of the mode, uniform over the workgroup
    const int mode = f.mode;
    const int hx = (mode == RTM3D_JPEG_422 || mode == RTM3D_JPEG_420) ? 2 : 1, vy = mode == RTM3D_JPEG_420 ? 2 : 1;
    const int mcus_x = (f.w + 8 * hx - 1) / (8 * hx), mcus_y = (f.h + 8 * vy - 1) / (8 * vy);
    const int ybw = mcus_x * hx;                                           // blocks of a row of the Y plane; chroma: mcus_x
    const size_t plane_cb = 192 + (size_t)ybw * (mcus_y * vy) * 64, plane_c = (size_t)mcus_x * mcus_y * 64;
    const int cw = (f.w + hx - 1) / hx, ch = (f.h + vy - 1) / vy;          // real chroma size
    const int hbx = hx - 1, hby = vy - 1;                                  // halo blocks on each side
    const int cbw = JPG_YBW / hx + 2 * hbx, cbh = JPG_YBH / vy + 2 * hby;  // blocks of a chroma tile in LDS
    const int cs = cbw * 8;
    const int cbx0 = tx0 / (8 * hx) - hbx, cby0 = ty0 / (8 * vy) - hby;    // the chroma block at column / row 0 of the LDS tile
    const int ntasks = JPG_YBW * JPG_YBH + (mode == RTM3D_JPEG_GREY ? 0 : 2 * cbw * cbh);
    for (int task = (int)threadIdx.x; task < ntasks; task += JPG_THREADS) {
        int comp, lbx, lby, gbx, gby, rw, rh, bw, stride;
        if (task < JPG_YBW * JPG_YBH) {
            comp = 0; lby = task / JPG_YBW; lbx = task - lby * JPG_YBW;
            gbx = tx0 / 8 + lbx; gby = ty0 / 8 + lby; rw = f.w; rh = f.h; bw = ybw; stride = JPG_TW;
        } else {
            int k = task - JPG_YBW * JPG_YBH;
            comp = 1 + (k >= cbw * cbh);
            k -= (comp - 1) * cbw * cbh;
            lby = k / cbw; lbx = k - lby * cbw;
            gbx = cbx0 + lbx; gby = cby0 + lby; rw = cw; rh = ch; bw = mcus_x; stride = cs;
        }
        if (gbx < 0 || gby < 0 || gbx * 8 >= rw || gby * 8 >= rh) continue;  // outside the component's real size: never read
        const size_t plane = comp == 0 ? 192 : plane_cb + (comp - 1) * plane_c;
        uint8_t* out = (comp == 0 ? lds_y : lds_c[comp - 1]) + lby * 8 * stride + lbx * 8;
        idct_block(f.coef + plane + ((size_t)gby * bw + gbx) * 64, (const uint16_t*)f.coef + 64 * comp, out, stride);
    }
    __syncthreads();
    const int lx0 = ((int)threadIdx.x % (JPG_TW / JPG_PX)) * JPG_PX, ly0 = ((int)threadIdx.x / (JPG_TW / JPG_PX)) * JPG_ROWS;
    if (lx0 >= nw || ly0 >= nh) return;
    const int cx0 = cbx0 * 8, cy0 = cby0 * 8;
    switch (mode) {
        case RTM3D_JPEG_GREY: pixel_run<RTM3D_JPEG_GREY>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, cw, ch, dst_order); break;
        case RTM3D_JPEG_444: pixel_run<RTM3D_JPEG_444>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, cw, ch, dst_order); break;
        case RTM3D_JPEG_422: pixel_run<RTM3D_JPEG_422>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, cw, ch, dst_order); break;
        default: pixel_run<RTM3D_JPEG_420>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, cw, ch, dst_order); break;
    }
}

extern int rt_jpeg_info(const uint8_t* data, size_t bytes, rtm3d_jpeg_stream_info* out, char* msg, size_t msg_len);
extern int rt_jpeg_entropy_decode(const uint8_t* data, size_t bytes, int16_t* h_coef, size_t capacity, char* msg, size_t msg_len);

// every refusal of the header, for the whole batch; h_dst may be NULL (the plan has no destinations)
static int check_jpeg(const char* who, int B, const rtm3d_jpeg_frame* h_frames, uint8_t* const* h_dst, int dst_order) {
    if (refuse_count(who, B) || refuse_null(who, h_frames) || refuse_order(who, "dst_order", dst_order)) return 1;
    for (int b = 0; b < B; ++b) {
        const rtm3d_jpeg_frame& s = h_frames[b];
        if (refuse_side(who, b, s.h, s.w, 1, JPG_MAX_SIDE)) return 1;
        if (s.mode < RTM3D_JPEG_GREY || s.mode > RTM3D_JPEG_420) { rt_set_error("%s: frame %d has the unknown mode %d", who, b, s.mode); return 1; }
        if (refuse_reserved(who, b, s.reserved)) return 1;
        if (!s.d_coef) { rt_set_error("%s: frame %d: the coefficient buffer is a NULL pointer", who, b); return 1; }
        if ((uintptr_t)s.d_coef & 15) { rt_set_error("%s: frame %d: the coefficient buffer is not 16-byte aligned", who, b); return 1; }
        if (h_dst && refuse_null_dst(who, b, h_dst[b])) return 1;
    }
    return 0;
}

static rtm3d_jpeg_plan plan_chunk(const FrameChunk c, const rtm3d_jpeg_frame* h_frames) {
    rtm3d_jpeg_plan P;
    P.first = c.b0; P.count = c.nb;
    P.tile_w = JPG_TW; P.tile_h = JPG_TH; P.halo = JPG_HALO; P.threads = JPG_THREADS;
    P.tiles = 0;
    for (int i = 0; i < c.nb; ++i) {
        const rtm3d_jpeg_frame& s = h_frames[c.b0 + i];
        const int tiles = ((s.w + JPG_TW - 1) / JPG_TW) * ((s.h + JPG_TH - 1) / JPG_TH);                // <= 128 * 256
        if (tiles > P.tiles) P.tiles = tiles;
    }
    P.grid_x = P.tiles;
    P.grid_y = c.nb;
    return P;
}

extern "C" int rtm3d_frames_jpeg_plan(int B, const rtm3d_jpeg_frame* h_frames, rtm3d_jpeg_plan* out) {
    if (refuse_null("frames_jpeg_plan", out) || check_jpeg("frames_jpeg_plan", B, h_frames, nullptr, 0)) return 1;
    for (const FrameChunk c : frame_chunks(B)) out[c.k] = plan_chunk(c, h_frames);
    return 0;
}

extern "C" int rtm3d_frames_jpeg_check(int B, const rtm3d_jpeg_frame* h_frames, uint8_t* const* h_dst, int dst_order) {
    if (refuse_null("frames_jpeg_idct", h_dst)) return 1;
    return check_jpeg("frames_jpeg_idct", B, h_frames, h_dst, dst_order);
}

// one chunk of a batch that is already checked
static void launch_chunk(hipStream_t stream, const FrameChunk c, const rtm3d_jpeg_frame* h_frames, uint8_t* const* h_dst, int dst_order) {
    const rtm3d_jpeg_plan plan = plan_chunk(c, h_frames);                              // the numbers of rtm3d_frames_jpeg_plan
    JpgBatch fb;
    for (int i = 0; i < FRAME_CHUNK; ++i) {
        JpgFrame& f = fb.f[i];
        f = JpgFrame{};                                                                // (h = w = 0: no tiles)
        if (i >= c.nb) continue;
        const rtm3d_jpeg_frame& s = h_frames[c.b0 + i];
        f.coef = s.d_coef; f.dst = h_dst[c.b0 + i]; f.h = s.h; f.w = s.w; f.mode = s.mode;
    }
    hipLaunchKernelGGL(frames_jpeg_kernel, dim3((unsigned)plan.grid_x, (unsigned)plan.grid_y), dim3(JPG_THREADS), 0, stream, fb, dst_order);
}

extern "C" int rtm3d_frames_jpeg_idct(void* stream, int B, const rtm3d_jpeg_frame* h_frames, uint8_t* const* h_dst, int dst_order) {
    if (rtm3d_frames_jpeg_check(B, h_frames, h_dst, dst_order)) return 1;              // the whole batch, before the first launch
    for (const FrameChunk c : frame_chunks(B)) launch_chunk((hipStream_t)stream, c, h_frames, h_dst, dst_order);
    return launch_ok("frames_jpeg_idct");
}

// ---- the chain: info, refusals, threaded entropy decode, one copy and one launch per chunk
extern "C" int rtm3d_frames_jpeg(void* stream, int B, const uint8_t* const* h_data, const size_t* h_bytes, int16_t* h_stage, int16_t* d_coef,
                                 size_t capacity, uint8_t* const* h_dst, const size_t* h_dst_bytes, int dst_order, int n_threads) {
    char msg[200];
    if (refuse_count("frames_jpeg", B)) return 1;
    if (!h_data || !h_bytes || !h_stage || !d_coef || !h_dst || !h_dst_bytes) { rt_set_error("frames_jpeg: null pointer"); return 1; }
    if (n_threads < 0 || n_threads > 64) { rt_set_error("frames_jpeg: n_threads = %d (0: min(B, 8); at most 64)", n_threads); return 1; }
    if (((uintptr_t)d_coef & 127) || ((uintptr_t)h_stage & 1)) { rt_set_error("frames_jpeg: d_coef must be 128-byte aligned, h_stage 2-byte"); return 1; }
    std::vector<rtm3d_jpeg_stream_info> info((size_t)B);
    std::vector<rtm3d_jpeg_frame> frames((size_t)B);
    std::vector<size_t> at((size_t)B + 1);                                             // int16 offset of every frame's buffer
    at[0] = 0;
    for (int b = 0; b < B; ++b) {
        if (rt_jpeg_info(h_data[b], h_bytes[b], &info[b], msg, sizeof(msg))) { rt_set_error("frames_jpeg: frame %d: %s", b, msg); return 1; }
        const size_t need = (size_t)info[b].h * info[b].w * 3;
        if (h_dst_bytes[b] < need) {
            rt_set_error("frames_jpeg: frame %d: the destination holds %zu bytes, %d x %d x 3 = %zu are written", b, h_dst_bytes[b], info[b].h, info[b].w, need);
            return 1;
        }
        at[b + 1] = at[b] + info[b].coef_count;
        frames[b].d_coef = d_coef + at[b]; frames[b].h = info[b].h; frames[b].w = info[b].w; frames[b].mode = info[b].mode; frames[b].reserved = 0;
    }
    if (at[B] * sizeof(int16_t) > capacity) {
        rt_set_error("frames_jpeg: the coefficient buffers hold %zu bytes, the batch needs %zu (rtm3d_jpeg_workspace_bytes)", capacity, at[B] * sizeof(int16_t));
        return 1;
    }
    if (rtm3d_frames_jpeg_check(B, frames.data(), h_dst, dst_order)) return 1;
    // the entropy decode: frames are handed out one by one; the refusal of the lowest frame is the one reported
    int nt = n_threads ? n_threads : (B < 8 ? B : 8);
    if (nt > B) nt = B;
    std::atomic<int> next(0), failed(B);
    std::vector<std::string> errors((size_t)B);
    auto work = [&]() {
        char m[200];
        for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1)) {
            if (b > failed.load()) continue;                                           // a lower frame is refused already
            if (rt_jpeg_entropy_decode(h_data[b], h_bytes[b], h_stage + at[b], info[b].coef_count, m, sizeof(m))) {
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
    if (failed.load() < B) { rt_set_error("frames_jpeg: frame %d: %s", failed.load(), errors[failed.load()].c_str()); return 1; }
    for (const FrameChunk c : frame_chunks(B)) {
        const size_t lo = at[c.b0], hi = at[c.b0 + c.nb];
        hipError_t e = hipMemcpyAsync(d_coef + lo, h_stage + lo, (hi - lo) * sizeof(int16_t), hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e != hipSuccess) { rt_set_error("frames_jpeg copy: %s", hipGetErrorString(e)); return 1; }
        launch_chunk((hipStream_t)stream, c, frames.data(), h_dst, dst_order);
    }
    return launch_ok("frames_jpeg");
}
