// Pixel formats (include/rtm3d_hip.h, "pixel formats"): camera and decoder surfaces - packed RGB with a row pitch, NV12 / NV21 /
// I420 / P010, YUYV / UYVY, GRAY8 - to the tightly packed uint8 (h, w, 3) frames every other entry point reads.  One launch
// per chunk of FRAME_CHUNK frames (frame_chunks.h), the per-frame descriptors travel by value (no copy, no memset, no synchronisation).
//
// Thread mapping (rtm3d_frames_convert_plan returns the same numbers): a frame is cut into runs of CONV_PX pixels of
// CONV_ROWS consecutive rows (a row pair: a 4:2:0 chroma row is read once); run t = blockIdx.x * CONV_THREADS + threadIdx.x
// of frame blockIdx.y covers pixels 8 * (t % runs_per_row) .. + 7 of rows 2 * (t / runs_per_row), + 1.  Consecutive lanes hold
// consecutive runs of a row, so a wave reads and writes whole cache lines.
//
// Any byte address is legal.  A run is read with 8- or 4-byte loads when its first byte is so aligned and the whole run lies
// inside the row's own bytes, byte by byte otherwise (row tails, odd pitches, odd bases): no read leaves rows x row bytes of
// a plane.  The 24 output bytes of a full run leave through store_rgb_run<8> (rgb_runs.h, shared with lens.hip): as aligned
// dwords - shifted by the destination's misalignment, with a byte-wise head and tail - and a partial run (the row's last)
// byte by byte: exactly h * w * 3 bytes are written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtm3d_hip.h"
#include "frame_chunks.h"
#include "rgb_runs.h"

#define CONV_PX 8
#define CONV_ROWS 2
#define CONV_THREADS 256
#define CONV_MAX_SIDE 16384

// [cy, crv, cgu, cgv, cbu] = round(2^S * v), v from (Kr, Kb) and the range scales (the header's table; tests/pixfmt_ref.py derives
// them again in float64).  Rows 0-3 serve 8-bit samples (S = 16) and, rows 0-1, limited-range 10-bit samples (S = 18: the two
// scales differ by exactly 4); rows 4-5 full-range 10-bit (S = 18).
#define CONV_TABLES                                        \
    {{76309, 104597, -25675, -53279, 132201},  /* BT.601 limited */ \
     {76309, 117489, -13975, -34925, 138438},  /* BT.709 limited */ \
     {65536, 91881, -22553, -46802, 116130},   /* BT.601 full, 8-bit */ \
     {65536, 103206, -12276, -30679, 121609},  /* BT.709 full, 8-bit */ \
     {65344, 91612, -22487, -46664, 115789},   /* BT.601 full, 10-bit */ \
     {65344, 102903, -12240, -30589, 121252}}  /* BT.709 full, 10-bit */
static const int h_conv_tab[6][5] = CONV_TABLES;
__constant__ int c_conv_tab[6][5] = CONV_TABLES;

struct ConvFrame {                       // 64 B
    const uint8_t* p[3];
    uint8_t* dst;
    int pitch[3];
    int h, w, format;
    int table;                           // row of c_conv_tab
    int yo_swap;                         // luma offset (0, 16 or 64) | bit 16: exchange the first and third output byte
};
struct ConvBatch { ConvFrame f[FRAME_CHUNK]; };          // 2 KB of kernel arguments

// ---- N bytes (a multiple of 8) at p into dwords; only the first n are read, the rest are zero
template <int N>
__device__ __forceinline__ void load_run(const uint8_t* p, int n, uint32_t (&v)[N / 4]) {
    const uintptr_t a = (uintptr_t)p;
    if (n == N && (a & 7) == 0) {
#pragma unroll
        for (int i = 0; i < N / 8; ++i) { const uint2 q = ((const uint2*)p)[i]; v[2 * i] = q.x; v[2 * i + 1] = q.y; }
    } else if (n == N && (a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) v[i] = ((const uint32_t*)p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) v[i] = 0;
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i < n) v[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
}
// the four bytes of an I420 chroma run
__device__ __forceinline__ uint32_t load_run4(const uint8_t* p, int n) {
    if (n == 4 && ((uintptr_t)p & 3) == 0) return *(const uint32_t*)p;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) v |= (uint32_t)p[i] << (8 * i);
    return v;
}
#define BYTE_OF(v, k) (int)(((v)[(k) >> 2] >> (8 * ((k) & 3))) & 255u)
#define HALF_OF(v, k) (int)(((v)[(k) >> 1] >> (16 * ((k) & 1))) & 65535u)

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// one chroma sample's share of R, G, B (with the rounding term), reused by every pixel the sample serves
struct Chroma { int r, g, b; };
template <int S>
__device__ __forceinline__ Chroma chroma_of(int U, int V, const int (&c)[5]) {
    Chroma k;
    k.r = c[1] * V + (1 << (S - 1));
    k.g = c[2] * U + c[3] * V + (1 << (S - 1));
    k.b = c[4] * U + (1 << (S - 1));
    return k;
}
template <int S>
__device__ __forceinline__ uint32_t pixel_of(int Y, const Chroma& k, int cy, int yo, bool swap) {
    const int l = cy * (Y - yo);
    const int r = clamp255((l + k.r) >> S), g = clamp255((l + k.g) >> S), b = clamp255((l + k.b) >> S);
    return swap ? (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16) : (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

template <int FMT>
__device__ __forceinline__ void convert_run(const ConvFrame& f, int x0, int y0) {
    const int n = min(CONV_PX, f.w - x0);                      // pixels of this run
    const int nrows = min(CONV_ROWS, f.h - y0);
    const bool swap = (f.yo_swap >> 16) != 0;
    constexpr bool RGB3 = FMT == RTM3D_PIX_RGB24 || FMT == RTM3D_PIX_BGR24, RGB4 = FMT == RTM3D_PIX_RGBA32 || FMT == RTM3D_PIX_BGRA32;
    constexpr bool SEMI = FMT == RTM3D_PIX_NV12 || FMT == RTM3D_PIX_NV21, P10 = FMT == RTM3D_PIX_P010, PLANAR = FMT == RTM3D_PIX_I420;
    constexpr bool PAIRS = FMT == RTM3D_PIX_YUYV || FMT == RTM3D_PIX_UYVY;
    constexpr bool YUV = SEMI || P10 || PLANAR || PAIRS;
    constexpr int S = P10 ? 18 : 16, COFF = P10 ? 512 : 128;
    int c[5] = {0, 0, 0, 0, 0};
    const int yo = f.yo_swap & 0xffff;
    if constexpr (YUV) {
#pragma unroll
        for (int i = 0; i < 5; ++i) c[i] = c_conv_tab[f.table][i];
    }
    const int cw = (f.w + 1) >> 1;
    Chroma k[CONV_PX / 2];
    if constexpr (SEMI) {                                       // Cb Cr (NV12) or Cr Cb (NV21) of chroma row y0 / 2, pairs x0 / 2 ..
        uint32_t v[2];
        load_run<8>(f.p[1] + (size_t)(y0 >> 1) * f.pitch[1] + x0, min(8, 2 * cw - x0), v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = BYTE_OF(v, 2 * i) - COFF, b = BYTE_OF(v, 2 * i + 1) - COFF;
            k[i] = FMT == RTM3D_PIX_NV12 ? chroma_of<S>(a, b, c) : chroma_of<S>(b, a, c);
        }
    }
    if constexpr (P10) {
        uint32_t v[4];
        load_run<16>(f.p[1] + (size_t)(y0 >> 1) * f.pitch[1] + 2 * x0, min(16, 4 * cw - 2 * x0), v);
#pragma unroll
        for (int i = 0; i < 4; ++i) k[i] = chroma_of<S>((HALF_OF(v, 2 * i) >> 6) - COFF, (HALF_OF(v, 2 * i + 1) >> 6) - COFF, c);
    }
    if constexpr (PLANAR) {
        const int m = min(4, cw - (x0 >> 1));
        const uint32_t u = load_run4(f.p[1] + (size_t)(y0 >> 1) * f.pitch[1] + (x0 >> 1), m);
        const uint32_t v = load_run4(f.p[2] + (size_t)(y0 >> 1) * f.pitch[2] + (x0 >> 1), m);
#pragma unroll
        for (int i = 0; i < 4; ++i) k[i] = chroma_of<S>((int)((u >> (8 * i)) & 255u) - COFF, (int)((v >> (8 * i)) & 255u) - COFF, c);
    }
#pragma unroll
    for (int r = 0; r < CONV_ROWS; ++r) {
        if (r >= nrows) break;
        const int y = y0 + r;
        const uint8_t* row = f.p[0] + (size_t)y * f.pitch[0];
        uint32_t px[CONV_PX];
        if constexpr (RGB3) {
            uint32_t v[6];
            load_run<24>(row + 3 * x0, 3 * n, v);
#pragma unroll
            for (int i = 0; i < CONV_PX; ++i) {
                const uint32_t a = BYTE_OF(v, 3 * i), g = BYTE_OF(v, 3 * i + 1), b = BYTE_OF(v, 3 * i + 2);
                px[i] = swap ? b | (g << 8) | (a << 16) : a | (g << 8) | (b << 16);
            }
        } else if constexpr (RGB4) {
            uint32_t v[8];
            load_run<32>(row + 4 * x0, 4 * n, v);
#pragma unroll
            for (int i = 0; i < CONV_PX; ++i)
                px[i] = swap ? ((v[i] >> 16) & 255u) | (v[i] & 0xff00u) | ((v[i] & 255u) << 16) : v[i] & 0xffffffu;
        } else if constexpr (FMT == RTM3D_PIX_GRAY8) {
            uint32_t v[2];
            load_run<8>(row + x0, n, v);
#pragma unroll
            for (int i = 0; i < CONV_PX; ++i) px[i] = (uint32_t)BYTE_OF(v, i) * 0x010101u;
        } else if constexpr (SEMI || PLANAR) {
            uint32_t v[2];
            load_run<8>(row + x0, n, v);
#pragma unroll
            for (int i = 0; i < CONV_PX; ++i) px[i] = pixel_of<S>(BYTE_OF(v, i), k[i >> 1], c[0], yo, swap);
        } else if constexpr (P10) {
            uint32_t v[4];
            load_run<16>(row + 2 * x0, 2 * n, v);
#pragma unroll
            for (int i = 0; i < CONV_PX; ++i) px[i] = pixel_of<S>(HALF_OF(v, i) >> 6, k[i >> 1], c[0], yo, swap);
        } else {                                                // YUYV / UYVY: the pair's own chroma on this row
            uint32_t v[4];
            load_run<16>(row + 2 * x0, min(16, 4 * cw - 2 * x0), v);
            constexpr int YB = FMT == RTM3D_PIX_YUYV ? 0 : 1;   // byte of Y0 inside the pair's four
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const Chroma q = chroma_of<S>(BYTE_OF(v, 4 * i + 1 - YB) - COFF, BYTE_OF(v, 4 * i + 3 - YB) - COFF, c);
                px[2 * i] = pixel_of<S>(BYTE_OF(v, 4 * i + YB), q, c[0], yo, swap);
                px[2 * i + 1] = pixel_of<S>(BYTE_OF(v, 4 * i + 2 + YB), q, c[0], yo, swap);
            }
        }
        store_rgb_run<CONV_PX>(f.dst + ((size_t)y * f.w + x0) * 3, px, n);
    }
}

__global__ __launch_bounds__(CONV_THREADS) void frames_convert_kernel(ConvBatch fb) {
    const ConvFrame& f = fb.f[blockIdx.y];
    const unsigned per_row = (unsigned)(f.w + CONV_PX - 1) / CONV_PX, pairs = (unsigned)(f.h + CONV_ROWS - 1) / CONV_ROWS;
    const unsigned t = blockIdx.x * CONV_THREADS + threadIdx.x;          // < 2^24 + 256
    if (t >= per_row * pairs) return;                                     // (a frame smaller than the chunk's largest, and the last block)
    const unsigned rp = t / per_row;
    const int x0 = (int)(t - rp * per_row) * CONV_PX, y0 = (int)rp * CONV_ROWS;
    switch (f.format) {                                                   // uniform over the workgroup
        case RTM3D_PIX_RGB24: convert_run<RTM3D_PIX_RGB24>(f, x0, y0); break;
        case RTM3D_PIX_BGR24: convert_run<RTM3D_PIX_BGR24>(f, x0, y0); break;
        case RTM3D_PIX_RGBA32: convert_run<RTM3D_PIX_RGBA32>(f, x0, y0); break;
        case RTM3D_PIX_BGRA32: convert_run<RTM3D_PIX_BGRA32>(f, x0, y0); break;
        case RTM3D_PIX_GRAY8: convert_run<RTM3D_PIX_GRAY8>(f, x0, y0); break;
        case RTM3D_PIX_NV12: convert_run<RTM3D_PIX_NV12>(f, x0, y0); break;
        case RTM3D_PIX_NV21: convert_run<RTM3D_PIX_NV21>(f, x0, y0); break;
        case RTM3D_PIX_I420: convert_run<RTM3D_PIX_I420>(f, x0, y0); break;
        case RTM3D_PIX_YUYV: convert_run<RTM3D_PIX_YUYV>(f, x0, y0); break;
        case RTM3D_PIX_UYVY: convert_run<RTM3D_PIX_UYVY>(f, x0, y0); break;
        case RTM3D_PIX_P010: convert_run<RTM3D_PIX_P010>(f, x0, y0); break;
        default: break;
    }
}

// planes, bytes of a row and rows per plane; 1 for an unknown format
static int src_layout(int format, int h, int w, int* n_planes, int row_bytes[3], int rows[3]) {
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    int np = 1;
    row_bytes[0] = row_bytes[1] = row_bytes[2] = 0;
    rows[0] = h; rows[1] = rows[2] = 0;
    switch (format) {
        case RTM3D_PIX_RGB24: case RTM3D_PIX_BGR24: row_bytes[0] = 3 * w; break;
        case RTM3D_PIX_RGBA32: case RTM3D_PIX_BGRA32: row_bytes[0] = 4 * w; break;
        case RTM3D_PIX_GRAY8: row_bytes[0] = w; break;
        case RTM3D_PIX_NV12: case RTM3D_PIX_NV21: np = 2; row_bytes[0] = w; row_bytes[1] = 2 * cw; rows[1] = ch; break;
        case RTM3D_PIX_I420: np = 3; row_bytes[0] = w; row_bytes[1] = row_bytes[2] = cw; rows[1] = rows[2] = ch; break;
        case RTM3D_PIX_YUYV: case RTM3D_PIX_UYVY: row_bytes[0] = 4 * cw; break;
        case RTM3D_PIX_P010: np = 2; row_bytes[0] = 2 * w; row_bytes[1] = 4 * cw; rows[1] = ch; break;
        default: return 1;
    }
    *n_planes = np;
    return 0;
}

extern "C" int rtm3d_frame_src_layout(int format, int h, int w, int* n_planes, int min_pitch[3], int rows[3]) {
    if (!n_planes || !min_pitch || !rows) { rt_set_error("frame_src_layout: null pointer"); return 1; }
    if (h < 1 || w < 1 || h > CONV_MAX_SIDE || w > CONV_MAX_SIDE) {
        rt_set_error("frame_src_layout: a frame of %d x %d; a side must lie in 1..%d", h, w, CONV_MAX_SIDE); return 1;
    }
    if (src_layout(format, h, w, n_planes, min_pitch, rows)) { rt_set_error("frame_src_layout: unknown format %d", format); return 1; }
    return 0;
}

static bool is_yuv(int format) { return format >= RTM3D_PIX_NV12 && format <= RTM3D_PIX_P010; }

// row of the coefficient table, -1 for an unknown matrix or range
static int table_row(int format, int matrix, int range) {
    if ((matrix != RTM3D_YUV_BT601 && matrix != RTM3D_YUV_BT709) || (range != RTM3D_YUV_LIMITED && range != RTM3D_YUV_FULL)) return -1;
    if (range == RTM3D_YUV_LIMITED) return matrix;
    return (format == RTM3D_PIX_P010 ? 4 : 2) + matrix;
}

extern "C" int rtm3d_yuv_coefficients(int format, int matrix, int range, int out[8]) {
    if (!out) { rt_set_error("yuv_coefficients: null pointer"); return 1; }
    const int row = table_row(format, matrix, range);
    if (!is_yuv(format) || row < 0) { rt_set_error("yuv_coefficients: format %d, matrix %d, range %d", format, matrix, range); return 1; }
    const bool p10 = format == RTM3D_PIX_P010;
    for (int i = 0; i < 5; ++i) out[i] = h_conv_tab[row][i];
    out[5] = range == RTM3D_YUV_LIMITED ? (p10 ? 64 : 16) : 0;
    out[6] = p10 ? 512 : 128;
    out[7] = p10 ? 18 : 16;
    return 0;
}

// every refusal of the header, for the whole batch; h_dst may be NULL (the plan has no destinations)
static int check_sources(const char* who, int B, const rtm3d_frame_src* h_src, uint8_t* const* h_dst, int dst_order) {
    if (refuse_count(who, B) || refuse_null(who, h_src) || refuse_order(who, "dst_order", dst_order)) return 1;
    for (int b = 0; b < B; ++b) {
        const rtm3d_frame_src& s = h_src[b];
        if (refuse_side(who, b, s.h, s.w, 1, CONV_MAX_SIDE)) return 1;
        int np, row_bytes[3], rows[3];
        if (src_layout(s.format, s.h, s.w, &np, row_bytes, rows)) { rt_set_error("%s: frame %d has the unknown format %d", who, b, s.format); return 1; }
        if (refuse_reserved(who, b, s.reserved)) return 1;
        if (is_yuv(s.format) && table_row(s.format, s.matrix, s.range) < 0) {
            rt_set_error("%s: frame %d: unknown matrix %d or range %d", who, b, s.matrix, s.range); return 1;
        }
        for (int p = 0; p < np; ++p) {
            if (!s.plane[p]) { rt_set_error("%s: frame %d: plane %d is a NULL pointer", who, b, p); return 1; }
            if (s.pitch[p] < row_bytes[p]) {
                rt_set_error("%s: frame %d: pitch %d of plane %d is below the row's %d bytes", who, b, s.pitch[p], p, row_bytes[p]); return 1;
            }
            if (s.format == RTM3D_PIX_P010 && ((((uintptr_t)s.plane[p]) | (unsigned)s.pitch[p]) & 1)) {
                rt_set_error("%s: frame %d: plane %d of a P010 surface has an odd address or pitch", who, b, p); return 1;
            }
        }
        if (h_dst && refuse_null_dst(who, b, h_dst[b])) return 1;
    }
    return 0;
}

static rtm3d_convert_plan plan_chunk(const FrameChunk c, const rtm3d_frame_src* h_src) {
    rtm3d_convert_plan P;
    P.first = c.b0; P.count = c.nb;
    P.px_per_thread = CONV_PX; P.rows_per_thread = CONV_ROWS; P.threads = CONV_THREADS;
    P.runs = 0;
    for (int i = 0; i < c.nb; ++i) {
        const rtm3d_frame_src& s = h_src[c.b0 + i];
        const int runs = ((s.w + CONV_PX - 1) / CONV_PX) * ((s.h + CONV_ROWS - 1) / CONV_ROWS);         // <= 2048 * 8192
        if (runs > P.runs) P.runs = runs;
    }
    P.grid_x = (P.runs + CONV_THREADS - 1) / CONV_THREADS;
    P.grid_y = c.nb;
    return P;
}

extern "C" int rtm3d_frames_convert_plan(int B, const rtm3d_frame_src* h_src, rtm3d_convert_plan* out) {
    if (refuse_null("frames_convert_plan", out) || check_sources("frames_convert_plan", B, h_src, nullptr, 0)) return 1;
    for (const FrameChunk c : frame_chunks(B)) out[c.k] = plan_chunk(c, h_src);
    return 0;
}

extern "C" int rtm3d_frames_convert_check(int B, const rtm3d_frame_src* h_src, uint8_t* const* h_dst, int dst_order) {
    if (refuse_null("frames_convert", h_dst)) return 1;
    return check_sources("frames_convert", B, h_src, h_dst, dst_order);
}

extern "C" int rtm3d_frames_convert(void* stream, int B, const rtm3d_frame_src* h_src, uint8_t* const* h_dst, int dst_order) {
    if (rtm3d_frames_convert_check(B, h_src, h_dst, dst_order)) return 1;       // the whole batch, before the first launch
    for (const FrameChunk c : frame_chunks(B)) {
        const rtm3d_convert_plan plan = plan_chunk(c, h_src);                   // the numbers of rtm3d_frames_convert_plan
        ConvBatch fb;
        for (int i = 0; i < FRAME_CHUNK; ++i) {
            ConvFrame& f = fb.f[i];
            if (i >= c.nb) { f = ConvFrame{{nullptr, nullptr, nullptr}, nullptr, {0, 0, 0}, 0, 0, -1, 0, 0}; continue; }
            const rtm3d_frame_src& s = h_src[c.b0 + i];
            for (int p = 0; p < 3; ++p) { f.p[p] = (const uint8_t*)s.plane[p]; f.pitch[p] = s.pitch[p]; }
            f.dst = h_dst[c.b0 + i];
            f.h = s.h; f.w = s.w; f.format = s.format;
            const bool yuv = is_yuv(s.format);
            f.table = yuv ? table_row(s.format, s.matrix, s.range) : 0;
            const int yo = yuv && s.range == RTM3D_YUV_LIMITED ? (s.format == RTM3D_PIX_P010 ? 64 : 16) : 0;
            const bool src_bgr = s.format == RTM3D_PIX_BGR24 || s.format == RTM3D_PIX_BGRA32;
            f.yo_swap = yo | ((src_bgr != (dst_order == 1)) ? 1 << 16 : 0);
        }
        hipLaunchKernelGGL(frames_convert_kernel, dim3((unsigned)plan.grid_x, (unsigned)plan.grid_y), dim3(CONV_THREADS), 0,
                           (hipStream_t)stream, fb);
    }
    return launch_ok("frames_convert");
}
