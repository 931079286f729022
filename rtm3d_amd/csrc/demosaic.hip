// Raw sensor frames (include/rtm3d_hip.h, "raw sensor frames"): Bayer mosaics of 8 / 10 / 12 / 14 / 16-bit samples - bytes,
// uint16 (LSB- or MSB-justified), MIPI RAW10 / RAW12 - to the tightly packed uint8 (h, w, 3) frames every other entry point
// reads.  Black level, white balance, demosaic (Malvar-He-Cutler or bilinear), colour matrix and tone table in one launch per
// chunk of FRAME_CHUNK frames (frame_chunks.h); the per-frame descriptors travel by value (no copy, no memset, no synchronisation).
//
// Mapping (rtm3d_frames_demosaic_plan returns the same numbers): workgroup blockIdx.x of frame blockIdx.y takes the tile of
// DEM_TW x DEM_TH pixels at (DEM_TW * (t % tiles_x), DEM_TH * (t / tiles_x)).
//   1. Staging.  The tile and DEM_HALO samples around it go to LDS as uint16 AFTER black level and white balance, so every
//      sample is fetched, unpacked and balanced once per tile, not once per tap.  The work is cut into units of 8 samples at
//      x = 0 mod 8 of one row - 8 / 16 / 10 / 12 bytes, whole MIPI groups.  A unit inside [0, w) is read with 4-byte loads
//      when its first byte is so aligned, 2-byte loads when that is even, byte by byte otherwise; a unit that crosses a border
//      of the frame goes sample by sample through fold(), which is where the reflection happens: the stencil is border-free.
//      Rows are folded once per unit.  No read leaves rows x row bytes of the plane.
//   2. Stencil.  Thread (rx, ry) = (tid % 16, tid / 16) writes pixels 8 rx .. + 7 of rows 2 ry, + 1 of the tile.  Its first
//      pixel has even x and even y, so the CFA cell of each of its 16 pixels is a compile-time constant: BGGR and GBRG are
//      RGGB and GRBG with R and B exchanged (one wave-uniform select), and RGGB / GRBG differ in the parity of the green
//      cells (a template parameter, chosen by a wave-uniform branch).  No per-pixel branch depends on the pattern.  The
//      6 x 12 window of a thread is read from LDS with 8-byte loads (row stride 264 B, run offset 16 B).
//   3. Store.  The 24 output bytes of a row of a run leave through store_rgb_run<8> (rgb_runs.h): aligned dwords, shifted by
//      the destination's misalignment, a partial run (the row's last) byte by byte: exactly h * w * 3 bytes are written.
// A frame's tone table is staged in LDS next to the tile (16 bytes per thread) and read there: 48 single-byte lookups per thread.
// Integer code only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtm3d_hip.h"
#include "frame_chunks.h"
#include "rgb_runs.h"

#define DEM_TW 128
#define DEM_TH 32
#define DEM_HALO 2
#define DEM_PX 8
#define DEM_ROWS 2
#define DEM_THREADS 256
#define DEM_MAX_SIDE 16384
#define DEM_TONE 4096                                   // bytes of a tone table
#define DEM_LW (DEM_TW + 2 * DEM_HALO)                  // 132 samples of an LDS row: 264 B, a multiple of 8
#define DEM_LH (DEM_TH + 2 * DEM_HALO)
#define DEM_UNITS (DEM_TW / 8 + 2)                      // units of 8 samples that cover x = tile - 8 .. tile + DEM_TW + 7
static_assert(DEM_THREADS == (DEM_TW / DEM_PX) * (DEM_TH / DEM_ROWS), "one run of DEM_PX x DEM_ROWS pixels per thread");
static_assert(DEM_TONE == 16 * DEM_THREADS, "a thread stages 16 bytes of the tone table");
static_assert(DEM_TW % 8 == 0 && DEM_TH % 2 == 0 && DEM_HALO == 2 && (DEM_LW * 2) % 8 == 0, "cell parities and 8-byte LDS reads");

struct DemFrame {                        // 104 B
    const uint8_t* plane;
    const uint8_t* tone;                 // or NULL
    uint8_t* dst;
    int pitch, h, w;
    int layout, bits;
    int flags;                           // bit 0: exchange R and B behind the stencil (BGGR, GBRG); bit 1: green at cells 0 and 3 (GRBG, GBRG);
                                         // bit 2: the colour matrix is not the identity
    int black[4], gain[4];
    int16_t ccm[9], pad;
};
struct DemBatch { DemFrame f[FRAME_CHUNK]; };            // 3.25 KB of kernel arguments

// fold() of the header for i in [-2, n + 1], n >= 2 (all that a halo of 2 asks for): |i| is the reflection at 0, p - i the one
// at n - 1; the second |.| serves n = 2, where p - i can be -1
__device__ __forceinline__ int fold_near(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i < 0 ? -i : i;
}

// ---- N bytes (even) at p into dwords, by the widest loads the address allows
template <int N>
__device__ __forceinline__ void load_unit(const uint8_t* p, uint32_t (&v)[(N + 3) / 4]) {
    static_assert(N % 2 == 0, "units are whole 16-bit words");
    const uintptr_t a = (uintptr_t)p;
#pragma unroll
    for (int i = 0; i < (N + 3) / 4; ++i) v[i] = 0;
    if ((a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) v[i] = ((const uint32_t*)p)[i];
        if (N % 4) v[N / 4] = ((const uint16_t*)p)[N / 2 - 1];
    } else if ((a & 1) == 0) {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) v[i >> 1] |= (uint32_t)((const uint16_t*)p)[i] << (16 * (i & 1));
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
}
#define DEM_BYTE(v, k) (int)(((v)[(k) >> 2] >> (8 * ((k) & 3))) & 255u)
#define DEM_HALF(v, k) (int)(((v)[(k) >> 1] >> (16 * ((k) & 1))) & 65535u)

template <int LAYOUT> struct UnitBytes { static constexpr int value = LAYOUT == RTM3D_RAW_U8 ? 8 : LAYOUT == RTM3D_RAW_MIPI10 ? 10 : LAYOUT == RTM3D_RAW_MIPI12 ? 12 : 16; };

// sample j (a constant) of a unit of 8
template <int LAYOUT>
__device__ __forceinline__ int unit_sample(const uint32_t (&v)[(UnitBytes<LAYOUT>::value + 3) / 4], int j, int bits, int M) {
    if constexpr (LAYOUT == RTM3D_RAW_U8) return DEM_BYTE(v, j);
    else if constexpr (LAYOUT == RTM3D_RAW_U16) return min(DEM_HALF(v, j), M);
    else if constexpr (LAYOUT == RTM3D_RAW_U16_MSB) return DEM_HALF(v, j) >> (16 - bits);
    else if constexpr (LAYOUT == RTM3D_RAW_MIPI10) return (DEM_BYTE(v, 5 * (j >> 2) + (j & 3)) << 2) | ((DEM_BYTE(v, 5 * (j >> 2) + 4) >> (2 * (j & 3))) & 3);
    else return (DEM_BYTE(v, 3 * (j >> 1) + (j & 1)) << 4) | ((DEM_BYTE(v, 3 * (j >> 1) + 2) >> (4 * (j & 1))) & 15);
}

// sample x (any, inside the row) of a row, byte by byte
template <int LAYOUT>
__device__ __forceinline__ int row_sample(const uint8_t* row, int x, int bits, int M) {
    if constexpr (LAYOUT == RTM3D_RAW_U8) return row[x];
    else if constexpr (LAYOUT == RTM3D_RAW_U16) return min((int)((const uint16_t*)row)[x], M);
    else if constexpr (LAYOUT == RTM3D_RAW_U16_MSB) return (int)((const uint16_t*)row)[x] >> (16 - bits);
    else if constexpr (LAYOUT == RTM3D_RAW_MIPI10) {
        const uint8_t* g = row + 5 * (x >> 2);
        return ((int)g[x & 3] << 2) | (((int)g[4] >> (2 * (x & 3))) & 3);
    } else {
        const uint8_t* g = row + 3 * (x >> 1);
        return ((int)g[x & 1] << 4) | (((int)g[2] >> (4 * (x & 1))) & 15);
    }
}

// steps 1-2 of the rule
__device__ __forceinline__ int balance(int s, int black, int gain, int M) { return min((max(s - black, 0) * gain + 512) >> 10, M); }

// ---- the tile's samples, x = tx0 - 2 .. tx0 + nw + 1, y = ty0 - 2 .. ty0 + nh + 1, folded into the frame, to LDS
template <int LAYOUT>
__device__ __forceinline__ void stage_tile(const DemFrame& f, int tx0, int ty0, int nw, int nh, uint16_t (*lds)[DEM_LW]) {
    constexpr int NB = UnitBytes<LAYOUT>::value;
    const int M = (1 << f.bits) - 1;
    const int b0 = f.black[0], b1 = f.black[1], b2 = f.black[2], b3 = f.black[3];
    const int g0 = f.gain[0], g1 = f.gain[1], g2 = f.gain[2], g3 = f.gain[3];
    for (int task = (int)threadIdx.x; task < (nh + 2 * DEM_HALO) * DEM_UNITS; task += DEM_THREADS) {
        const int ly = task / DEM_UNITS, u = task - ly * DEM_UNITS;
        const int x8 = tx0 - 8 + 8 * u;                                    // the unit's first sample; lx = x - (tx0 - 2)
        if (x8 >= tx0 + nw + DEM_HALO) continue;                           // right of everything the tile's pixels read
        const int fy = fold_near(ty0 - DEM_HALO + ly, f.h);
        const uint8_t* row = f.plane + (size_t)fy * f.pitch;
        const bool odd_row = (fy & 1) != 0;
        const int be = odd_row ? b2 : b0, bo = odd_row ? b3 : b1, ge = odd_row ? g2 : g0, go = odd_row ? g3 : g1;   // even / odd x
        if (x8 >= 0 && x8 + 8 <= f.w) {
            uint32_t v[(NB + 3) / 4];
            load_unit<NB>(row + (size_t)(x8 >> 3) * NB, v);
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int lx = 8 * u - 6 + j;                              // even: the pair is one dword of the LDS row
                if ((unsigned)lx < (unsigned)DEM_LW) {
                    const uint32_t lo = (uint32_t)balance(unit_sample<LAYOUT>(v, j, f.bits, M), be, ge, M);
                    const uint32_t hi = (uint32_t)balance(unit_sample<LAYOUT>(v, j + 1, f.bits, M), bo, go, M);
                    *(uint32_t*)&lds[ly][lx] = lo | (hi << 16);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int lx = 8 * u - 6 + j;
                if (lx >= 0 && lx < nw + 2 * DEM_HALO) {                   // x in [-2, w + 1]
                    const int fx = fold_near(x8 + j, f.w);                 // keeps the parity of x
                    lds[ly][lx] = (uint16_t)balance(row_sample<LAYOUT>(row, fx, f.bits, M), (j & 1) ? bo : be, (j & 1) ? go : ge, M);
                }
            }
        }
    }
}

// ---- one thread's 8 x 2 pixels.  GF: green at the cells with (x ^ y) even (GRBG, GBRG) rather than odd (RGGB, BGGR)
template <int METHOD, int GF>
__device__ __forceinline__ void demosaic_run(const DemFrame& f, int x0, int y0, int lx0, int ly0, const uint16_t (*lds)[DEM_LW],
                                             const uint8_t* tone, int dst_order) {
    const int M = (1 << f.bits) - 1;
    const int n = min(DEM_PX, f.w - x0), nrows = min(DEM_ROWS, f.h - y0);
    const bool swap_rb = (f.flags & 1) != 0, use_ccm = (f.flags & 4) != 0;
    const int up = f.bits - 12;                                            // tone index: >> up, or << -up
    uint32_t win[DEM_ROWS + 4][6];                                         // rows y0 - 2 .. y0 + 3, samples x0 - 2 .. x0 + 9, two per dword
#pragma unroll
    for (int r = 0; r < DEM_ROWS + 4; ++r) {
        const uint2* p = (const uint2*)&lds[ly0 + r][lx0];                 // 264 * row + 16 * run bytes: 8-byte aligned
#pragma unroll
        for (int q = 0; q < 3; ++q) { const uint2 t = p[q]; win[r][2 * q] = t.x; win[r][2 * q + 1] = t.y; }
    }
#define DEM_M(r, c) DEM_HALF(win[r], c)
    int c9[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) c9[i] = f.ccm[i];
#pragma unroll
    for (int j = 0; j < DEM_ROWS; ++j) {
        if (j >= nrows) break;
        uint32_t px[DEM_PX];
#pragma unroll
        for (int i = 0; i < DEM_PX; ++i) {
            const int r = j + 2, c = i + 2;
            const int C = DEM_M(r, c);
            const int ax1 = DEM_M(r, c - 1) + DEM_M(r, c + 1), ay1 = DEM_M(r - 1, c) + DEM_M(r + 1, c);
            const int d = DEM_M(r - 1, c - 1) + DEM_M(r - 1, c + 1) + DEM_M(r + 1, c - 1) + DEM_M(r + 1, c + 1);
            int R, G, B;
            const bool green = (((i ^ j) & 1) != 0) != (GF != 0);          // a constant after unrolling
            if (green) {
                int H, V;
                if (METHOD == RTM3D_DEMOSAIC_MHC) {
                    const int ax2 = DEM_M(r, c - 2) + DEM_M(r, c + 2), ay2 = DEM_M(r - 2, c) + DEM_M(r + 2, c);
                    H = min(max((10 * C + 8 * ax1 - 2 * d - 2 * ax2 + ay2 + 8) >> 4, 0), M);
                    V = min(max((10 * C + 8 * ay1 - 2 * d - 2 * ay2 + ax2 + 8) >> 4, 0), M);
                } else {
                    H = (ax1 + 1) >> 1;
                    V = (ay1 + 1) >> 1;
                }
                G = C;
                R = (j & 1) ? V : H;                                       // RGGB / GRBG: the red cells lie on the even rows
                B = (j & 1) ? H : V;
            } else {
                int O;
                if (METHOD == RTM3D_DEMOSAIC_MHC) {
                    const int a2 = DEM_M(r, c - 2) + DEM_M(r, c + 2) + DEM_M(r - 2, c) + DEM_M(r + 2, c);
                    G = min(max((8 * C + 4 * (ax1 + ay1) - 2 * a2 + 8) >> 4, 0), M);
                    O = min(max((12 * C + 4 * d - 3 * a2 + 8) >> 4, 0), M);
                } else {
                    G = (ax1 + ay1 + 2) >> 2;
                    O = (d + 2) >> 2;
                }
                R = (j & 1) ? O : C;
                B = (j & 1) ? C : O;
            }
            if (swap_rb) { const int t = R; R = B; B = t; }
            if (use_ccm) {
                const int r2 = min(max((c9[0] * R + c9[1] * G + c9[2] * B + 512) >> 10, 0), M);
                const int g2 = min(max((c9[3] * R + c9[4] * G + c9[5] * B + 512) >> 10, 0), M);
                const int b2 = min(max((c9[6] * R + c9[7] * G + c9[8] * B + 512) >> 10, 0), M);
                R = r2; G = g2; B = b2;
            }
            R = up >= 0 ? R >> up : R << -up;
            G = up >= 0 ? G >> up : G << -up;
            B = up >= 0 ? B >> up : B << -up;
            if (f.tone) {
                R = tone[R & (DEM_TONE - 1)];                              // (the mask: a pixel past the row's end holds unstaged samples)
                G = tone[G & (DEM_TONE - 1)];
                B = tone[B & (DEM_TONE - 1)];
            } else {
                R >>= 4; G >>= 4; B >>= 4;
            }
            px[i] = dst_order ? (uint32_t)B | ((uint32_t)G << 8) | ((uint32_t)R << 16) : (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
            px[i] &= 0xffffffu;
        }
        store_rgb_run<DEM_PX>(f.dst + ((size_t)(y0 + j) * f.w + x0) * 3, px, n);
    }
#undef DEM_M
}

// (5 waves per SIMD: the MHC instance would otherwise take 101 VGPRs and lose a workgroup per CU for it; 96 fit without a spill)
template <int METHOD>
__global__ __launch_bounds__(DEM_THREADS, 5) void frames_demosaic_kernel(DemBatch fb, int dst_order) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[DEM_LH][DEM_LW];
    __shared__ __attribute__((aligned(16))) uint8_t tone[DEM_TONE];
    const DemFrame& f = fb.f[blockIdx.y];
    const int tiles_x = (f.w + DEM_TW - 1) / DEM_TW, tiles_y = (f.h + DEM_TH - 1) / DEM_TH;
    const int t = (int)blockIdx.x;
    if (t >= tiles_x * tiles_y) return;                                    // (a frame smaller than the chunk's largest): the whole workgroup
    const int tyi = t / tiles_x;
    const int tx0 = (t - tyi * tiles_x) * DEM_TW, ty0 = tyi * DEM_TH;
    const int nw = min(DEM_TW, f.w - tx0), nh = min(DEM_TH, f.h - ty0);    // the tile's own pixels
    switch (f.layout) {                                                    // uniform over the workgroup
        case RTM3D_RAW_U8: stage_tile<RTM3D_RAW_U8>(f, tx0, ty0, nw, nh, lds); break;
        case RTM3D_RAW_U16: stage_tile<RTM3D_RAW_U16>(f, tx0, ty0, nw, nh, lds); break;
        case RTM3D_RAW_U16_MSB: stage_tile<RTM3D_RAW_U16_MSB>(f, tx0, ty0, nw, nh, lds); break;
        case RTM3D_RAW_MIPI10: stage_tile<RTM3D_RAW_MIPI10>(f, tx0, ty0, nw, nh, lds); break;
        case RTM3D_RAW_MIPI12: stage_tile<RTM3D_RAW_MIPI12>(f, tx0, ty0, nw, nh, lds); break;
        default: break;
    }
    if (f.tone) {                                                          // 16 bytes per thread, as one load where the table is so aligned
        const uint8_t* src = f.tone + 16 * threadIdx.x;
        if (((uintptr_t)src & 15) == 0) {
            ((uint4*)tone)[threadIdx.x] = *(const uint4*)src;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) tone[16 * threadIdx.x + i] = src[i];
        }
    }
    __syncthreads();
    const int lx0 = ((int)threadIdx.x % (DEM_TW / DEM_PX)) * DEM_PX, ly0 = ((int)threadIdx.x / (DEM_TW / DEM_PX)) * DEM_ROWS;
    if (lx0 >= nw || ly0 >= nh) return;
    if (f.flags & 2) demosaic_run<METHOD, 1>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds, tone, dst_order);
    else demosaic_run<METHOD, 0>(f, tx0 + lx0, ty0 + ly0, lx0, ly0, lds, tone, dst_order);
}

// bytes of a row; 0 for an unknown layout or bits the layout does not take
static int raw_row_bytes(int layout, int bits, int w) {
    switch (layout) {
        case RTM3D_RAW_U8: return bits == 8 ? w : 0;
        case RTM3D_RAW_U16: case RTM3D_RAW_U16_MSB: return bits == 10 || bits == 12 || bits == 14 || bits == 16 ? 2 * w : 0;
        case RTM3D_RAW_MIPI10: return bits == 10 ? 5 * ((w + 3) / 4) : 0;
        case RTM3D_RAW_MIPI12: return bits == 12 ? 3 * ((w + 1) / 2) : 0;
        default: return 0;
    }
}
static bool known_layout(int layout) { return layout >= RTM3D_RAW_U8 && layout <= RTM3D_RAW_MIPI12; }

extern "C" int rtm3d_raw_src_layout(int layout, int bits, int h, int w, int* min_pitch, int* rows) {
    if (!min_pitch || !rows) { rt_set_error("raw_src_layout: null pointer"); return 1; }
    if (h < 2 || w < 2 || h > DEM_MAX_SIDE || w > DEM_MAX_SIDE) {
        rt_set_error("raw_src_layout: a frame of %d x %d; a side must lie in 2..%d", h, w, DEM_MAX_SIDE); return 1;
    }
    if (!known_layout(layout)) { rt_set_error("raw_src_layout: unknown layout %d", layout); return 1; }
    const int rb = raw_row_bytes(layout, bits, w);
    if (!rb) { rt_set_error("raw_src_layout: layout %d does not take %d bits", layout, bits); return 1; }
    *min_pitch = rb; *rows = h;
    return 0;
}

// every refusal of the header, for the whole batch; h_dst may be NULL (the plan has no destinations)
static int check_raw(const char* who, int B, const rtm3d_raw_src* h_src, uint8_t* const* h_dst, int method, int dst_order) {
    if (refuse_count(who, B) || refuse_null(who, h_src)) return 1;
    if (method != RTM3D_DEMOSAIC_MHC && method != RTM3D_DEMOSAIC_BILINEAR) { rt_set_error("%s: method %d (0 MHC, 1 bilinear)", who, method); return 1; }
    if (refuse_order(who, "dst_order", dst_order)) return 1;
    for (int b = 0; b < B; ++b) {
        const rtm3d_raw_src& s = h_src[b];
        if (refuse_side(who, b, s.h, s.w, 2, DEM_MAX_SIDE)) return 1;
        if (!known_layout(s.layout)) { rt_set_error("%s: frame %d has the unknown layout %d", who, b, s.layout); return 1; }
        const int rb = raw_row_bytes(s.layout, s.bits, s.w);
        if (!rb) { rt_set_error("%s: frame %d: layout %d does not take %d bits", who, b, s.layout, s.bits); return 1; }
        if (s.pattern < RTM3D_CFA_RGGB || s.pattern > RTM3D_CFA_GBRG) { rt_set_error("%s: frame %d has the unknown pattern %d", who, b, s.pattern); return 1; }
        if (refuse_reserved(who, b, s.reserved)) return 1;
        if (s.pad != 0) { rt_set_error("%s: frame %d: pad = %d, not 0", who, b, s.pad); return 1; }
        if (!s.plane) { rt_set_error("%s: frame %d: the plane is a NULL pointer", who, b); return 1; }
        if (s.pitch < rb) { rt_set_error("%s: frame %d: pitch %d is below the row's %d bytes", who, b, s.pitch, rb); return 1; }
        if ((s.layout == RTM3D_RAW_U16 || s.layout == RTM3D_RAW_U16_MSB) && ((((uintptr_t)s.plane) | (unsigned)s.pitch) & 1)) {
            rt_set_error("%s: frame %d: a uint16 plane has an odd address or pitch", who, b); return 1;
        }
        const int M = (1 << s.bits) - 1;
        for (int k = 0; k < 4; ++k) {
            if (s.black[k] > M) { rt_set_error("%s: frame %d: black[%d] = %d is above %d", who, b, k, s.black[k], M); return 1; }
            if (s.gain[k] > 16384) { rt_set_error("%s: frame %d: gain[%d] = %d is above 16384", who, b, k, s.gain[k]); return 1; }
        }
        for (int i = 0; i < 9; ++i)
            if (s.ccm[i] > 8192 || s.ccm[i] < -8192) { rt_set_error("%s: frame %d: ccm[%d] = %d is outside +-8192", who, b, i, s.ccm[i]); return 1; }
        if (h_dst && refuse_null_dst(who, b, h_dst[b])) return 1;
    }
    return 0;
}

static rtm3d_demosaic_plan plan_chunk(const FrameChunk c, const rtm3d_raw_src* h_src) {
    rtm3d_demosaic_plan P;
    P.first = c.b0; P.count = c.nb;
    P.tile_w = DEM_TW; P.tile_h = DEM_TH; P.halo = DEM_HALO; P.threads = DEM_THREADS;
    P.tiles = 0;
    for (int i = 0; i < c.nb; ++i) {
        const rtm3d_raw_src& s = h_src[c.b0 + i];
        const int tiles = ((s.w + DEM_TW - 1) / DEM_TW) * ((s.h + DEM_TH - 1) / DEM_TH);              // <= 128 * 512
        if (tiles > P.tiles) P.tiles = tiles;
    }
    P.grid_x = P.tiles;
    P.grid_y = c.nb;
    return P;
}

extern "C" int rtm3d_frames_demosaic_plan(int B, const rtm3d_raw_src* h_src, int method, rtm3d_demosaic_plan* out) {
    if (refuse_null("frames_demosaic_plan", out) || check_raw("frames_demosaic_plan", B, h_src, nullptr, method, 0)) return 1;
    for (const FrameChunk c : frame_chunks(B)) out[c.k] = plan_chunk(c, h_src);
    return 0;
}

extern "C" int rtm3d_frames_demosaic_check(int B, const rtm3d_raw_src* h_src, uint8_t* const* h_dst, int method, int dst_order) {
    if (refuse_null("frames_demosaic", h_dst)) return 1;
    return check_raw("frames_demosaic", B, h_src, h_dst, method, dst_order);
}

extern "C" int rtm3d_frames_demosaic(void* stream, int B, const rtm3d_raw_src* h_src, uint8_t* const* h_dst, int method, int dst_order) {
    if (rtm3d_frames_demosaic_check(B, h_src, h_dst, method, dst_order)) return 1;     // the whole batch, before the first launch
    for (const FrameChunk c : frame_chunks(B)) {
        const rtm3d_demosaic_plan plan = plan_chunk(c, h_src);                         // the numbers of rtm3d_frames_demosaic_plan
        DemBatch fb;
        for (int i = 0; i < FRAME_CHUNK; ++i) {
            DemFrame& f = fb.f[i];
            f = DemFrame{};                                                            // (h = w = 0: no tiles)
            if (i >= c.nb) continue;
            const rtm3d_raw_src& s = h_src[c.b0 + i];
            f.plane = (const uint8_t*)s.plane; f.tone = s.d_tone; f.dst = h_dst[c.b0 + i];
            f.pitch = s.pitch; f.h = s.h; f.w = s.w; f.layout = s.layout; f.bits = s.bits;
            bool identity = true;
            for (int k = 0; k < 9; ++k) { f.ccm[k] = s.ccm[k]; identity = identity && s.ccm[k] == (k % 4 == 0 ? 1024 : 0); }
            for (int k = 0; k < 4; ++k) { f.black[k] = s.black[k]; f.gain[k] = s.gain[k]; }
            f.flags = (s.pattern & 1) | (s.pattern & 2) | (identity ? 0 : 4);
        }
        const dim3 grid((unsigned)plan.grid_x, (unsigned)plan.grid_y), block(DEM_THREADS);
        if (method == RTM3D_DEMOSAIC_MHC)
            hipLaunchKernelGGL(frames_demosaic_kernel<RTM3D_DEMOSAIC_MHC>, grid, block, 0, (hipStream_t)stream, fb, dst_order);
        else
            hipLaunchKernelGGL(frames_demosaic_kernel<RTM3D_DEMOSAIC_BILINEAR>, grid, block, 0, (hipStream_t)stream, fb, dst_order);
    }
    return launch_ok("frames_demosaic");
}
