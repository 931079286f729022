// Measurement only (not part of the library): the OTHER launch shape of the JPEG device stage (csrc/jpeg.hip recomputes the halo
// chroma blocks of a tile inside one launch).  Here launch A runs the inverse DCT of every block ONCE into sample planes in a
// caller's workspace, and launch B stages a tile of those planes, chroma halo included, in LDS and writes the pixels with the
// library's own pixel_run.  Built as a library of its own from the library's source; tools/jpeg_two_launch.py builds it, checks
// that both shapes write the same bytes and times them (profiles/jpeg.txt).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -o tools/microbench/jpeg_two_launch.out tools/microbench/jpeg_two_launch.hip
#include "../../rtm3d_amd/csrc/jpeg.hip"

#include <stdarg.h>
void rt_set_error(const char* fmt, ...) { (void)fmt; }
int rt_jpeg_info(const uint8_t*, size_t, rtm3d_jpeg_stream_info*, char*, size_t) { return 1; }
int rt_jpeg_entropy_decode(const uint8_t*, size_t, int16_t*, size_t, char*, size_t) { return 1; }

struct TwoFrame { const int16_t* coef; uint8_t* dst; uint8_t* ws; int h, w, mode, pad; };
struct TwoBatch { TwoFrame f[FRAME_CHUNK]; };

struct Geo { int hx, vy, mcus_x, mcus_y, ybw, ybh, cw, ch; size_t ny, nc; };
__device__ __forceinline__ Geo geo_of(int h, int w, int mode) {
    Geo g;
    g.hx = (mode == RTM3D_JPEG_422 || mode == RTM3D_JPEG_420) ? 2 : 1; g.vy = mode == RTM3D_JPEG_420 ? 2 : 1;
    g.mcus_x = (w + 8 * g.hx - 1) / (8 * g.hx); g.mcus_y = (h + 8 * g.vy - 1) / (8 * g.vy);
    g.ybw = g.mcus_x * g.hx; g.ybh = g.mcus_y * g.vy;
    g.cw = (w + g.hx - 1) / g.hx; g.ch = (h + g.vy - 1) / g.vy;
    g.ny = (size_t)g.ybw * g.ybh; g.nc = (size_t)g.mcus_x * g.mcus_y;
    return g;
}

__global__ __launch_bounds__(JPG_THREADS) void planes_kernel(TwoBatch fb) {
    const TwoFrame& f = fb.f[blockIdx.y];
    if (f.w == 0) return;
    const Geo g = geo_of(f.h, f.w, f.mode);
    const size_t total = g.ny + (f.mode == RTM3D_JPEG_GREY ? 0 : 2 * g.nc);
    const size_t t = (size_t)blockIdx.x * JPG_THREADS + threadIdx.x;
    if (t >= total) return;
    int comp = 0; size_t k = t;
    if (k >= g.ny) { k -= g.ny; comp = 1 + (k >= g.nc); k -= (size_t)(comp - 1) * g.nc; }
    const int bw = comp ? g.mcus_x : g.ybw;
    const int by = (int)(k / bw), bx = (int)(k - (size_t)by * bw);
    const int rw = comp ? g.cw : f.w, rh = comp ? g.ch : f.h;
    if (bx * 8 >= rw || by * 8 >= rh) return;
    const size_t plane = comp == 0 ? 0 : (g.ny + (comp - 1) * g.nc) * 64;                // samples: one byte each
    idct_block(f.coef + 192 + plane + k * 64, (const uint16_t*)f.coef + 64 * comp, f.ws + plane + (size_t)by * 8 * (bw * 8) + bx * 8, bw * 8);
}

__global__ __launch_bounds__(JPG_THREADS) void pixels_kernel(TwoBatch fb, int dst_order) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_y[JPG_TW * JPG_TH];
    __shared__ __attribute__((aligned(16))) uint8_t lds_c[2][JPG_CMAX];
    const TwoFrame& f = fb.f[blockIdx.y];
    const int tiles_x = (f.w + JPG_TW - 1) / JPG_TW, tiles_y = (f.h + JPG_TH - 1) / JPG_TH;
    const int t = (int)blockIdx.x;
    if (t >= tiles_x * tiles_y) return;
    const int tyi = t / tiles_x;
    const int tx0 = (t - tyi * tiles_x) * JPG_TW, ty0 = tyi * JPG_TH;
    const int nw = min(JPG_TW, f.w - tx0), nh = min(JPG_TH, f.h - ty0);
    const Geo g = geo_of(f.h, f.w, f.mode);
    const int hbx = g.hx - 1, hby = g.vy - 1;
    const int cbw = JPG_YBW / g.hx + 2 * hbx, cbh = JPG_YBH / g.vy + 2 * hby;
    const int cs = cbw * 8;
    const int cx0 = (tx0 / (8 * g.hx) - hbx) * 8, cy0 = (ty0 / (8 * g.vy) - hby) * 8;
    // Y: 64 rows of 16 units of 8 bytes
    for (int u = (int)threadIdx.x; u < JPG_TH * (JPG_TW / 8); u += JPG_THREADS) {
        const int r = u / (JPG_TW / 8), c = (u - r * (JPG_TW / 8)) * 8;
        const int gy = ty0 + r, gx = tx0 + c;
        if (gy < g.ybh * 8 && gx < g.ybw * 8) *(uint2*)(lds_y + r * JPG_TW + c) = *(const uint2*)(f.ws + (size_t)gy * (g.ybw * 8) + gx);
    }
    if (f.mode != RTM3D_JPEG_GREY) {
        for (int u = (int)threadIdx.x; u < 2 * cbh * 8 * cbw; u += JPG_THREADS) {
            const int comp = u >= cbh * 8 * cbw, v = u - comp * cbh * 8 * cbw;
            const int r = v / cbw, c = (v - r * cbw) * 8;
            const int gy = cy0 + r, gx = cx0 + c;
            if (gy >= 0 && gx >= 0 && gy < g.mcus_y * 8 && gx < g.mcus_x * 8)
                *(uint2*)(lds_c[comp] + r * cs + c) = *(const uint2*)(f.ws + (g.ny + comp * g.nc) * 64 + (size_t)gy * (g.mcus_x * 8) + gx);
        }
    }
    __syncthreads();
    const int lx0 = ((int)threadIdx.x % (JPG_TW / JPG_PX)) * JPG_PX, ly0 = ((int)threadIdx.x / (JPG_TW / JPG_PX)) * JPG_ROWS;
    if (lx0 >= nw || ly0 >= nh) return;
    JpgFrame jf; jf.coef = f.coef; jf.dst = f.dst; jf.h = f.h; jf.w = f.w; jf.mode = f.mode; jf.pad = 0;
    switch (f.mode) {
        case RTM3D_JPEG_GREY: pixel_run<RTM3D_JPEG_GREY>(jf, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, g.cw, g.ch, dst_order); break;
        case RTM3D_JPEG_444: pixel_run<RTM3D_JPEG_444>(jf, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, g.cw, g.ch, dst_order); break;
        case RTM3D_JPEG_422: pixel_run<RTM3D_JPEG_422>(jf, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, g.cw, g.ch, dst_order); break;
        default: pixel_run<RTM3D_JPEG_420>(jf, tx0 + lx0, ty0 + ly0, lx0, ly0, lds_y, lds_c[0], lds_c[1], cx0, cy0, cs, g.cw, g.ch, dst_order); break;
    }
}

// B <= 32 frames of one chunk; h_ws[b]: DEVICE workspace of (coef_count - 192) bytes, 16-byte aligned
extern "C" int two_launch(void* stream, int B, const rtm3d_jpeg_frame* h_frames, uint8_t* const* h_dst, uint8_t* const* h_ws, int dst_order) {
    if (B < 1 || B > FRAME_CHUNK) return 1;
    TwoBatch fb;
    size_t max_blocks = 0;
    int max_tiles = 0;
    for (int i = 0; i < FRAME_CHUNK; ++i) {
        TwoFrame& f = fb.f[i];
        f = TwoFrame{};
        if (i >= B) continue;
        f.coef = h_frames[i].d_coef; f.dst = h_dst[i]; f.ws = h_ws[i]; f.h = h_frames[i].h; f.w = h_frames[i].w; f.mode = h_frames[i].mode;
        const int hx = (f.mode == RTM3D_JPEG_422 || f.mode == RTM3D_JPEG_420) ? 2 : 1, vy = f.mode == RTM3D_JPEG_420 ? 2 : 1;
        const size_t mx = (f.w + 8 * hx - 1) / (8 * hx), my = (f.h + 8 * vy - 1) / (8 * vy);
        const size_t blocks = mx * my * (hx * vy + (f.mode == RTM3D_JPEG_GREY ? 0 : 2));
        if (blocks > max_blocks) max_blocks = blocks;
        const int tiles = ((f.w + JPG_TW - 1) / JPG_TW) * ((f.h + JPG_TH - 1) / JPG_TH);
        if (tiles > max_tiles) max_tiles = tiles;
    }
    hipLaunchKernelGGL(planes_kernel, dim3((unsigned)((max_blocks + JPG_THREADS - 1) / JPG_THREADS), (unsigned)B), dim3(JPG_THREADS), 0, (hipStream_t)stream, fb);
    hipLaunchKernelGGL(pixels_kernel, dim3((unsigned)max_tiles, (unsigned)B), dim3(JPG_THREADS), 0, (hipStream_t)stream, fb, dst_order);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
