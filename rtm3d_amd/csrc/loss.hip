// Validation loss of the reference (models/rtm3d_loss.py:268-340 fed by datasets/dataset_reader.py:215-291) on the device
// (include/rtm3d_hip.h, "validation loss"):
//   rtm3d_loss_objects   one lane per object: the derived table (centre, projections, offsets, Gaussian radius, masks);
//   rtm3d_loss_eval      the fused target + focal reduction - the heat-map target is never written: a workgroup takes an image
//                        and a band of rows, keeps that image's objects in LDS and forms each cell's target as it reads the
//                        logit - then one wave that sums the partials in a fixed order, gathers the regression logits of the
//                        three L1 terms and writes the five losses and the counts;
//   rtm3d_loss_heatmap   the target map itself, from the same device function (inspection and tests).
// The table is fp64 in the operation order the header writes out, compiled with -ffp-contract=off (Makefile) so that numpy
// restates it bit for bit; the projection of the corners is box_project.h's, the one statement of the corner order the 3D decode
// fits against.  Element terms of the loss are fp32 as in the reference, every sum is fp64 and no result depends on the order in
// which lanes or workgroups retire: no atomics, no tickets, every workgroup owns one slot.
#include "common.h"
#include "../../include/rtm3d_hip.h"

#include "box_project.h"

#define LS_THREADS 256
#define LS_WAVES (LS_THREADS / 64)
#define LS_CHUNK 128           // objects of one image held in LDS at a time
#define LS_CELLS 4             // cells per lane and tile: one 16-byte load where the map allows it
#define LS_ROW RTM3D_LOSS_ROW
#define LS_TAB RTM3D_LOSS_TABLE
#define LS_MAX_WG 1024         // workgroups the bands of a batch aim at (4 per compute unit)

// table columns
enum { T_IMG = 0, T_CLS, T_MASK, T_NOISE, T_MASK3D, T_INSIDE, T_CX, T_CY, T_MX, T_MY, T_MOFF, T_R = 12, T_SIGMA, T_RADIUS, T_INV,
       T_V = 16, T_VPROJ = 32, T_VOFF = 48, T_VCOOR = 64, T_VMASK = 80 };

__global__ __launch_bounds__(64) void loss_objects_kernel(int N, int B, const double* __restrict__ obj, const double* __restrict__ Ks,
                                                          double ds, int H, int W, double* __restrict__ tab) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= N) return;
    const double* o = obj + (size_t)i * LS_ROW;
    double* t = tab + (size_t)i * LS_TAB;
    const int img = (int)o[0], cls = (int)o[1];
    const bool img_ok = img >= 0 && img < B;
    const bool mask = cls >= 0 && img_ok;
    const bool noise = o[2] != 0.0;
    const double x1 = o[3] / ds, y1 = o[4] / ds, x2 = o[5] / ds, y2 = o[6] / ds;
    const double cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;
    const double mx = trunc(cx), my = trunc(cy);
    t[T_IMG] = (double)img; t[T_CLS] = (double)cls; t[T_MASK] = mask ? 1.0 : 0.0; t[T_NOISE] = noise ? 1.0 : 0.0;
    t[T_INSIDE] = (mx >= 0.0 && mx < (double)W && my >= 0.0 && my < (double)H) ? 1.0 : 0.0;
    t[T_CX] = cx; t[T_CY] = cy; t[T_MX] = mx; t[T_MY] = my; t[T_MOFF] = cx - mx; t[T_MOFF + 1] = cy - my;

    // _compute_gaussian_radius (utils/data_utils.py:97-118), min_overlap = 0.7
    const double mo = 0.7;
    const double hh = ceil(y2 - y1), ww = ceil(x2 - x1);
    const double b1 = hh + ww;
    const double c1 = ww * hh * (1 - mo) / (1 + mo);
    const double r1 = (b1 + sqrt(b1 * b1 - 4.0 * c1)) / 2;
    const double b2 = 2 * (hh + ww);
    const double c2 = (1 - mo) * ww * hh;
    const double r2 = (b2 + sqrt(b2 * b2 - 16.0 * c2)) / 2;
    const double a3 = 4 * mo;
    const double b3 = -2 * mo * (hh + ww);
    const double c3 = (mo - 1) * ww * hh;
    const double r3 = (b3 + sqrt(b3 * b3 - (4 * a3) * c3)) / 2;
    double r = r1 < r2 ? r1 : r2;
    r = r < r3 ? r : r3;
    const double sigma = (2 * r + 1) / 6;
    t[T_R] = r; t[T_SIGMA] = sigma; t[T_RADIUS] = ceil(r); t[T_INV] = 1.0 / (2 * (sigma * sigma));

    // vertices: K's first two rows over DOWN_SAMPLE, the box centre at Y - h / 2, the host's sine and cosine of Ry snapped like
    // rotation_matrix (utils/model_utils.py:66-77)
    double k[9];
    const double* K = Ks + (size_t)(img_ok ? img : 0) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) k[e] = e < 6 ? K[e] / ds : K[e];
    double sn = o[14], cs = o[15];
    if (fabs(sn) < 1e-3) sn = 0.0;
    if (fabs(cs) < 1e-3) cs = 0.0;
    double xs[8];
    xs[0] = sn; xs[1] = cs; xs[2] = o[9]; xs[3] = o[7]; xs[4] = o[8];           // l, h, w from dimension = (h, w, l)
    xs[5] = o[10]; xs[6] = o[11] - o[7] / 2; xs[7] = o[12];
    const double dx = xs[2] / 2, dz = xs[4] / 2;
    bool front = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        double u, v;
        box_project_corner(xs, k, sn, cs, c, u, v);
        const double sx = (c & 4) ? -1.0 : 1.0, sz = (c & 1) ? -1.0 : 1.0;
        const double Z = (-sn * dx) * sx + (cs * dz) * sz + xs[7];                // the corner's depth, as box_project_corner forms it
        front = front && (Z > 0.0);
        const double pu = trunc(u), pv = trunc(v);
        t[T_V + 2 * c] = u; t[T_V + 2 * c + 1] = v;
        t[T_VPROJ + 2 * c] = pu; t[T_VPROJ + 2 * c + 1] = pv;
        t[T_VOFF + 2 * c] = u - pu; t[T_VOFF + 2 * c + 1] = v - pv;
        t[T_VCOOR + 2 * c] = u - cx; t[T_VCOOR + 2 * c + 1] = v - cy;
        t[T_VMASK + c] = (pu >= 0.0 && pu < (double)W && pv >= 0.0 && pv < (double)H) ? 1.0 : 0.0;
    }
    t[T_MASK3D] = o[16] < 0.0 ? (front ? 1.0 : 0.0) : (o[16] != 0.0 ? 1.0 : 0.0);
}

// what the heat-map kernels keep of an object: cf = class | noise << 16, or -1 when mask = 0
struct LsObj { int mx, my, R, cf; double inv; };

__device__ __forceinline__ LsObj ls_load_obj(const double* __restrict__ t) {
    LsObj o;
    const double lim = (double)(1 << 28);                                     // (the host admits far less; keeps x - mx an int)
    const double mx = t[T_MX], my = t[T_MY], R = t[T_RADIUS];
    o.mx = (int)(mx < -lim ? -lim : (mx > lim ? lim : mx)); o.my = (int)(my < -lim ? -lim : (my > lim ? lim : my));
    o.R = R >= 0.0 ? (int)(R > lim ? lim : R) : -1;                           // a NaN radius covers nothing
    o.cf = t[T_MASK] != 0.0 ? ((int)t[T_CLS] | (t[T_NOISE] != 0.0 ? 1 << 16 : 0)) : -1;
    o.inv = t[T_INV];
    return o;
}

// m = max(m, g of object o at cell (c, y, x)) when the object's square covers the cell; the one statement of the target
__device__ __forceinline__ double ls_cover(const LsObj& o, int c, int y, int x, double m) {
    const int dx = x - o.mx, dy = y - o.my;
    if ((o.cf & 0xffff) != c || o.cf < 0 || dx > o.R || dx < -o.R || dy > o.R || dy < -o.R) return m;
    double g;
    if (dx == 0 && dy == 0 && (o.cf >> 16)) g = 0.9999;
    else g = exp(-((double)dx * (double)dx + (double)dy * (double)dy) * o.inv);
    return g > m ? g : m;
}

__device__ __forceinline__ void ls_img_range(const int32_t* __restrict__ img_start, int b, int N, int& o0, int& n) {
    int s = img_start[b], e = img_start[b + 1];
    s = s < 0 ? 0 : (s > N ? N : s);
    e = e < s ? s : (e > N ? N : e);
    o0 = s; n = e - s;
}

__global__ __launch_bounds__(LS_THREADS) void loss_heatmap_kernel(int C, int H, int W, const int32_t* __restrict__ img_start,
                                                                  const double* __restrict__ tab, int N, float* __restrict__ hm) {
    const int b = blockIdx.y;
    const int per = C * H * W;
    const int idx = blockIdx.x * LS_THREADS + threadIdx.x;
    if (idx >= per) return;
    const int c = idx / (H * W), rem = idx - c * (H * W), y = rem / W, x = rem - y * W;
    int o0, n;
    ls_img_range(img_start, b, N, o0, n);
    double m = 0.0;
    for (int i = 0; i < n; ++i) m = ls_cover(ls_load_obj(tab + (size_t)(o0 + i) * LS_TAB), c, y, x, m);
    hm[(size_t)b * per + idx] = (float)m;
}

template <bool SQ> __device__ __forceinline__ float ls_pow(float v, float e, bool four) {
    if (SQ) { const float s = v * v; return four ? s * s : s; }
    return powf(v, e);
}

__device__ __forceinline__ float ls_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ double ls_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// SQ: alpha = 2, beta = 4 (squares); otherwise powf.  VEC: W % 4 == 0 and a 16-byte aligned map - a lane's four cells are one load.
template <bool SQ, bool VEC>
__global__ __launch_bounds__(LS_THREADS) void loss_focal_kernel(int C, int H, int W, int band_rows, const float* __restrict__ hm,
                                                                const int32_t* __restrict__ img_start, const double* __restrict__ tab,
                                                                int N, float alpha, float beta, double* __restrict__ slots) {
    __shared__ LsObj objs[LS_CHUNK];
    __shared__ double red[LS_WAVES][3];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * band_rows;
    const int rows = (y0 + band_rows <= H ? band_rows : H - y0);
    const int plane = rows * W, cells = C * plane;
    int o0, nobj;
    ls_img_range(img_start, b, N, o0, nobj);
    const bool single = nobj <= LS_CHUNK;
    if (single) {
        if (tid < nobj) objs[tid] = ls_load_obj(tab + (size_t)(o0 + tid) * LS_TAB);
        __syncthreads();
    }
    const float* img = hm + (size_t)b * C * H * W;
    double pos = 0.0, neg = 0.0;
    int npos = 0;
    for (int base = 0; base < cells; base += LS_THREADS * LS_CELLS) {
        int cc[LS_CELLS], yy[LS_CELLS], xx[LS_CELLS];
        float lg[LS_CELLS];
        double m[LS_CELLS];
        if (VEC) {
            const int idx = base + tid * LS_CELLS;                               // cells is a multiple of 4 here: all four or none
            const bool ok = idx < cells;
            const int c = ok ? idx / plane : 0, rem = ok ? idx - c * plane : 0, y = rem / W, x = rem - y * W;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) v = *reinterpret_cast<const float4*>(img + ((size_t)c * H + y0 + y) * W + x);
            lg[0] = v.x; lg[1] = v.y; lg[2] = v.z; lg[3] = v.w;
#pragma unroll
            for (int k = 0; k < LS_CELLS; ++k) { cc[k] = ok ? c : -2; yy[k] = y0 + y; xx[k] = x + k; }
        } else {
#pragma unroll
            for (int k = 0; k < LS_CELLS; ++k) {
                const int idx = base + k * LS_THREADS + tid;
                const bool ok = idx < cells;
                const int c = ok ? idx / plane : 0, rem = ok ? idx - c * plane : 0, y = rem / W, x = rem - y * W;
                lg[k] = ok ? img[((size_t)c * H + y0 + y) * W + x] : 0.f;
                cc[k] = ok ? c : -2; yy[k] = y0 + y; xx[k] = x;
            }
        }
#pragma unroll
        for (int k = 0; k < LS_CELLS; ++k) m[k] = 0.0;
        for (int ob = 0; ob < nobj; ob += LS_CHUNK) {
            const int cnt = nobj - ob < LS_CHUNK ? nobj - ob : LS_CHUNK;
            if (!single) {                                                       // (uniform over the workgroup)
                __syncthreads();
                if (tid < cnt) objs[tid] = ls_load_obj(tab + (size_t)(o0 + ob + tid) * LS_TAB);
                __syncthreads();
            }
            for (int i = 0; i < cnt; ++i) {
                const LsObj o = objs[i];
#pragma unroll
                for (int k = 0; k < LS_CELLS; ++k) m[k] = ls_cover(o, cc[k], yy[k], xx[k], m[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < LS_CELLS; ++k) {
            if (cc[k] < 0) continue;
            const float t = (float)m[k];
            float p = ls_sigmoid(lg[k]);
            p = p < 1e-4f ? 1e-4f : (p > 0.9999f ? 0.9999f : p);                 // a NaN stays a NaN, as in torch.clamp
            if (t == 1.0f) {
                pos += (double)(logf(p) * ls_pow<SQ>(1.0f - p, alpha, false));
                ++npos;
            } else {
                neg += (double)((logf(1.0f - p) * ls_pow<SQ>(p, alpha, false)) * ls_pow<SQ>(1.0f - t, beta, true));
            }
        }
    }
    pos = ls_wave_sum(pos); neg = ls_wave_sum(neg);
    const double np = ls_wave_sum((double)npos);
    if ((tid & 63) == 0) { red[tid >> 6][0] = pos; red[tid >> 6][1] = neg; red[tid >> 6][2] = np; }
    __syncthreads();
    if (tid == 0) {
        double s0 = red[0][0], s1 = red[0][1], s2 = red[0][2];
#pragma unroll
        for (int w = 1; w < LS_WAVES; ++w) { s0 += red[w][0]; s1 += red[w][1]; s2 += red[w][2]; }
        double* s = slots + ((size_t)b * gridDim.x + blockIdx.x) * 3;
        s[0] = s0; s[1] = s1; s[2] = s2;
    }
}

// One wave.  Lane l sums the slots l, l + 64, ... in index order, the lanes are folded by a fixed butterfly; the L1 terms
// alike over the objects.  A single wave hides no latency behind other waves, so every load of a step is issued before the first
// is used: four slots at a time, and per object first the whole table row, then all 34 regression logits - unconditionally, from
// cell 0 of image 0 where the object or the vertex takes no part - and only then the masked sums.
__global__ __launch_bounds__(64) void loss_finish_kernel(int B, int H, int W, int nslots, const double* __restrict__ slots,
                                                         const float* __restrict__ vc, const float* __restrict__ moff,
                                                         const float* __restrict__ voff, const double* __restrict__ tab, int N,
                                                         float w_mkf, float w_vfm, float w_moff, float w_voff,
                                                         float* __restrict__ out, int32_t* __restrict__ counts,
                                                         double* __restrict__ accum) {
    const int lane = threadIdx.x;
    double pos = 0.0, neg = 0.0, np = 0.0;
    int s = lane;
    for (; s + 192 < nslots; s += 256) {
        double a[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 3; ++e) a[u][e] = slots[3 * (size_t)(s + 64 * u) + e];
#pragma unroll
        for (int u = 0; u < 4; ++u) { pos += a[u][0]; neg += a[u][1]; np += a[u][2]; }
    }
    for (; s < nslots; s += 64) { pos += slots[3 * (size_t)s]; neg += slots[3 * (size_t)s + 1]; np += slots[3 * (size_t)s + 2]; }
    pos = ls_wave_sum(pos); neg = ls_wave_sum(neg); np = ls_wave_sum(np);

    const size_t hw = (size_t)H * W;
    double s_vc = 0.0, s_vo = 0.0, s_mo = 0.0, n_v = 0.0, n_m = 0.0, n_out = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double* t = tab + (size_t)i * LS_TAB;
        const double mask = t[T_MASK], noise = t[T_NOISE], m3 = t[T_MASK3D], mxd = t[T_MX], myd = t[T_MY], bd = t[T_IMG];
        double vproj[16], vmask[8];
        float t_mo[2], t_vo[16], t_vc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { vproj[k] = t[T_VPROJ + k]; t_vo[k] = (float)t[T_VOFF + k]; t_vc[k] = (float)t[T_VCOOR + k]; }
#pragma unroll
        for (int v = 0; v < 8; ++v) vmask[v] = t[T_VMASK + v];
        t_mo[0] = (float)t[T_MOFF]; t_mo[1] = (float)t[T_MOFF + 1];
        const bool sel = mask != 0.0 && noise == 0.0 && bd >= 0.0 && bd < (double)B;
        const bool use = sel && mxd >= 0.0 && mxd < (double)W && myd >= 0.0 && myd < (double)H;
        if (sel && !use) n_out += 1.0;
        const size_t b = use ? (size_t)bd : 0, cell = use ? (size_t)myd * W + (size_t)mxd : 0;
        float g_mo[2], g_vc[16], g_vo[16];
        bool ok[8];
        g_mo[0] = moff[(b * 2) * hw + cell]; g_mo[1] = moff[(b * 2 + 1) * hw + cell];
#pragma unroll
        for (int k = 0; k < 16; ++k) g_vc[k] = vc[(b * 16 + k) * hw + cell];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const double vx = vproj[2 * v], vy = vproj[2 * v + 1];
            ok[v] = use && m3 != 0.0 && vmask[v] != 0.0 && vx >= 0.0 && vx < (double)W && vy >= 0.0 && vy < (double)H;
            const size_t vcell = ok[v] ? (size_t)vy * W + (size_t)vx : 0;
            g_vo[2 * v] = voff[(b * 2) * hw + vcell]; g_vo[2 * v + 1] = voff[(b * 2 + 1) * hw + vcell];
        }
        if (use) {
            s_mo += (double)fabsf(ls_sigmoid(g_mo[0]) - t_mo[0]);
            s_mo += (double)fabsf(ls_sigmoid(g_mo[1]) - t_mo[1]);
            n_m += 1.0;
        }
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (!ok[v]) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                s_vc += (double)fabsf(g_vc[2 * v + j] - t_vc[2 * v + j]);
                s_vo += (double)fabsf(ls_sigmoid(g_vo[2 * v + j]) - t_vo[2 * v + j]);
            }
            n_v += 1.0;
        }
    }
    s_vc = ls_wave_sum(s_vc); s_vo = ls_wave_sum(s_vo); s_mo = ls_wave_sum(s_mo);
    n_v = ls_wave_sum(n_v); n_m = ls_wave_sum(n_m); n_out = ls_wave_sum(n_out);
    if (lane != 0) return;
    const double main = np == 0.0 ? -neg : -(pos + neg) / np;
    const float l_main = (float)main * w_mkf;
    const float l_vc = (float)(s_vc / (2 * n_v)) * w_vfm;                         // 0 / 0: the NaN of F.l1_loss on nothing
    const float l_mo = (float)(s_mo / (2 * n_m)) * w_moff;
    const float l_vo = (float)(s_vo / (2 * n_v)) * w_voff;
    const float total = ((l_main + l_vc) + l_mo) + l_vo;
    out[0] = l_main; out[1] = l_vc; out[2] = l_mo; out[3] = l_vo; out[4] = total;
    counts[0] = (int32_t)np; counts[1] = (int32_t)n_v; counts[2] = (int32_t)n_v; counts[3] = (int32_t)n_m; counts[4] = (int32_t)n_out;
    if (accum) { accum[0] += (double)total * (double)B; accum[1] += (double)B; }
}

extern void rt_set_error(const char* fmt, ...);

static int ls_band_rows(int B, int H) {
    int bands = LS_MAX_WG / B;
    bands = bands < 1 ? 1 : (bands > H ? H : bands);
    return (H + bands - 1) / bands;
}

static int ls_sizes_ok(const char* what, int B, int C, int H, int W, int N) {
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || H <= 0 || W <= 0 || N < 0 || N > RTM3D_LOSS_MAX_OBJECTS) {
        rt_set_error("%s: bad sizes (B %d, C %d, H %d, W %d, N %d)", what, B, C, H, W, N);
        return 0;
    }
    if ((long long)C * H * W > 0x7fffffffLL / 2) { rt_set_error("%s: a map of %d x %d x %d cells is more than an int index holds", what, C, H, W); return 0; }
    return 1;
}

static int ls_launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("%s launch: %s", what, hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int rtm3d_loss_objects(void* stream, int N, int B, const double* d_obj, const double* d_K, double down_sample, int H, int W,
                                  double* d_table) {
    if (!ls_sizes_ok("loss_objects", B, 1, H, W, N)) return 1;
    if (!(down_sample > 0.0) || down_sample > 1e6) { rt_set_error("loss_objects: down_sample %g", down_sample); return 1; }
    if (N == 0) return 0;
    if (!d_obj || !d_K || !d_table) { rt_set_error("loss_objects: null pointer"); return 1; }
    hipLaunchKernelGGL(loss_objects_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, N, B, d_obj, d_K, down_sample, H, W,
                       d_table);
    return ls_launched("loss_objects");
}

extern "C" int rtm3d_loss_heatmap(void* stream, int B, int C, int H, int W, const int32_t* d_img_start, const double* d_table, int N,
                                  float* d_hm) {
    if (!ls_sizes_ok("loss_heatmap", B, C, H, W, N)) return 1;
    if (!d_img_start || !d_hm || (N > 0 && !d_table)) { rt_set_error("loss_heatmap: null pointer"); return 1; }
    const int per = C * H * W;
    hipLaunchKernelGGL(loss_heatmap_kernel, dim3((per + LS_THREADS - 1) / LS_THREADS, B), dim3(LS_THREADS), 0, (hipStream_t)stream, C, H, W,
                       d_img_start, d_table, N, d_hm);
    return ls_launched("loss_heatmap");
}

extern "C" size_t rtm3d_loss_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0) return 0;
    const int rb = ls_band_rows(B, H);
    return (size_t)B * ((H + rb - 1) / rb) * 3 * sizeof(double);
}

extern "C" int rtm3d_loss_eval(void* stream, int B, int C, int H, int W, const float* d_hm, const float* d_ver_coor, const float* d_m_off,
                               const float* d_v_off, const int32_t* d_img_start, const double* d_table, int N,
                               const rtm3d_loss_params* params, void* d_ws, float* d_out, int32_t* d_counts, double* d_accum) {
    if (!ls_sizes_ok("loss_eval", B, C, H, W, N)) return 1;
    if (!d_hm || !d_ver_coor || !d_m_off || !d_v_off || !d_img_start || !params || !d_ws || !d_out || !d_counts || (N > 0 && !d_table)) {
        rt_set_error("loss_eval: null pointer");
        return 1;
    }
    const float alpha = params->alpha, beta = params->beta;
    if (!(alpha > 0.f) || !(beta > 0.f) || alpha > 64.f || beta > 64.f) { rt_set_error("loss_eval: focal alpha %g / beta %g", alpha, beta); return 1; }
    for (int k = 0; k < 4; ++k)
        if (params->weight[k] != params->weight[k]) { rt_set_error("loss_eval: weight %d is NaN", k); return 1; }
    const int rb = ls_band_rows(B, H), bands = (H + rb - 1) / rb;
    const bool sq = alpha == 2.f && beta == 4.f;
    const bool vec = (W % 4) == 0 && (reinterpret_cast<uintptr_t>(d_hm) % 16) == 0;
    const dim3 grid(bands, B), block(LS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    double* slots = (double*)d_ws;
#define LS_LAUNCH(SQ, VEC) hipLaunchKernelGGL((loss_focal_kernel<SQ, VEC>), grid, block, 0, s, C, H, W, rb, d_hm, d_img_start, d_table, N, \
                                              alpha, beta, slots)
    if (sq && vec) LS_LAUNCH(true, true);
    else if (sq) LS_LAUNCH(true, false);
    else if (vec) LS_LAUNCH(false, true);
    else LS_LAUNCH(false, false);
#undef LS_LAUNCH
    if (ls_launched("loss_eval (focal)")) return 1;
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, s, B, H, W, bands * B, slots, d_ver_coor, d_m_off, d_v_off, d_table, N,
                       params->weight[0], params->weight[1], params->weight[2], params->weight[3], d_out, d_counts, d_accum);
    return ls_launched("loss_eval (finish)");
}

extern "C" int rtm3d_loss_accum_reset(void* stream, double* d_accum) {
    if (!d_accum) { rt_set_error("loss_accum_reset: null pointer"); return 1; }
    hipError_t e = hipMemsetAsync(d_accum, 0, 2 * sizeof(double), (hipStream_t)stream);
    if (e != hipSuccess) { rt_set_error("loss_accum_reset: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int rtm3d_loss_accum_read(void* stream, const double* d_accum, double* h_sum_count) {
    if (!d_accum || !h_sum_count) { rt_set_error("loss_accum_read: null pointer"); return 1; }
    hipError_t e = hipMemcpyAsync(h_sum_count, d_accum, 2 * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { rt_set_error("loss_accum_read: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
