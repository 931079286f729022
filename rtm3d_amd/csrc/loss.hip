// Validation loss of the reference (models/rtm3d_loss.py:268-340 fed by datasets/dataset_reader.py:215-291) on the device
// (include/rtm3d_hip.h, "validation loss"):
//   rtm3d_loss_objects   one lane per object: the derived table (centre, projections, offsets, Gaussian radius, masks);
//   rtm3d_loss_eval      the fused target + focal reduction - the heat-map target is never written: a workgroup takes an image
//                        and a band of rows, keeps that image's objects in LDS and forms each cell's target as it reads the
//                        logit - then one wave that sums the partials in a fixed order, gathers the regression logits of the
//                        three L1 terms and writes the five losses and the counts;
//   rtm3d_loss_heatmap   the target map itself, from the same device function (inspection and tests);
//   rtm3d_loss_grad      the gradient of the total with respect to the four logit maps ("loss gradient"): a dense pass with the
//                        focal kernel's decomposition that turns each heat-map logit into its gradient and clears the regression
//                        maps, then a sparse pass that adds the L1 terms' contributions in a fixed order, one writer per element.
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

// ---- loss gradient (include/rtm3d_hip.h, "loss gradient") -------------------------------------------------------------------
#define LG_BATCH 64            // objects of one image the sparse pass resolves at a time
#define LG_VERTS (LG_BATCH * 8)

template <bool SQ> __device__ __forceinline__ float ls_pow1(float v, float e) { return SQ ? v : powf(v, e - 1.0f); }

// The sigmoid of the sparse pass, through fp64 and rounded to fp32 once: the contributions to one element differ in sign only,
// so whether a run of them cancels to exactly zero hangs on the last bit of s - this one is the same on every device and host.
__device__ __forceinline__ float ls_sigmoid_cr(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

// sign with sign(0) = +0; a NaN stays a NaN, so a NaN logit shows in its own element
__device__ __forceinline__ float ls_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : (d == d ? 0.f : d)); }

// +0.0f into rows y0 .. y0 + rows - 1 of the ch channels of image b: 16-byte stores where the map allows them
__device__ __forceinline__ void ls_zero_band(float* g, int ch, int b, int H, int W, int y0, int rows, bool vec, int tid) {
    const size_t hw = (size_t)H * W;
    float* base = g + ((size_t)b * ch * H + y0) * W;                            // channel c of the band: base + c * hw
    const int plane = rows * W;
    if (vec) {
        const int q = plane / 4, n = ch * q;                                     // W % 4 == 0: whole float4s
        for (int i = tid; i < n; i += LS_THREADS) {
            const int c = i / q, r = i - c * q;
            *reinterpret_cast<float4*>(base + c * hw + 4 * (size_t)r) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        const int n = ch * plane;
        for (int i = tid; i < n; i += LS_THREADS) {
            const int c = i / plane, r = i - c * plane;
            base[c * hw + r] = 0.f;
        }
    }
}

// The dense pass: loss_focal_kernel's decomposition (one workgroup per image and band of rows, the image's objects in LDS), but
// each cell's logit becomes its gradient instead of a term of a sum; the same workgroup clears its band of the regression maps.
// g_hm, g_vc, g_mo, g_vo: NULL = not wanted.  zvec: bit 0 / 1 / 2 = g_vc / g_mo / g_vo take 16-byte stores.
template <bool SQ, bool VEC>
__global__ __launch_bounds__(LS_THREADS) void loss_grad_dense_kernel(int C, int H, int W, int band_rows, const float* __restrict__ hm,
                                                                     const int32_t* __restrict__ img_start, const double* __restrict__ tab,
                                                                     int N, float alpha, float beta, float w_mkf,
                                                                     const int32_t* __restrict__ counts, const float* __restrict__ up,
                                                                     float* __restrict__ g_hm, float* g_vc, float* g_mo, float* g_vo, int zvec) {
    __shared__ LsObj objs[LS_CHUNK];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = blockIdx.x * band_rows;
    const int rows = (y0 + band_rows <= H ? band_rows : H - y0);
    if (g_vc) ls_zero_band(g_vc, 16, b, H, W, y0, rows, (zvec & 1) != 0, tid);
    if (g_mo) ls_zero_band(g_mo, 2, b, H, W, y0, rows, (zvec & 2) != 0, tid);
    if (g_vo) ls_zero_band(g_vo, 2, b, H, W, y0, rows, (zvec & 4) != 0, tid);
    if (!g_hm) return;                                                           // (uniform over the grid)
    const int plane = rows * W, cells = C * plane;
    int o0, nobj;
    ls_img_range(img_start, b, N, o0, nobj);
    const bool single = nobj <= LS_CHUNK;
    if (single) {
        if (tid < nobj) objs[tid] = ls_load_obj(tab + (size_t)(o0 + tid) * LS_TAB);
        __syncthreads();
    }
    const int np = counts[0];
    const float u = up ? up[0] : 1.0f;
    const float ks = -((u * w_mkf) / (float)(np > 1 ? np : 1));
    const float* img = hm + (size_t)b * C * H * W;
    float* gimg = g_hm + (size_t)b * C * H * W;
    for (int base = 0; base < cells; base += LS_THREADS * LS_CELLS) {
        int cc[LS_CELLS], yy[LS_CELLS], xx[LS_CELLS];
        float lg[LS_CELLS];
        double m[LS_CELLS];
        size_t at[VEC ? 1 : LS_CELLS];
        if (VEC) {
            const int idx = base + tid * LS_CELLS;                               // cells is a multiple of 4 here: all four or none
            const bool ok = idx < cells;
            const int c = ok ? idx / plane : 0, rem = ok ? idx - c * plane : 0, y = rem / W, x = rem - y * W;
            at[0] = ((size_t)c * H + y0 + y) * W + x;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) v = *reinterpret_cast<const float4*>(img + at[0]);
            lg[0] = v.x; lg[1] = v.y; lg[2] = v.z; lg[3] = v.w;
#pragma unroll
            for (int k = 0; k < LS_CELLS; ++k) { cc[k] = ok ? c : -2; yy[k] = y0 + y; xx[k] = x + k; }
        } else {
#pragma unroll
            for (int k = 0; k < LS_CELLS; ++k) {
                const int idx = base + k * LS_THREADS + tid;
                const bool ok = idx < cells;
                const int c = ok ? idx / plane : 0, rem = ok ? idx - c * plane : 0, y = rem / W, x = rem - y * W;
                at[k] = ((size_t)c * H + y0 + y) * W + x;
                lg[k] = ok ? img[at[k]] : 0.f;
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
        float g[LS_CELLS];
#pragma unroll
        for (int k = 0; k < LS_CELLS; ++k) {
            const float t = (float)m[k];
            const float s = ls_sigmoid(lg[k]);
            const float p = s < 1e-4f ? 1e-4f : (s > 0.9999f ? 0.9999f : s);     // a NaN stays a NaN
            const bool in = s >= 1e-4f && s <= 0.9999f;                          // (false for a NaN)
            const float q = 1.0f - p;
            float dp;
            if (t == 1.0f) dp = ls_pow<SQ>(q, alpha, false) / p - (alpha * ls_pow1<SQ>(q, alpha)) * logf(p);
            else dp = (-ls_pow<SQ>(p, alpha, false) / q + (alpha * ls_pow1<SQ>(p, alpha)) * logf(q)) * ls_pow<SQ>(1.0f - t, beta, true);
            g[k] = (ks * (in ? dp : 0.0f)) * (s * (1.0f - s));
        }
        if (VEC) {
            if (cc[0] >= 0) *reinterpret_cast<float4*>(gimg + at[0]) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
#pragma unroll
            for (int k = 0; k < LS_CELLS; ++k)
                if (cc[k] >= 0) gimg[at[k]] = g[k];
        }
    }
}

// The sparse pass, behind the dense one on the same stream: one workgroup per image walks that image's objects LG_BATCH at a
// time.  Every contribution of a batch - its element (a cell key) and its fp32 value - goes to LDS; a contribution no earlier one
// of the batch shares its element with owns the element: it reads the element, adds the batch's contributions to it in rising
// (object, vertex) order and writes it back.  One writer per element and batch, the batches one after the other behind a
// barrier: the sums are those of a serial walk, without atomics.  Elements of different images never meet.
__global__ __launch_bounds__(LS_THREADS) void loss_grad_sparse_kernel(int B, int H, int W, const float* __restrict__ vc,
                                                                      const float* __restrict__ moff, const float* __restrict__ voff,
                                                                      const int32_t* __restrict__ img_start, const double* __restrict__ tab,
                                                                      int N, float w_vfm, float w_moff, float w_voff,
                                                                      const int32_t* __restrict__ counts, const float* __restrict__ up,
                                                                      float* g_vc, float* g_mo, float* g_vo) {
    __shared__ int mkey[LG_BATCH];                                               // the object's m_proj cell, -1: takes no part
    __shared__ int vkey[LG_VERTS];                                               // the vertex's v_proj cell, -1: takes no part
    __shared__ float c_mo[LG_BATCH][2], c_vc[LG_VERTS][2], c_vo[LG_VERTS][2];
    const int tid = threadIdx.x, b = blockIdx.x;
    int o0, nobj;
    ls_img_range(img_start, b, N, o0, nobj);
    const float u = up ? up[0] : 1.0f;
    const float k_vc = (u * w_vfm) / (2.0f * (float)counts[1]);
    const float k_vo = (u * w_voff) / (2.0f * (float)counts[2]);
    const float k_mo = (u * w_moff) / (2.0f * (float)counts[3]);
    const size_t hw = (size_t)H * W;
    for (int ob = 0; ob < nobj; ob += LG_BATCH) {
        const int cnt = nobj - ob < LG_BATCH ? nobj - ob : LG_BATCH;
        if (ob) __syncthreads();                                                 // the last batch's elements are written, its LDS is read
        for (int c = tid; c < cnt * 8; c += LS_THREADS) {
            const int i = c >> 3, j = c & 7;
            const double* t = tab + (size_t)(o0 + ob + i) * LS_TAB;
            const double mxd = t[T_MX], myd = t[T_MY], vx = t[T_VPROJ + 2 * j], vy = t[T_VPROJ + 2 * j + 1];
            const bool sel = t[T_MASK] != 0.0 && t[T_NOISE] == 0.0 && t[T_IMG] == (double)b;
            const bool use = sel && mxd >= 0.0 && mxd < (double)W && myd >= 0.0 && myd < (double)H;
            const bool ok = use && t[T_MASK3D] != 0.0 && t[T_VMASK + j] != 0.0 && vx >= 0.0 && vx < (double)W && vy >= 0.0 && vy < (double)H;
            const int cell = use ? (int)myd * W + (int)mxd : 0, vcell = ok ? (int)vy * W + (int)vx : 0;
            if (j == 0) {
                mkey[i] = use ? cell : -1;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float s = ls_sigmoid_cr(moff[((size_t)b * 2 + e) * hw + cell]);
                    c_mo[i][e] = (ls_sign(s - (float)t[T_MOFF + e]) * (s * (1.0f - s))) * k_mo;
                }
            }
            vkey[c] = ok ? vcell : -1;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float x = vc[((size_t)b * 16 + 2 * j + e) * hw + cell];
                const float s = ls_sigmoid_cr(voff[((size_t)b * 2 + e) * hw + vcell]);
                c_vc[c][e] = ls_sign(x - (float)t[T_VCOOR + 2 * j + e]) * k_vc;
                c_vo[c][e] = (ls_sign(s - (float)t[T_VOFF + 2 * j + e]) * (s * (1.0f - s))) * k_vo;
            }
        }
        __syncthreads();
        if (g_mo && tid < cnt && mkey[tid] >= 0) {
            const int key = mkey[tid];
            bool own = true;
            for (int i = 0; i < tid; ++i) own = own && mkey[i] != key;
            if (own) {
                float* e0 = g_mo + ((size_t)b * 2) * hw + key;
                float a0 = e0[0], a1 = e0[hw];
                for (int i = tid; i < cnt; ++i)
                    if (mkey[i] == key) { a0 += c_mo[i][0]; a1 += c_mo[i][1]; }
                e0[0] = a0; e0[hw] = a1;
            }
        }
        for (int c = tid; c < cnt * 8; c += LS_THREADS) {
            if (vkey[c] < 0) continue;
            const int i0 = c >> 3, j = c & 7;
            if (g_vc) {                                                          // channels 2 j, 2 j + 1 at m_proj: the objects on one cell
                const int key = mkey[i0];
                bool own = true;
                for (int i = 0; i < i0; ++i) own = own && !(mkey[i] == key && vkey[i * 8 + j] >= 0);
                if (own) {
                    float* e0 = g_vc + ((size_t)b * 16 + 2 * j) * hw + key;
                    float a0 = e0[0], a1 = e0[hw];
                    for (int i = i0; i < cnt; ++i)
                        if (mkey[i] == key && vkey[i * 8 + j] >= 0) { a0 += c_vc[i * 8 + j][0]; a1 += c_vc[i * 8 + j][1]; }
                    e0[0] = a0; e0[hw] = a1;
                }
            }
            if (g_vo) {                                                          // channels 0, 1 at v_proj: any vertices on one cell
                const int key = vkey[c];
                bool own = true;
                for (int d = 0; d < c; ++d) own = own && vkey[d] != key;
                if (own) {
                    float* e0 = g_vo + ((size_t)b * 2) * hw + key;
                    float a0 = e0[0], a1 = e0[hw];
                    for (int d = c; d < cnt * 8; ++d)
                        if (vkey[d] == key) { a0 += c_vo[d][0]; a1 += c_vo[d][1]; }
                    e0[0] = a0; e0[hw] = a1;
                }
            }
        }
    }
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

extern "C" int rtm3d_loss_grad(void* stream, int B, int C, int H, int W, const float* d_hm, const float* d_ver_coor, const float* d_m_off,
                               const float* d_v_off, const int32_t* d_img_start, const double* d_table, int N,
                               const rtm3d_loss_params* params, const int32_t* d_counts, const float* d_upstream, float* d_g_hm,
                               float* d_g_ver_coor, float* d_g_m_off, float* d_g_v_off) {
    if (!ls_sizes_ok("loss_grad", B, C, H, W, N)) return 1;
    if ((long long)16 * H * W > 0x7fffffffLL / 2) { rt_set_error("loss_grad: a map of 16 x %d x %d cells is more than an int index holds", H, W); return 1; }
    if (!d_hm || !d_ver_coor || !d_m_off || !d_v_off || !d_img_start || !params || (N > 0 && !d_table)) {
        rt_set_error("loss_grad: null pointer");
        return 1;
    }
    if (!d_counts) { rt_set_error("loss_grad: null d_counts (rtm3d_loss_eval's counts of the same inputs)"); return 1; }
    const float alpha = params->alpha, beta = params->beta;
    if (!(alpha > 0.f) || !(beta > 0.f) || alpha > 64.f || beta > 64.f) { rt_set_error("loss_grad: focal alpha %g / beta %g", alpha, beta); return 1; }
    for (int k = 0; k < 4; ++k)
        if (params->weight[k] != params->weight[k]) { rt_set_error("loss_grad: weight %d is NaN", k); return 1; }
    const void* outs[4] = {d_g_hm, d_g_ver_coor, d_g_m_off, d_g_v_off};
    const void* ins[8] = {d_hm, d_ver_coor, d_m_off, d_v_off, d_img_start, d_table, d_counts, d_upstream};
    if (!d_g_hm && !d_g_ver_coor && !d_g_m_off && !d_g_v_off) { rt_set_error("loss_grad: no output wanted (all four are NULL)"); return 1; }
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i < 8; ++i)
            if (outs[o] && outs[o] == ins[i]) { rt_set_error("loss_grad: output %d is input %d (the gradient is not formed in place)", o, i); return 1; }
    const int rb = ls_band_rows(B, H), bands = (H + rb - 1) / rb;
    const bool sq = alpha == 2.f && beta == 4.f;
    auto al16 = [&](const void* p) { return (W % 4) == 0 && (reinterpret_cast<uintptr_t>(p) % 16) == 0; };
    const bool vec = al16(d_hm) && al16(d_g_hm);
    const int zvec = (al16(d_g_ver_coor) ? 1 : 0) | (al16(d_g_m_off) ? 2 : 0) | (al16(d_g_v_off) ? 4 : 0);
    const dim3 grid(bands, B), block(LS_THREADS);
    hipStream_t s = (hipStream_t)stream;
#define LG_LAUNCH(SQ, VEC) hipLaunchKernelGGL((loss_grad_dense_kernel<SQ, VEC>), grid, block, 0, s, C, H, W, rb, d_hm, d_img_start, d_table, N, \
                                              alpha, beta, params->weight[0], d_counts, d_upstream, d_g_hm, d_g_ver_coor, d_g_m_off, d_g_v_off, zvec)
    if (sq && vec) LG_LAUNCH(true, true);
    else if (sq) LG_LAUNCH(true, false);
    else if (vec) LG_LAUNCH(false, true);
    else LG_LAUNCH(false, false);
#undef LG_LAUNCH
    if (ls_launched("loss_grad (dense)")) return 1;
    if (N == 0 || (!d_g_ver_coor && !d_g_m_off && !d_g_v_off)) return 0;
    hipLaunchKernelGGL(loss_grad_sparse_kernel, dim3(B), block, 0, s, B, H, W, d_ver_coor, d_m_off, d_v_off, d_img_start, d_table, N,
                       params->weight[1], params->weight[2], params->weight[3], d_counts, d_upstream, d_g_ver_coor, d_g_m_off, d_g_v_off);
    return ls_launched("loss_grad (sparse)");
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
