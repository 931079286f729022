// Overlaps of 3D boxes in the ground plane and 3D non-maximum suppression of detection records (include/rtm3d_hip.h,
// "box overlaps"):
//   rtm3d_box_overlaps     pairwise BEV and 3D overlap matrices of two ragged box lists per image, one lane per pair;
//   rtm3d_records_nms3d    greedy NMS over the kept (flag 2) slots of the detection records, in place, one workgroup per image.
// Box = (h, w, l, X, Y, Z, ry), record fields [24:31]: (X, Y, Z) is the box CENTRE in camera coordinates (y down).  The footprint
// lies in the x-z plane as in rtm3d_amd/kitti_results.py create_corners: half extents l/2 along local x and w/2 along local z,
// rotated by R = [[c,0,s],[0,1,0],[-s,0,c]] with PLAIN c = cos(ry), s = sin(ry).  There is NO snapping of small sines / cosines
// to zero here: that snap (rotation_matrix, |s|, |c| < 1e-3 -> 0) belongs to the reference's drawing code, not to the geometry
// of the box.  Vertical extent [Y - h/2, Y + h/2].
// One pair = box_prepare of either box + box_pair: rectangle A's corners are expressed in B's frame (world offsets from B's
// centre dotted with B's axes), clipped against B's four half-planes |x| <= l_b/2, |z| <= w_b/2 (Sutherland-Hodgman, closed
// inside tests `>= 0`, a new vertex gets the clipped coordinate EXACTLY), area by the shoelace sum.  All fp64, fixed operation
// order, compiled with -ffp-contract=off like frames.hip (Makefile).  A box with h, w or l <= 0 or any non-finite value
// overlaps nothing; no overlap is ever NaN.
// The polygon (at most 8 vertices, two buffers) lives in LDS, one 16-byte column per lane ([vertex][lane]: lanes of a wave hit
// consecutive banks whatever vertex each is at): its vertex count is data dependent, and a per-lane array indexed by it would
// be placed in private memory.
#include "common.h"
#include "../../include/rtm3d_hip.h"

#include "box_geom.h"

#define NMS_MAX_TOPK 256

__global__ __launch_bounds__(BO_LANES) void box_overlaps_kernel(long long total, int cap_a, int cap_b, const int32_t* __restrict__ na,
                                                               const int32_t* __restrict__ nb, const double* __restrict__ A,
                                                               const double* __restrict__ Bx, int criterion, double* __restrict__ bev,
                                                               double* __restrict__ vol) {
    __shared__ double2 poly[2][BO_MAXV][BO_LANES];
    const int lane = threadIdx.x;
    const long long t = (long long)blockIdx.x * BO_LANES + lane;
    if (t >= total) return;
    const long long per = (long long)cap_a * cap_b;
    const int img = (int)(t / per);
    const int r = (int)(t - img * per);
    const int i = r / cap_b, j = r - i * cap_b;
    double o_bev = 0.0, o_vol = 0.0;
    if (i < na[img] && j < nb[img]) {
        const BoxP a = box_load(A + ((size_t)img * cap_a + i) * 7);
        const BoxP b = box_load(Bx + ((size_t)img * cap_b + j) * 7);
        double inter, ov;
        box_pair(a, b, poly[0], poly[1], lane, inter, ov);
        o_bev = overlap_ratio(inter, a.area, b.area, criterion);
        o_vol = overlap_ratio(inter * ov, a.area * a.h, b.area * b.h, criterion);
    }
    if (bev) bev[t] = o_bev;
    if (vol) vol[t] = o_vol;
}

// One workgroup per image.  (1) the flag-2 slots are compacted in slot order (ballot prefix) and prepared into LDS; (2) every
// pair of candidates is visited once - round d = 1 .. nc / 2 pairs candidate i with (i + d) mod nc, the last round of an even
// nc only for i < nc / 2 - and a pair over the threshold sets bit `earlier` in the row of the later one; (3) wave 0 walks the
// candidates in order with the kept set in registers; (4) the suppressed slots are rewritten.
__global__ __launch_bounds__(BO_LANES) void records_nms3d_kernel(int topk, float* __restrict__ rec, double iou_thresh, int metric,
                                                                int class_aware, double* __restrict__ kitti) {
    __shared__ double2 poly[2][BO_MAXV][BO_LANES];
    __shared__ double g[10][NMS_MAX_TOPK];               // X, Z, c, s, hl, hw, y0, y1, area, h of candidate k
    __shared__ float g_cls[NMS_MAX_TOPK];
    __shared__ int g_valid[NMS_MAX_TOPK];
    __shared__ int g_slot[NMS_MAX_TOPK];
    __shared__ uint32_t over[NMS_MAX_TOPK][NMS_MAX_TOPK / 32];
    __shared__ uint32_t keepw[NMS_MAX_TOPK / 32];
    __shared__ int wave_n[BO_LANES / 64];
    const int tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
    float* r_img = rec + (size_t)blockIdx.x * topk * 32;

    const float* r = r_img + (size_t)tid * 32;
    const bool cand = tid < topk && r[31] == 2.0f;
    const unsigned long long bal = __ballot(cand);
    if (wl == 0) wave_n[wave] = __popcll(bal);
#pragma unroll
    for (int w = 0; w < NMS_MAX_TOPK / 32; ++w) over[tid][w] = 0u;
    __syncthreads();
    int base = 0, nc = 0;
#pragma unroll
    for (int w = 0; w < BO_LANES / 64; ++w) { if (w < wave) base += wave_n[w]; nc += wave_n[w]; }
    if (cand) {
        const int k = base + __popcll(bal & ((1ull << wl) - 1ull));
        const BoxP p = box_prepare((double)r[24], (double)r[25], (double)r[26], (double)r[27], (double)r[28], (double)r[29], (double)r[30]);
        g[0][k] = p.X; g[1][k] = p.Z; g[2][k] = p.c; g[3][k] = p.s; g[4][k] = p.hl; g[5][k] = p.hw;
        g[6][k] = p.y0; g[7][k] = p.y1; g[8][k] = p.area; g[9][k] = p.h;
        g_valid[k] = p.valid ? 1 : 0;
        g_cls[k] = r[0];
        g_slot[k] = tid;
    }
    __syncthreads();

    const int rounds = nc >> 1, npairs = rounds * nc;
    for (int p = tid; p < npairs; p += BO_LANES) {
        const int d = p / nc + 1, i = p - (d - 1) * nc;
        if ((nc & 1) == 0 && d == rounds && i >= rounds) continue;         // the half round of an even count
        int j = i + d;
        if (j >= nc) j -= nc;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        if (class_aware && g_cls[lo] != g_cls[hi]) continue;
        BoxP a, b;
        a.X = g[0][lo]; a.Z = g[1][lo]; a.c = g[2][lo]; a.s = g[3][lo]; a.hl = g[4][lo]; a.hw = g[5][lo];
        a.y0 = g[6][lo]; a.y1 = g[7][lo]; a.area = g[8][lo]; a.h = g[9][lo]; a.valid = g_valid[lo] != 0;
        b.X = g[0][hi]; b.Z = g[1][hi]; b.c = g[2][hi]; b.s = g[3][hi]; b.hl = g[4][hi]; b.hw = g[5][hi];
        b.y0 = g[6][hi]; b.y1 = g[7][hi]; b.area = g[8][hi]; b.h = g[9][hi]; b.valid = g_valid[hi] != 0;
        double inter, ov;
        box_pair(a, b, poly[0], poly[1], tid, inter, ov);
        const double iou = metric == 0 ? overlap_ratio(inter, a.area, b.area, 0)
                                       : overlap_ratio(inter * ov, a.area * a.h, b.area * b.h, 0);
        if (iou > iou_thresh) atomicOr(&over[hi][lo >> 5], 1u << (lo & 31));
    }
    __syncthreads();

    if (wave == 0) {                                    // every lane walks the same sequence: uniform LDS reads
        uint32_t keep[NMS_MAX_TOPK / 32];
#pragma unroll
        for (int w = 0; w < NMS_MAX_TOPK / 32; ++w) keep[w] = 0u;
        for (int k = 0; k < nc; ++k) {
            uint32_t hit = 0u;
#pragma unroll
            for (int w = 0; w < NMS_MAX_TOPK / 32; ++w) hit |= over[k][w] & keep[w];
            const uint32_t bit = hit ? 0u : 1u << (k & 31);
#pragma unroll
            for (int w = 0; w < NMS_MAX_TOPK / 32; ++w) keep[w] |= (w == (k >> 5)) ? bit : 0u;
        }
        if (wl < NMS_MAX_TOPK / 32) {
            uint32_t v = 0u;
#pragma unroll
            for (int w = 0; w < NMS_MAX_TOPK / 32; ++w) v = (w == wl) ? keep[w] : v;
            keepw[wl] = v;
        }
    }
    __syncthreads();

    if (tid < nc && !((keepw[tid >> 5] >> (tid & 31)) & 1u)) {
        const int slot = g_slot[tid];
        r_img[(size_t)slot * 32 + 31] = 1.0f;
        if (kitti) {
            double* row = kitti + ((size_t)blockIdx.x * topk + slot) * 16;
#pragma unroll
            for (int e = 0; e < 16; ++e) row[e] = 0.0;
        }
    }
}

extern void rt_set_error(const char* fmt, ...);

extern "C" int rtm3d_box_overlaps(void* stream, int B, int cap_a, int cap_b, const int32_t* d_na, const int32_t* d_nb, const double* d_a,
                                  const double* d_b, int criterion, double* d_bev, double* d_3d) {
    if (B <= 0 || cap_a <= 0 || cap_b <= 0) { rt_set_error("box_overlaps: bad sizes (B %d, cap_a %d, cap_b %d)", B, cap_a, cap_b); return 1; }
    if (!d_na || !d_nb || !d_a || !d_b) { rt_set_error("box_overlaps: null pointer"); return 1; }
    if (!d_bev && !d_3d) { rt_set_error("box_overlaps: both outputs are NULL"); return 1; }
    if (criterion < 0 || criterion > 2) { rt_set_error("box_overlaps: unknown criterion %d (0 iou, 1 over a, 2 over b)", criterion); return 1; }
    const long long total = (long long)B * cap_a * cap_b;
    const long long blocks = (total + BO_LANES - 1) / BO_LANES;
    if (blocks > 0x7fffffffLL) { rt_set_error("box_overlaps: %lld pairs are more than one launch holds", total); return 1; }
    hipLaunchKernelGGL(box_overlaps_kernel, dim3((unsigned)blocks), dim3(BO_LANES), 0, (hipStream_t)stream, total, cap_a, cap_b, d_na, d_nb,
                       d_a, d_b, criterion, d_bev, d_3d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("box_overlaps launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int rtm3d_records_nms3d(void* stream, int B, int topk, float* d_rec, double iou_thresh, int metric, int class_aware,
                                   double* d_kitti) {
    if (B <= 0 || topk <= 0) { rt_set_error("records_nms3d: bad sizes (B %d, topk %d)", B, topk); return 1; }
    if (topk > NMS_MAX_TOPK) { rt_set_error("records_nms3d: topk %d is more than the %d slots per image this kernel holds", topk, NMS_MAX_TOPK); return 1; }
    if (!d_rec) { rt_set_error("records_nms3d: null pointer"); return 1; }
    if (metric != 0 && metric != 1) { rt_set_error("records_nms3d: unknown metric %d (0 BEV IoU, 1 3D IoU)", metric); return 1; }
    if (iou_thresh != iou_thresh) { rt_set_error("records_nms3d: iou_thresh is NaN"); return 1; }
    hipLaunchKernelGGL(records_nms3d_kernel, dim3(B), dim3(BO_LANES), 0, (hipStream_t)stream, topk, d_rec, iou_thresh, metric, class_aware,
                       d_kitti);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("records_nms3d launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
