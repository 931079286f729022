// The device side of the KITTI AP protocol (include/rtm3d_hip.h, "KITTI evaluation"; host side: rtm3d_amd/kitti_eval.py):
//   rtm3d_rect_overlaps   pairwise overlaps of axis-aligned image rectangles of two ragged lists per frame, one lane per pair;
//   rtm3d_kitti_match     the greedy matching of detections to ground truths, one wavefront per (frame, class, difficulty) in
//                         scores mode and per (frame, class, difficulty, score threshold) in counts mode.
// The matching never computes an overlap: it reads one matrix [cap_d][cap_g] per frame, whatever metric produced it
// (rtm3d_rect_overlaps for bbox, rtm3d_box_overlaps for BEV / 3D).  Every float that is compared is fp64; the file is compiled
// without contraction (Makefile), so rtm3d_rect_overlaps is one fixed operation order that numpy reproduces bit for bit.
//
// Matching, per wave: lane L holds detections 4 L .. 4 L + 3 (at most 256 per frame) in statically unrolled registers - score,
// flag, and one "assigned" bit each; nothing is indexed at run time, so there is no private memory and no LDS.  The ground
// truths are walked serially (the assignment is sequential in them).  One step = every lane picks its own best candidate
// (lowest k wins a tie: strict >), a wave maximum, and a ballot of the lanes that hold it: the lowest such lane holds the
// lowest detection index, because a lane's detections are consecutive.
#include "common.h"
#include "../../include/rtm3d_hip.h"

#define RO_LANES 256
#define KM_WAVES 4
#define KM_PER_LANE 4
#define KM_MAX_DET (64 * KM_PER_LANE)

__global__ __launch_bounds__(RO_LANES) void rect_overlaps_kernel(long long total, int cap_a, int cap_b, const int32_t* __restrict__ na,
                                                                const int32_t* __restrict__ nb, const double* __restrict__ A,
                                                                const double* __restrict__ Bx, int criterion, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * RO_LANES + threadIdx.x;
    if (t >= total) return;
    const long long per = (long long)cap_a * cap_b;
    const int img = (int)(t / per);
    const int r = (int)(t - img * per);
    const int i = r / cap_b, j = r - i * cap_b;
    double o = 0.0;
    if (i < na[img] && j < nb[img]) {
        const double* a = A + ((size_t)img * cap_a + i) * 4;
        const double* b = Bx + ((size_t)img * cap_b + j) * 4;
        const double ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3], bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
        const double w = fmin(ax2, bx2) - fmax(ax1, bx1);
        const double h = fmin(ay2, by2) - fmax(ay1, by1);
        const bool finite = __builtin_isfinite(ax1) && __builtin_isfinite(ay1) && __builtin_isfinite(ax2) && __builtin_isfinite(ay2) &&
                            __builtin_isfinite(bx1) && __builtin_isfinite(by1) && __builtin_isfinite(bx2) && __builtin_isfinite(by2);
        if (finite && !(w <= 0.0 || h <= 0.0)) {
            const double inter = w * h;
            const double sa = (ax2 - ax1) * (ay2 - ay1), sb = (bx2 - bx1) * (by2 - by1);
            const double den = criterion == 0 ? (sa + sb) - inter : (criterion == 1 ? sa : sb);
            if (den != 0.0 && __builtin_isfinite(den)) {
                o = inter / den;
                if (!__builtin_isfinite(o)) o = 0.0;           // a quotient that overflows
            }
        }
    }
    out[t] = o;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// MODE 0: scores mode (the devkit's compute_fp = false), one wave per item; MODE 1: counts mode, one wave per (item, threshold).
template <int MODE>
__global__ __launch_bounds__(64 * KM_WAVES) void kitti_match_kernel(
    long long n_work, int n_groups, int cap_d, int cap_g, const int32_t* __restrict__ nd, const int32_t* __restrict__ ng,
    const int8_t* __restrict__ gflag, const int8_t* __restrict__ dflag, const double* __restrict__ score, const uint8_t* __restrict__ dc_hit,
    const double* __restrict__ alpha_g, const double* __restrict__ alpha_d, const double* __restrict__ overlap,
    const double* __restrict__ min_overlap, double* __restrict__ match_score, int max_thr, const int32_t* __restrict__ nthr,
    const double* __restrict__ thr, int32_t* __restrict__ tp, int32_t* __restrict__ fp, int32_t* __restrict__ fn, double* __restrict__ sim) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long w = (long long)blockIdx.x * KM_WAVES + wave;
    if (w >= n_work) return;
    long long item = w;
    int t = 0;
    if (MODE == 1) { item = w / max_thr; t = (int)(w - item * max_thr); }
    const long long frame = item / n_groups;
    const int grp = (int)(item - frame * n_groups);
    double tcut = 0.0;
    if (MODE == 1) {
        if (t >= nthr[grp]) {                              // no such threshold in this group: the partial is defined, nothing is counted
            if (lane == 0) sim[w] = 0.0;
            return;
        }
        tcut = thr[(size_t)grp * max_thr + t];
    }
    const double ninf = -__builtin_inf();
    const double mo = min_overlap[grp];
    const int n_d = min(max(nd[frame], 0), cap_d), n_g = min(max(ng[frame], 0), cap_g);
    const int8_t* GF = gflag + (size_t)item * cap_g;
    const int8_t* DF = dflag + (size_t)item * cap_d;
    const double* OV = overlap + (size_t)frame * cap_d * cap_g;
    double* MS = MODE == 0 ? match_score + (size_t)item * cap_g : nullptr;

    double sc[KM_PER_LANE];
    int df[KM_PER_LANE];                                   // -1: takes no part (other class, past the count, below the threshold)
#pragma unroll
    for (int k = 0; k < KM_PER_LANE; ++k) {
        const int d = lane * KM_PER_LANE + k;
        sc[k] = 0.0; df[k] = -1;
        if (d < n_d) {
            sc[k] = score[(size_t)frame * cap_d + d];
            df[k] = DF[d];
            if (MODE == 1 && sc[k] < tcut) df[k] = -1;      // strict: a detection AT the threshold exists
        }
    }
    unsigned assigned = 0u;
    int n_tp = 0, n_fn = 0;
    double s = 0.0;

    for (int g = 0; g < n_g; ++g) {
        const int gf = GF[g];
        if (gf == -1) {
            if (MODE == 0 && lane == 0) MS[g] = ninf;
            continue;
        }
        // The devkit walks the detections once, keeping max_overlap and assigned_ignored_det: a counted (flag 0) detection takes
        // over from an ignored one whatever its overlap, after that only a strictly larger overlap takes over, and an ignored
        // (flag 1) detection is taken only while nothing is held.  With min_overlap >= 0 its outcome has a closed form: if any
        // eligible detection has flag 0, the one of largest overlap among those, lowest index at a tie; otherwise the
        // lowest-index eligible detection with flag 1.  Scores mode: the eligible detection of highest score, lowest index at a tie.
        double best = ninf;
        int bk = -1, bdf = 0, ik = -1;
#pragma unroll
        for (int k = 0; k < KM_PER_LANE; ++k) {
            if (df[k] != -1 && !((assigned >> k) & 1u)) {
                const double ov = OV[(size_t)(lane * KM_PER_LANE + k) * cap_g + g];
                if (ov > mo) {
                    if (MODE == 0) {
                        if (bk < 0 || sc[k] > best) { best = sc[k]; bk = k; bdf = df[k]; }
                    } else if (df[k] == 0) {
                        if (bk < 0 || ov > best) { best = ov; bk = k; }
                    } else if (df[k] == 1 && ik < 0) {
                        ik = k;
                    }
                }
            }
        }
        int wl = -1, wk = 0, wdf = 0;
        double m = ninf;
        if (__ballot(bk >= 0)) {
            m = wave_max(bk >= 0 ? best : ninf);
            const unsigned long long win = __ballot(bk >= 0 && best == m);
            if (win) {
                wl = __ffsll(win) - 1;
                wk = __shfl(bk, wl, 64);
                wdf = MODE == 0 ? __shfl(bdf, wl, 64) : 0;
            }
        } else if (MODE == 1) {
            const unsigned long long ign = __ballot(ik >= 0);
            if (ign) {
                wl = __ffsll(ign) - 1;
                wk = __shfl(ik, wl, 64);
                wdf = 1;
            }
        }
        if (wl < 0) {                                      // no candidate
            if (gf == 0) ++n_fn;
            if (MODE == 0 && lane == 0) MS[g] = ninf;
            continue;
        }
        if (lane == wl) assigned |= 1u << wk;
        if (gf == 1 || wdf == 1) {                         // assigned, nothing counted
            if (MODE == 0 && lane == 0) MS[g] = ninf;
            continue;
        }
        ++n_tp;
        if (MODE == 0) {
            if (lane == 0) MS[g] = m;
        } else if (alpha_g && alpha_d) {
            const double delta = alpha_g[(size_t)frame * cap_g + g] - alpha_d[(size_t)frame * cap_d + wl * KM_PER_LANE + wk];
            s = s + (1.0 + cos(delta)) / 2.0;
        }
    }

    if (MODE == 0) {
        for (int g = n_g + lane; g < cap_g; g += 64) MS[g] = ninf;
    } else {
        const uint8_t* DC = dc_hit ? dc_hit + (size_t)item * cap_d : nullptr;
        int n_fp = 0;
#pragma unroll
        for (int k = 0; k < KM_PER_LANE; ++k) {
            bool c = df[k] == 0 && !((assigned >> k) & 1u);
            if (c && DC) c = DC[lane * KM_PER_LANE + k] == 0;
            n_fp += __popcll(__ballot(c));
        }
        if (lane == 0) {
            const size_t o = (size_t)grp * max_thr + t;
            if (n_tp) atomicAdd(&tp[o], n_tp);
            if (n_fp) atomicAdd(&fp[o], n_fp);
            if (n_fn) atomicAdd(&fn[o], n_fn);
            sim[w] = s;
        }
    }
}

extern void rt_set_error(const char* fmt, ...);

extern "C" int rtm3d_rect_overlaps(void* stream, int B, int cap_a, int cap_b, const int32_t* d_na, const int32_t* d_nb, const double* d_a,
                                   const double* d_b, int criterion, double* d_out) {
    if (B <= 0 || cap_a <= 0 || cap_b <= 0) { rt_set_error("rect_overlaps: bad sizes (B %d, cap_a %d, cap_b %d)", B, cap_a, cap_b); return 1; }
    if (!d_na || !d_nb || !d_a || !d_b || !d_out) { rt_set_error("rect_overlaps: null pointer"); return 1; }
    if (criterion < 0 || criterion > 2) { rt_set_error("rect_overlaps: unknown criterion %d (0 iou, 1 over a, 2 over b)", criterion); return 1; }
    const long long total = (long long)B * cap_a * cap_b;
    const long long blocks = (total + RO_LANES - 1) / RO_LANES;
    if (blocks > 0x7fffffffLL) { rt_set_error("rect_overlaps: %lld pairs are more than one launch holds", total); return 1; }
    hipLaunchKernelGGL(rect_overlaps_kernel, dim3((unsigned)blocks), dim3(RO_LANES), 0, (hipStream_t)stream, total, cap_a, cap_b, d_na, d_nb,
                       d_a, d_b, criterion, d_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("rect_overlaps launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int rtm3d_kitti_match(void* stream, int mode, int n_frames, int n_groups, int cap_d, int cap_g, const int32_t* d_nd,
                                 const int32_t* d_ng, const int8_t* d_gflag, const int8_t* d_dflag, const double* d_score,
                                 const uint8_t* d_dc_hit, const double* d_alpha_g, const double* d_alpha_d, const double* d_overlap,
                                 const double* d_min_overlap, double* d_match_score, int max_thr, const int32_t* d_nthr, const double* d_thr,
                                 int32_t* d_tp, int32_t* d_fp, int32_t* d_fn, double* d_sim) {
    if (mode != 0 && mode != 1) { rt_set_error("kitti_match: unknown mode %d (0 scores, 1 counts)", mode); return 1; }
    if (n_frames <= 0 || n_groups <= 0 || cap_d <= 0 || cap_g <= 0) {
        rt_set_error("kitti_match: bad sizes (frames %d, groups %d, cap_d %d, cap_g %d)", n_frames, n_groups, cap_d, cap_g);
        return 1;
    }
    if (cap_d > KM_MAX_DET) { rt_set_error("kitti_match: cap_d %d is more than the %d detections per frame this kernel holds", cap_d, KM_MAX_DET); return 1; }
    if (!d_nd || !d_ng || !d_gflag || !d_dflag || !d_score || !d_overlap || !d_min_overlap) { rt_set_error("kitti_match: null pointer"); return 1; }
    if ((d_alpha_g == nullptr) != (d_alpha_d == nullptr)) { rt_set_error("kitti_match: d_alpha_g and d_alpha_d go together"); return 1; }
    long long n_work = (long long)n_frames * n_groups;
    if (mode == 0) {
        if (!d_match_score) { rt_set_error("kitti_match: scores mode needs d_match_score"); return 1; }
    } else {
        if (max_thr <= 0 || !d_nthr || !d_thr || !d_tp || !d_fp || !d_fn || !d_sim) {
            rt_set_error("kitti_match: counts mode needs max_thr > 0 (got %d), d_nthr, d_thr, d_tp, d_fp, d_fn and d_sim", max_thr);
            return 1;
        }
        n_work *= max_thr;
    }
    const long long blocks = (n_work + KM_WAVES - 1) / KM_WAVES;
    if (blocks > 0x7fffffffLL) { rt_set_error("kitti_match: %lld matchings are more than one launch holds", n_work); return 1; }
    if (mode == 0)
        hipLaunchKernelGGL(kitti_match_kernel<0>, dim3((unsigned)blocks), dim3(64 * KM_WAVES), 0, (hipStream_t)stream, n_work, n_groups, cap_d,
                           cap_g, d_nd, d_ng, d_gflag, d_dflag, d_score, d_dc_hit, d_alpha_g, d_alpha_d, d_overlap, d_min_overlap,
                           d_match_score, max_thr, d_nthr, d_thr, d_tp, d_fp, d_fn, d_sim);
    else
        hipLaunchKernelGGL(kitti_match_kernel<1>, dim3((unsigned)blocks), dim3(64 * KM_WAVES), 0, (hipStream_t)stream, n_work, n_groups, cap_d,
                           cap_g, d_nd, d_ng, d_gflag, d_dflag, d_score, d_dc_hit, d_alpha_g, d_alpha_d, d_overlap, d_min_overlap,
                           d_match_score, max_thr, d_nthr, d_thr, d_tp, d_fp, d_fn, d_sim);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("kitti_match launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
