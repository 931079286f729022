// Tracking evaluation on the device (include/rtm3d_hip.h, "tracking evaluation"): HOTA and CLEAR-MOT over per-frame similarity
// matrices of whatever metric, everything fp64, compiled with -ffp-contract=off.
//   mot_assign_kernel      one wave per frame: ASSIGN on a given score matrix (rtm3d_mot_assign; the KITTI preprocessing uses it);
//   mot_sums_kernel        one workgroup per frame: row and column sums of sim over the valid entries, in index order;
//   mot_align_kernel       one lane per (gid, tid) pair of a sequence, walking that sequence's frames in order through the slot
//                          tables: potential, gcount, tcount and the alignment score A.  The sum of a pair is ONE lane's running
//                          sum in frame order, so it is defined bit for bit; there is no fp64 atomic anywhere in this file;
//   mot_hota_match_kernel  one wave per frame: ASSIGN on w = A * sim computed on the fly, then the per-alpha counts (integer
//                          vector atomics: order-free) and the similarity of every matched pair into the workspace;
//   mot_loc_kernel         one wave per sequence: loc[a], ONE running sum per alpha (lane a) over the matched similarities in
//                          frame order, then ground-truth slot order - 64 values per load, handed round by lane reads;
//   mot_clear_kernel       one wave per sequence, walking its frames with the carried identity state.  A frame's scores depend on
//                          the previous frame's match, so the frames of a sequence are a chain: S waves are all the parallelism
//                          CLEAR has.
// ASSIGN is the one-wave shortest-augmenting-path solver of assign_wave.h (the tracker's optimal match runs the same text) on a
// frame of ng x nt with the gain w: every ground-truth slot 0 .. ng - 1 is a root, in slot order, and lane L owns NC tracker slots.
// A frame with ng, nt <= 64 runs it with one column per lane (NC = 1), a larger one with four (NC = 4): the work follows the
// frame's own size, never the caps.  The tie rule - the lowest tracker slot at equal slack, "stay unmatched" at a tie with it -
// is the solver's.
#include "common.h"
#include "../../include/rtm3d_hip.h"
#include "assign_wave.h"

#define MOT_MAX 256                 // ground truths and tracker boxes per frame, at most
#define MOT_EPS 2.220446049250313e-16
#define MOT_NALPHA RTM3D_MOT_ALPHAS
#define MOT_INF (__builtin_inf())

// global memory handed between lanes of one wave from one frame to the next (mot_clear_kernel)
#define MOT_GSYNC() do { __threadfence(); __builtin_amdgcn_wave_barrier(); } while (0)

struct MotLds {                     // the solver's four arrays (assign_wave.h: AssignWave) and rowaux
    double row_dual[MOT_MAX];       // [ground-truth slot] dual of the row
    int row_col[MOT_MAX];           // ground-truth slot -> tracker slot it holds, -1 none
    int col_row[MOT_MAX];           // tracker slot -> ground-truth slot that holds it, -1 none
    int pred[MOT_MAX];              // tracker slot -> the row its slack came from, this path
    int rowaux[MOT_MAX];            // per row: its gid (HOTA) or the tracker id of its previous match (CLEAR), -1 none
};

__device__ __forceinline__ int mot_wave_sum(int x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

__device__ __forceinline__ int mot_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the score of (row i, column col): aux = rowaux[i], ct = the tracker id of the column
struct MotWPlain {
    const double* w; int ld;
    __device__ __forceinline__ double operator()(int i, int aux, int col, int ct) const { return w[(size_t)i * ld + col]; }
};
struct MotWHota {                   // w = A[gid][tid] * sim
    const double* sim; int ld; const double* A; int n_tid;
    __device__ __forceinline__ double operator()(int i, int aux, int col, int ct) const {
        if (aux < 0 || ct < 0) return 0.0;
        return A[(size_t)aux * n_tid + ct] * sim[(size_t)i * ld + col];
    }
};
struct MotWClear {                  // w = 1000 * (prev[gid] == tid) + sim, 0 where sim < thr - eps (cut = thr - eps)
    const double* sim; int ld; double cut;
    __device__ __forceinline__ double operator()(int i, int aux, int col, int ct) const {
        const double s = sim[(size_t)i * ld + col];
        if (s < cut) return 0.0;
        return (aux >= 0 && aux == ct ? 1000.0 : 0.0) + s;
    }
};

// ASSIGN of one frame by one wave with NC columns per lane: L.rowaux is set by the caller, tids are the tracker ids of the frame's
// columns or NULL; on return (after a wave sync) L.row_col holds the match
template <int NC, class WF>
__device__ __forceinline__ void mot_assign_frame(int ng, int nt, const WF& wf, MotLds& L, const int (&ct)[NC], int wl) {
    for (int q = wl; q < MOT_MAX; q += 64) { L.row_dual[q] = 0.0; L.row_col[q] = -1; L.col_row[q] = -1; }
    AW_WSYNC();
    uint32_t live = 0u;                                       // this lane's columns that exist
#pragma unroll
    for (int c = 0; c < NC; ++c) if (NC * wl + c < nt) live |= 1u << c;
    const AssignWave st{L.row_dual, L.row_col, L.col_row, L.pred};
    double v[NC];                                             // column duals
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = 0.0;
    for (int cur = 0; cur < ng; ++cur) {                      // one augmentation per row, in slot order
        AwPath p = aw_path(cur);
        for (int step = 0; step <= nt; ++step) {              // every step scans another matched row or ends: at most nt + 1
            const int i = p.i, aux = L.rowaux[i];
            const auto gain = [&](int c, double& g) {
                g = wf(i, aux, NC * wl + c, ct[c]);
                return g > 0.0;
            };
            aw_step<NC>(st, p, v, wl, live, gain);
            if (p.sink != -2) break;
        }
        aw_finish<NC>(st, p, v, cur, nt, wl);
    }
    AW_WSYNC();
}

// the frame's own size picks the form
template <class WF>
__device__ __forceinline__ void mot_run(int ng, int nt, const WF& wf, MotLds& L, const int32_t* __restrict__ tids, int n_tid, int wl) {
    if (ng <= 64 && nt <= 64) {
        int ct[1];
        ct[0] = -1;
        if (tids && wl < nt) { const int t = tids[wl]; ct[0] = t >= 0 && t < n_tid ? t : -1; }
        mot_assign_frame<1>(ng, nt, wf, L, ct, wl);
    } else {
        int ct[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            ct[c] = -1;
            if (tids && 4 * wl + c < nt) { const int t = tids[4 * wl + c]; ct[c] = t >= 0 && t < n_tid ? t : -1; }
        }
        mot_assign_frame<4>(ng, nt, wf, L, ct, wl);
    }
}

// the sequence of frame f: the s with seq_start[s] <= f < seq_start[s + 1] (empty sequences are skipped)
__device__ __forceinline__ int mot_seq_of(const int32_t* __restrict__ seq_start, int S, int f) {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seq_start[mid + 1] <= f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void mot_assign_kernel(int cap_g, int cap_t, const int32_t* __restrict__ d_ng, const int32_t* __restrict__ d_nt,
                                                       const double* __restrict__ w, int32_t* __restrict__ match) {
    __shared__ MotLds L;
    const int f = blockIdx.x, wl = threadIdx.x;
    const int ng = mot_clamp(d_ng[f], cap_g), nt = mot_clamp(d_nt[f], cap_t);
    for (int q = wl; q < MOT_MAX; q += 64) L.rowaux[q] = -1;
    mot_run(ng, nt, MotWPlain{w + (size_t)f * cap_g * cap_t, cap_t}, L, nullptr, 0, wl);
    for (int g = wl; g < cap_g; g += 64) match[(size_t)f * cap_g + g] = g < ng ? L.row_col[g] : -1;
}

__global__ __launch_bounds__(256) void mot_sums_kernel(int cap_g, int cap_t, const int32_t* __restrict__ d_ng, const int32_t* __restrict__ d_nt,
                                                      const double* __restrict__ sim, double* __restrict__ rowsum, double* __restrict__ colsum) {
    const int f = blockIdx.x, q = threadIdx.x;
    const int ng = mot_clamp(d_ng[f], cap_g), nt = mot_clamp(d_nt[f], cap_t);
    const double* s = sim + (size_t)f * cap_g * cap_t;
    if (q < cap_g) {
        double acc = 0.0;
        if (q < ng) for (int t = 0; t < nt; ++t) acc = acc + s[(size_t)q * cap_t + t];
        rowsum[(size_t)f * cap_g + q] = acc;
    }
    if (q < cap_t) {
        double acc = 0.0;
        if (q < nt) for (int g = 0; g < ng; ++g) acc = acc + s[(size_t)g * cap_t + q];
        colsum[(size_t)f * cap_t + q] = acc;
    }
}

__global__ __launch_bounds__(256) void mot_align_kernel(int cap_g, int cap_t, int n_gid, int n_tid, const int32_t* __restrict__ seq_start,
                                                       const int32_t* __restrict__ gslot, const int32_t* __restrict__ tslot,
                                                       const double* __restrict__ sim, const double* __restrict__ rowsum,
                                                       const double* __restrict__ colsum, double* __restrict__ potential,
                                                       int32_t* __restrict__ gcount, int32_t* __restrict__ tcount, double* __restrict__ A) {
    const int s = blockIdx.y;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)n_gid * n_tid) return;
    const int i = (int)(p / n_tid), j = (int)(p - (long long)i * n_tid);
    const int f0 = seq_start[s], f1 = seq_start[s + 1];
    double acc = 0.0;
    int gc = 0, tc = 0;
    for (int f = f0; f < f1; ++f) {
        const int gs = gslot[(size_t)f * n_gid + i], ts = tslot[(size_t)f * n_tid + j];
        const bool hg = gs >= 0 && gs < cap_g, ht = ts >= 0 && ts < cap_t;
        gc += hg ? 1 : 0;
        tc += ht ? 1 : 0;
        if (hg && ht) {
            const double sv = sim[((size_t)f * cap_g + gs) * cap_t + ts];
            const double den = (rowsum[(size_t)f * cap_g + gs] + colsum[(size_t)f * cap_t + ts]) - sv;
            acc = acc + (den > 0.0 ? sv / den : 0.0);
        }
    }
    const size_t o = ((size_t)s * n_gid + i) * n_tid + j;
    potential[o] = acc;
    if (j == 0) gcount[(size_t)s * n_gid + i] = gc;
    if (i == 0) tcount[(size_t)s * n_tid + j] = tc;
    const double den = (double)(gc + tc) - acc;
    A[o] = den > 0.0 ? acc / den : 0.0;
}

__global__ __launch_bounds__(64) void mot_hota_match_kernel(int S, int cap_g, int cap_t, int n_gid, int n_tid, const int32_t* __restrict__ seq_start,
                                                           const int32_t* __restrict__ d_ng, const int32_t* __restrict__ d_nt,
                                                           const int32_t* __restrict__ gid, const int32_t* __restrict__ tid,
                                                           const double* __restrict__ sim, const double* __restrict__ A,
                                                           int32_t* __restrict__ match, double* __restrict__ msim, int32_t* __restrict__ tp,
                                                           int32_t* __restrict__ fn, int32_t* __restrict__ fp, int32_t* __restrict__ mc) {
    __shared__ MotLds L;
    const int f = blockIdx.x, wl = threadIdx.x;
    const int ng = mot_clamp(d_ng[f], cap_g), nt = mot_clamp(d_nt[f], cap_t);
    const int s = mot_seq_of(seq_start, S, f);
    const double* sf = sim + (size_t)f * cap_g * cap_t;
    for (int q = wl; q < MOT_MAX; q += 64) {
        int gi = -1;
        if (q < ng) { gi = gid[(size_t)f * cap_g + q]; if (gi < 0 || gi >= n_gid) gi = -1; }
        L.rowaux[q] = gi;
    }
    mot_run(ng, nt, MotWHota{sf, cap_t, A + (size_t)s * n_gid * n_tid, n_tid}, L, tid + (size_t)f * cap_t, n_tid, wl);
    int mine = 0;                                             // lane a: the pairs counted at alpha_a in this frame
    for (int base = 0; base < cap_g; base += 64) {
        const int g = base + wl;
        const int m = g < ng ? L.row_col[g] : -1;
        double sv = -1.0;
        int gi = -1, ti = -1;
        if (m >= 0) {
            sv = sf[(size_t)g * cap_t + m];
            gi = L.rowaux[g];
            ti = tid[(size_t)f * cap_t + m];
            if (ti < 0 || ti >= n_tid) ti = -1;
        }
        if (g < cap_g) { match[(size_t)f * cap_g + g] = m; msim[(size_t)f * cap_g + g] = sv; }
        if (base < ng) {
#pragma unroll 1
            for (int a = 0; a < MOT_NALPHA; ++a) {
                const double alpha = 0.05 + (double)a * 0.05;
                const bool counted = m >= 0 && sv >= alpha - MOT_EPS;
                const int n = __popcll(__ballot(counted));
                if (wl == a) mine += n;
                if (counted && gi >= 0 && ti >= 0) atomicAdd(&mc[(((size_t)s * MOT_NALPHA + a) * n_gid + gi) * n_tid + ti], 1);
            }
        }
    }
    if (wl < MOT_NALPHA) {
        atomicAdd(&tp[s * MOT_NALPHA + wl], mine);
        atomicAdd(&fn[s * MOT_NALPHA + wl], ng - mine);
        atomicAdd(&fp[s * MOT_NALPHA + wl], nt - mine);
    }
}

__global__ __launch_bounds__(64) void mot_loc_kernel(int cap_g, const int32_t* __restrict__ seq_start, const double* __restrict__ msim,
                                                    double* __restrict__ loc) {
    const int s = blockIdx.x, wl = threadIdx.x;
    const size_t first = (size_t)seq_start[s] * cap_g, n = (size_t)(seq_start[s + 1] - seq_start[s]) * cap_g;
    const double bar = wl < MOT_NALPHA ? (0.05 + (double)wl * 0.05) - MOT_EPS : MOT_INF;
    double acc = 0.0;
    for (size_t base = 0; base < n; base += 64) {
        const double x = base + wl < n ? msim[first + base + wl] : -1.0;
        unsigned long long todo = __ballot(x >= 0.0);         // the matched pairs of these 64 slots, in order
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            const double y = __shfl(x, k, 64);
            if (y >= bar) acc = acc + y;
        }
    }
    if (wl < MOT_NALPHA) loc[s * MOT_NALPHA + wl] = acc;
}

__global__ __launch_bounds__(64) void mot_clear_kernel(int cap_g, int cap_t, int n_gid, int n_tid, const int32_t* __restrict__ seq_start,
                                                      const int32_t* __restrict__ d_ng, const int32_t* __restrict__ d_nt,
                                                      const int32_t* __restrict__ gid, const int32_t* __restrict__ tid,
                                                      const double* __restrict__ sim, double cut, int32_t* __restrict__ match,
                                                      int32_t* __restrict__ counts, double* __restrict__ simsum, int32_t* __restrict__ idcount,
                                                      int32_t* __restrict__ matched, int32_t* __restrict__ frag, int32_t* __restrict__ ws) {
    __shared__ MotLds L;
    const int s = blockIdx.x, wl = threadIdx.x;
    int32_t* last = ws + (size_t)s * 3 * n_gid;               // tracker id of the most recent match, -1 none
    int32_t* prev_tid = last + n_gid;                         // tracker id of the match in processed frame prev_at, valid iff
    int32_t* prev_at = prev_tid + n_gid;                      //   prev_at == the number of frames processed so far
    idcount += (size_t)s * n_gid; matched += (size_t)s * n_gid; frag += (size_t)s * n_gid;
    for (int q = wl; q < n_gid; q += 64) { last[q] = -1; prev_tid[q] = -1; prev_at[q] = -1; }
    MOT_GSYNC();
    int tp = 0, fn = 0, fp = 0, sw = 0, done = 0;             // tp, fn, sw: per lane, summed at the end; fp, done: wave-uniform
    double ssum = 0.0;                                        // the same running sum in every lane
    const int f0 = seq_start[s], f1 = seq_start[s + 1];
    for (int f = f0; f < f1; ++f) {
        const int ng = mot_clamp(d_ng[f], cap_g), nt = mot_clamp(d_nt[f], cap_t);
        int32_t* mrow = match + (size_t)f * cap_g;
        if (ng == 0 || nt == 0) {                             // nothing to match: counted, the carried state stays as it is
            fp += nt;
            if (wl == 0) fn += ng;
            for (int g = wl; g < cap_g; g += 64) mrow[g] = -1;
            if (ng > 0) {                                     // the tracker is empty: the frame still counts in its ids' lives
                for (int g = wl; g < ng; g += 64) {
                    const int gi = gid[(size_t)f * cap_g + g];
                    if (gi >= 0 && gi < n_gid) idcount[gi] += 1;
                }
                MOT_GSYNC();                                  // another lane may own the id in the next frame
            }
            continue;
        }
        const int32_t* gf = gid + (size_t)f * cap_g;
        const int32_t* tf = tid + (size_t)f * cap_t;
        const double* sf = sim + (size_t)f * cap_g * cap_t;
        for (int q = wl; q < MOT_MAX; q += 64) {
            int pv = -1;
            if (q < ng) { const int gi = gf[q]; if (gi >= 0 && gi < n_gid && prev_at[gi] == done) pv = prev_tid[gi]; }
            L.rowaux[q] = pv;
        }
        mot_run(ng, nt, MotWClear{sf, cap_t, cut}, L, tf, n_tid, wl);
        int hits = 0;
        for (int base = 0; base < cap_g; base += 64) {
            const int g = base + wl;
            const int m = g < ng ? L.row_col[g] : -1;
            double sv = 0.0;
            if (g < ng) {
                const int gi = gf[g];
                const bool ok = gi >= 0 && gi < n_gid;
                if (ok) idcount[gi] += 1;
                if (m >= 0) {
                    const int t = tf[m];
                    sv = sf[(size_t)g * cap_t + m];
                    ++tp;
                    if (ok) {
                        matched[gi] += 1;
                        const int l = last[gi];
                        if (l >= 0 && l != t) ++sw;
                        last[gi] = t;
                        if (L.rowaux[g] < 0) frag[gi] += 1;
                        prev_tid[gi] = t;
                        prev_at[gi] = done + 1;
                    }
                } else {
                    ++fn;
                }
            }
            if (g < cap_g) mrow[g] = m;
            unsigned long long todo = __ballot(m >= 0);
            hits += __popcll(todo);
            while (todo) {                                    // simsum: frame order, then ground-truth slot order
                const int k = __ffsll(todo) - 1;
                todo &= todo - 1ull;
                ssum = ssum + __shfl(sv, k, 64);
            }
        }
        fp += nt - hits;
        ++done;
        MOT_GSYNC();
    }
    tp = mot_wave_sum(tp); fn = mot_wave_sum(fn); sw = mot_wave_sum(sw);
    if (wl == 0) {
        counts[s * 4 + 0] += tp; counts[s * 4 + 1] += fn; counts[s * 4 + 2] += fp; counts[s * 4 + 3] += sw;
        simsum[s] = ssum;
    }
}

extern void rt_set_error(const char* fmt, ...);

static bool mot_sizes_ok(const char* what, int S, int F, int cap_g, int cap_t, int n_gid, int n_tid, bool say) {
    const char* bad = nullptr;
    if (S < 1) bad = "S (sequences) must be positive";
    else if (F < 1) bad = "F (frames) must be positive";
    else if (cap_g < 1 || cap_g > MOT_MAX) bad = "cap_g must be in 1..256";
    else if (cap_t < 1 || cap_t > MOT_MAX) bad = "cap_t must be in 1..256";
    else if (n_gid < 1 || n_tid < 1) bad = "n_gid and n_tid must be positive";
    else if ((double)S * MOT_NALPHA * n_gid * n_tid > 2147483647.0) bad = "S * 19 * n_gid * n_tid exceeds 2^31 - 1";
    else if ((double)F * cap_g * cap_t > 4.0e9 || (double)F * (n_gid > n_tid ? n_gid : n_tid) > 2147483647.0) bad = "too many frames for these sizes";
    if (bad && say) rt_set_error("%s: %s (S %d, F %d, cap_g %d, cap_t %d, n_gid %d, n_tid %d)", what, bad, S, F, cap_g, cap_t, n_gid, n_tid);
    return bad == nullptr;
}

// workspace layout, in doubles: rowsum [F][cap_g], msim [F][cap_g], colsum [F][cap_t], A [S][n_gid][n_tid]; CLEAR uses the front
// as 3 * S * n_gid int32
extern "C" size_t rtm3d_mot_workspace_bytes(int S, int F, int cap_g, int cap_t, int n_gid, int n_tid) {
    if (!mot_sizes_ok("mot_workspace_bytes", S, F, cap_g, cap_t, n_gid, n_tid, false)) return 0;
    const size_t hota = ((size_t)F * cap_g * 2 + (size_t)F * cap_t + (size_t)S * n_gid * n_tid) * sizeof(double);
    const size_t clear = (size_t)3 * S * n_gid * sizeof(int32_t);
    return hota > clear ? hota : clear;
}

#define MOT_LAUNCHED(what) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) { rt_set_error("%s launch: %s", what, hipGetErrorString(e_)); return 1; } } while (0)

extern "C" int rtm3d_mot_assign(void* stream, int F, int cap_g, int cap_t, const int32_t* d_ng, const int32_t* d_nt, const double* d_w,
                                int32_t* d_match) {
    if (!mot_sizes_ok("mot_assign", 1, F, cap_g, cap_t, 1, 1, true)) return 1;
    if (!d_ng || !d_nt || !d_w || !d_match) { rt_set_error("mot_assign: null pointer (d_ng, d_nt, d_w and d_match are required)"); return 1; }
    hipLaunchKernelGGL(mot_assign_kernel, dim3(F), dim3(64), 0, (hipStream_t)stream, cap_g, cap_t, d_ng, d_nt, d_w, d_match);
    MOT_LAUNCHED("mot_assign");
    return 0;
}

extern "C" int rtm3d_mot_hota(void* stream, int S, int F, int cap_g, int cap_t, int n_gid, int n_tid, const int32_t* d_seq_start,
                              const int32_t* d_ng, const int32_t* d_nt, const int32_t* d_gid, const int32_t* d_tid, const int32_t* d_gslot,
                              const int32_t* d_tslot, const double* d_sim, double* d_potential, int32_t* d_gcount, int32_t* d_tcount,
                              int32_t* d_match, int32_t* d_tp, int32_t* d_fn, int32_t* d_fp, double* d_loc, int32_t* d_mc, void* d_ws) {
    if (!mot_sizes_ok("mot_hota", S, F, cap_g, cap_t, n_gid, n_tid, true)) return 1;
    if (!d_seq_start || !d_ng || !d_nt || !d_gid || !d_tid || !d_gslot || !d_tslot || !d_sim || !d_potential || !d_gcount || !d_tcount ||
        !d_match || !d_tp || !d_fn || !d_fp || !d_loc || !d_mc || !d_ws) {
        rt_set_error("mot_hota: null pointer (every array and the workspace are required)"); return 1;
    }
    const long long pair_blocks = ((long long)n_gid * n_tid + 255) / 256;
    if (S > 65535) { rt_set_error("mot_hota: %d sequences are more than one launch holds (65535)", S); return 1; }
    double* rowsum = (double*)d_ws;
    double* msim = rowsum + (size_t)F * cap_g;
    double* colsum = msim + (size_t)F * cap_g;
    double* A = colsum + (size_t)F * cap_t;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mot_sums_kernel, dim3(F), dim3(256), 0, st, cap_g, cap_t, d_ng, d_nt, d_sim, rowsum, colsum);
    MOT_LAUNCHED("mot_hota sums");
    hipLaunchKernelGGL(mot_align_kernel, dim3((unsigned)pair_blocks, S), dim3(256), 0, st, cap_g, cap_t, n_gid, n_tid, d_seq_start, d_gslot, d_tslot,
                       d_sim, (const double*)rowsum, (const double*)colsum, d_potential, d_gcount, d_tcount, A);
    MOT_LAUNCHED("mot_hota alignment");
    hipLaunchKernelGGL(mot_hota_match_kernel, dim3(F), dim3(64), 0, st, S, cap_g, cap_t, n_gid, n_tid, d_seq_start, d_ng, d_nt, d_gid, d_tid, d_sim,
                       (const double*)A, d_match, msim, d_tp, d_fn, d_fp, d_mc);
    MOT_LAUNCHED("mot_hota match");
    hipLaunchKernelGGL(mot_loc_kernel, dim3(S), dim3(64), 0, st, cap_g, d_seq_start, (const double*)msim, d_loc);
    MOT_LAUNCHED("mot_hota loc");
    return 0;
}

extern "C" int rtm3d_mot_clear(void* stream, int S, int F, int cap_g, int cap_t, int n_gid, int n_tid, const int32_t* d_seq_start,
                               const int32_t* d_ng, const int32_t* d_nt, const int32_t* d_gid, const int32_t* d_tid, const double* d_sim,
                               double thr, int32_t* d_match, int32_t* d_counts, double* d_simsum, int32_t* d_idcount, int32_t* d_matched,
                               int32_t* d_frag, void* d_ws) {
    if (!mot_sizes_ok("mot_clear", S, F, cap_g, cap_t, n_gid, n_tid, true)) return 1;
    if (!(thr > -MOT_INF && thr < MOT_INF)) { rt_set_error("mot_clear: thr %g must be finite", thr); return 1; }
    if (!d_seq_start || !d_ng || !d_nt || !d_gid || !d_tid || !d_sim || !d_match || !d_counts || !d_simsum || !d_idcount || !d_matched ||
        !d_frag || !d_ws) {
        rt_set_error("mot_clear: null pointer (every array and the workspace are required)"); return 1;
    }
    hipLaunchKernelGGL(mot_clear_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, cap_g, cap_t, n_gid, n_tid, d_seq_start, d_ng, d_nt, d_gid, d_tid,
                       d_sim, thr - MOT_EPS, d_match, d_counts, d_simsum, d_idcount, d_matched, d_frag, (int32_t*)d_ws);
    MOT_LAUNCHED("mot_clear");
    return 0;
}
