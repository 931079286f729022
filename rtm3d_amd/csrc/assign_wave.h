// The assignment solver of the tracker's optimal match (track.hip, step 3b) and of the tracking evaluation's ASSIGN (mot_eval.hip):
// shortest augmenting paths (Hungarian method in the Jonker-Volgenant form), fp64, run by ONE wave.  Rows take columns so that the
// sum of the gains of the matched pairs is largest, cost = -gain; only candidates are matched, and a candidate's gain is > 0.
// "Stay unmatched" is a zero-cost column private to every row, kept as one scalar per path (the smallest slack of the scanned rows'
// private columns) instead of in memory: such a column is reachable from its own row only, is free whenever that row is scanned,
// and a free column's dual is 0.  Lane L owns the columns NC * L .. NC * L + NC - 1 with their duals and slacks in registers; row
// duals, predecessors and the two owner arrays are in LDS.  A path step has no block barrier: every lane relaxes its unscanned
// candidate columns against the newly scanned row, a wave minimum and a ballot pick the column of least slack - the lowest column
// at equal slack, the private column at a tie with it - and nothing depends on the order in which lanes retire.  Both loops are
// counted.
// The header offers one path STEP (aw_step) and the end of a path (aw_finish); the loop over the roots, the counted loop over
// the steps, and where a row's gains come from, are the caller's:
//     AwPath p = aw_path(cur);
//     for (int step = 0; step <= ncols; ++step) { aw_step<NC>(st, p, v, wl, cand, gain); if (p.sink != -2) break; <fetch row p.i> }
//     aw_finish<NC>(st, p, v, cur, ncols, wl);
// Callers compile with -ffp-contract=off: the expressions below are the definition of the match, ties included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// a wave's LDS instructions execute in order: between lanes of ONE wave this is only a compiler / LDS ordering fence
#define AW_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

__device__ __forceinline__ double aw_wave_min(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = fmin(x, __shfl_xor(x, m, 64));
    return x;
}

// the LDS state of one solve, in arrays of the caller.  Before the first augmentation: row_dual 0, row_col and col_row -1, and
// the writes ordered before the wave that solves (AW_WSYNC, or a block barrier).
struct AssignWave {
    double* row_dual;               // [row] dual of the row
    int* row_col;                   // row -> the column it holds, -1 none
    int* col_row;                   // column -> the row that holds it, -1 none
    int* pred;                      // column -> the row its slack came from, this path
};

// the registers of one path from the free row `cur`
struct AwPath {
    // slacks: shortest path costs of this lane's columns, the first NC.  (A fixed aggregate, not an array of NC filled in a
    // loop: filled in a loop, this compiler turns the choice of the least slack into branches - profiles/track.txt has the
    // times.  The shape of this struct is therefore sensitive to the compiler version; look at the listing after an upgrade.)
    double sp[4];
    uint32_t sc;                    // this lane's scanned columns
    double minval, dbest;           // dbest / drow: least slack of a scanned row's private column
    int drow, sink;                 // sink: -2 none yet, -1 the private column of drow, else a column
    int i;                          // the row to scan next (wave-uniform)
};

__device__ __forceinline__ AwPath aw_path(int cur) {
    return AwPath{{__builtin_inf(), __builtin_inf(), __builtin_inf(), __builtin_inf()}, 0u, 0.0, __builtin_inf(), -1, -2, cur};
}

// One step, by every lane of the wave (wl: the lane): scan row p.i, pick the column of least slack.  v: the duals of this lane's
// columns, 0 before the first path.  cand: bit c set where column NC * wl + c exists and may be a candidate of row p.i;
// gain(c, a), asked for set bits that are not scanned yet: whether the pair is a candidate, and if so its gain in a.  The caller
// guarantees that a candidate's gain is > 0; the step does not check it.  Afterwards p.sink != -2 if the path has ended; else it
// goes on with the matched row p.i, whose gains the caller fetches before the next step.  (The end is read from p.sink, not
// returned: with a returned flag the compiler needs more scalar registers in the evaluator's CLEAR kernel than that kernel has.)
template <int NC, class Gain>
__device__ __forceinline__ void aw_step(const AssignWave& S, AwPath& p, const double (&v)[NC], int wl, uint32_t cand, const Gain& gain) {
    static_assert(NC >= 1 && NC <= 4, "columns per lane");
    const int i = p.i;
    const double ui = S.row_dual[i];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double a;
        if ((((cand & ~p.sc) >> c) & 1u) && gain(c, a)) {
            const double r = ((p.minval - a) - ui) - v[c];
            if (r < p.sp[c]) { p.sp[c] = r; S.pred[NC * wl + c] = i; }
        }
    }
    const double dv = p.minval - ui;
    if (dv < p.dbest) { p.dbest = dv; p.drow = i; }
    double lv = __builtin_inf();
    int lc = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (!((p.sc >> c) & 1u) && p.sp[c] < lv) { lv = p.sp[c]; lc = c; }
    const double m = aw_wave_min(lv);
    const unsigned long long win = __ballot(lv == m);
    if (!(m < p.dbest) || win == 0ull) { p.sink = -1; p.minval = p.dbest; return; }
    const int wlane = __ffsll(win) - 1;                       // lowest lane, and in it the lowest c: the lowest column
    const int j = __builtin_amdgcn_readfirstlane(NC * wlane + __shfl(lc, wlane, 64));
    p.minval = m;
    if (wl == wlane) p.sc |= 1u << lc;
    const int o = __builtin_amdgcn_readfirstlane(S.col_row[j]);
    if (o < 0) { p.sink = j; return; }
    p.i = o;
}

// The end of the path from `cur`: the dual update and the augmentation (nothing if the counted loop ran out before the path
// ended).  ncols: the number of columns, the bound of the walk back.  On return the LDS writes are ordered for the whole wave.
template <int NC>
__device__ __forceinline__ void aw_finish(const AssignWave& S, const AwPath& p, double (&v)[NC], int cur, int ncols, int wl) {
    if (p.sink != -2 && p.drow >= 0) {
        // duals: scanned columns and the rows that hold them move by what the path still had to go; the root by all of it
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if ((p.sc >> c) & 1u) {
                const double d = p.minval - p.sp[c];
                v[c] = v[c] - d;
                const int o = S.col_row[NC * wl + c];
                if (o >= 0) S.row_dual[o] = S.row_dual[o] + d;
            }
        }
        if (wl == 0) S.row_dual[cur] = S.row_dual[cur] + p.minval;
        AW_WSYNC();
        // augment back along the predecessors (every lane walks the same path and writes the same values)
        int j = p.sink, r = -1;
        if (p.sink == -1) { r = p.drow; j = S.row_col[r]; S.row_col[r] = -1; }
        for (int g = 0; g <= ncols && r != cur && j >= 0; ++g) {
            r = S.pred[j];
            S.col_row[j] = r;
            const int t = S.row_col[r];
            S.row_col[r] = j;
            j = t;
        }
        AW_WSYNC();
    }
}
