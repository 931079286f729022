// Tracking of the kept 3D boxes across frames (include/rtm3d_hip.h, "tracking"): a constant-velocity Kalman filter per object
// and a greedy association of this frame's detections to the live tracks, per stream, on the device.
//   track_affinity_kernel   one lane per (track slot, record slot) pair of every stream: the track's predicted box against the
//                           detection's, affinity written to the workspace, -infinity where the pair is no candidate;
//   track_step_kernel       one workgroup per stream: predict, match, update, deaths, births, ids.
// Both kernels predict through ONE function (trk_predict_pose) and the translation unit is compiled with -ffp-contract=off, so the
// box the affinity was computed for is bit for bit the predicted state the update starts from.
// The match is the sequential global greedy one computed in rounds of mutual best.  Order the candidate pairs by (affinity
// descending, track slot ascending, record slot ascending).  A track's best remaining pair (largest affinity, lowest record slot)
// is the first of its row in that order, a detection's best (largest affinity, lowest track slot) the first of its column; a
// pair that is both precedes every remaining pair that shares its row or column, so the sequential rule takes it before anything
// can block it, and taking it removes exactly its row and column.  Every round with a candidate left matches at least the first
// pair of the whole order, so the rounds end.  Candidates are kept as two LDS bit matrices (rows, columns); the fp64 affinities
// stay in the workspace and are read for set bits only.
// The OPTIMAL match (step 3b; track_step_kernel<1>, reached only through rtm3d_tracks_update_assign) replaces the rounds by
// shortest augmenting paths over the same candidates, gain = affinity - thresh: the one-wave solver of assign_wave.h, which states
// the method, the tie rule (the lowest record slot at equal slack, "stay unmatched" at a tie with it) and why nothing depends on
// the order in which lanes retire.  Lane L owns the record slots 4L .. 4L + 3.  What is the tracker's own: the rows are the live
// slots with a candidate, in slot order (at most T augmentations of at most topk + 1 path steps each), and a row's gains come from
// the LDS candidate bits and the workspace, the next root's row fetched behind the current path.
#include "common.h"
#include "../../include/rtm3d_hip.h"
#include "box_geom.h"
#include "assign_wave.h"

#define TRK_MAX 256                 // track slots per stream and record slots per image, at most
#define TRK_HDR RTM3D_TRACK_HEADER_DOUBLES
#define TRK_SLOT RTM3D_TRACK_SLOT_DOUBLES
#define TRK_PI 3.141592653589793
#define TRK_TWO_PI 6.283185307179586
#define TRK_HALF_PI 1.5707963267948966
#define TRK_NEG_INF (-__builtin_inf())

__device__ __forceinline__ double trk_wrap(double a) { return a - TRK_TWO_PI * floor((a + TRK_PI) / TRK_TWO_PI); }

struct TrkPose { double X, Y, Z, ry, vx, vy, vz; };

// position, heading and velocity of a stored slot `s` one step of dt later, in the current frame's camera coordinates
__device__ __forceinline__ TrkPose trk_predict_pose(const double* __restrict__ s, double dt, const double* __restrict__ ego) {
    TrkPose p;
    p.vx = s[14]; p.vy = s[15]; p.vz = s[16];
    p.X = s[10] + dt * p.vx; p.Y = s[11] + dt * p.vy; p.Z = s[12] + dt * p.vz;
    p.ry = s[13];
    if (ego) {
        const double x = p.X, y = p.Y, z = p.Z, vx = p.vx, vy = p.vy, vz = p.vz;
        p.X = ((ego[0] * x + ego[1] * y) + ego[2] * z) + ego[3];
        p.Y = ((ego[4] * x + ego[5] * y) + ego[6] * z) + ego[7];
        p.Z = ((ego[8] * x + ego[9] * y) + ego[10] * z) + ego[11];
        p.vx = (ego[0] * vx + ego[1] * vy) + ego[2] * vz;
        p.vy = (ego[4] * vx + ego[5] * vy) + ego[6] * vz;
        p.vz = (ego[8] * vx + ego[9] * vy) + ego[10] * vz;
        const double c = cos(p.ry), sn = sin(p.ry);           // heading vector (c, 0, -sn)
        const double hx = ego[0] * c - ego[2] * sn, hz = ego[8] * c - ego[10] * sn;
        p.ry = atan2(-hz, hx);
    }
    p.ry = trk_wrap(p.ry);
    return p;
}

__device__ __forceinline__ bool trk_is_detection(const float* __restrict__ r, double min_score) {
    return r[31] == 2.0f && (double)r[1] >= min_score;
}

__global__ __launch_bounds__(BO_LANES) void track_affinity_kernel(long long total, int topk, int T, const float* __restrict__ rec, double dt,
                                                                 const double* __restrict__ ego, rtm3d_track_params P,
                                                                 const double* __restrict__ state, double* __restrict__ aff) {
    __shared__ double2 poly[2][BO_MAXV][BO_LANES];
    const int lane = threadIdx.x;
    const long long t = (long long)blockIdx.x * BO_LANES + lane;
    if (t >= total) return;
    const int per = T * topk;
    const int b = (int)(t / per);
    const int r = (int)(t - (long long)b * per);
    const int ts = r / topk, k = r - ts * topk;
    const double* s = state + (size_t)b * (TRK_HDR + TRK_SLOT * T) + TRK_HDR + (size_t)ts * TRK_SLOT;
    const float* rr = rec + ((size_t)b * topk + k) * 32;
    double out = TRK_NEG_INF;
    if (s[0] != 0.0 && trk_is_detection(rr, P.min_score) && !(P.class_aware && s[1] != (double)rr[0])) {
        const TrkPose p = trk_predict_pose(s, dt, ego ? ego + (size_t)b * 12 : nullptr);
        const double dh = (double)rr[24], dw = (double)rr[25], dl = (double)rr[26], dX = (double)rr[27], dY = (double)rr[28],
                     dZ = (double)rr[29], dry = (double)rr[30];
        const double ex = p.X - dX, ey = p.Y - dY, ez = p.Z - dZ;
        double a;
        if (P.metric == 2) {
            a = -sqrt((ex * ex + ey * ey) + ez * ez);
        } else {
            // footprints whose centres lie further apart than their two half diagonals cannot meet: 0 without clipping
            const double reach = 0.5 * sqrt(s[8] * s[8] + s[9] * s[9]) + 0.5 * sqrt(dw * dw + dl * dl);
            a = 0.0;
            if (!(ex * ex + ez * ez > reach * reach)) {
                const BoxP ba = box_prepare(s[7], s[8], s[9], p.X, p.Y, p.Z, p.ry);
                const BoxP bb = box_prepare(dh, dw, dl, dX, dY, dZ, dry);
                double inter, ov;
                box_pair(ba, bb, poly[0], poly[1], lane, inter, ov);
                a = P.metric == 0 ? overlap_ratio(inter, ba.area, bb.area, 0) : overlap_ratio(inter * ov, ba.area * ba.h, bb.area * bb.h, 0);
            }
        }
        if (a > P.thresh) out = a;
    }
    aff[t] = out;
}

// ASSIGN: RTM3D_TRACK_ASSIGN_GREEDY (step 3) or RTM3D_TRACK_ASSIGN_OPTIMAL (step 3b); everything else is one code
template <int ASSIGN>
__global__ __launch_bounds__(BO_LANES) void track_step_kernel(int topk, int T, const float* __restrict__ rec, double dt,
                                                             const double* __restrict__ ego, rtm3d_track_params P,
                                                             double* __restrict__ state, int32_t* __restrict__ ids,
                                                             const double* __restrict__ aff) {
    constexpr bool OPT = ASSIGN == RTM3D_TRACK_ASSIGN_OPTIMAL;
    __shared__ uint32_t rowmask[TRK_MAX][TRK_MAX / 32];       // [track slot]: candidate record slots
    __shared__ uint32_t colmask[OPT ? 1 : TRK_MAX][TRK_MAX / 32];   // [record slot]: candidate track slots (greedy only)
    __shared__ double row_dual[OPT ? TRK_MAX : 1];            // optimal only: [track slot] dual of the row
    __shared__ int trk_det[OPT ? TRK_MAX : 1];                //   track slot -> record slot it holds, -1 none
    __shared__ int pred[OPT ? TRK_MAX : 1];                   //   record slot -> the row its slack came from, this path
    __shared__ unsigned long long rowsel[OPT ? BO_LANES / 64 : 1];   //   the rows: live slots with a candidate
    __shared__ uint32_t det_free[TRK_MAX / 32], trk_free[TRK_MAX / 32];
    __shared__ int cbest[TRK_MAX];
    __shared__ int det_owner[TRK_MAX];                        // record slot -> track slot (match or birth), -1 none
    __shared__ int birth_det[TRK_MAX];                        // track slot -> record slot born into it, -1 none
    __shared__ int birth_rank[TRK_MAX];
    __shared__ int freelist[TRK_MAX];
    __shared__ int sid[TRK_MAX];                              // track slot -> signed id of this frame
    __shared__ int wave_births[BO_LANES / 64], wave_frees[BO_LANES / 64];
    const int tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
    const int b = blockIdx.x;
    double* hdr = state + (size_t)b * (TRK_HDR + TRK_SLOT * T);
    double* s = hdr + TRK_HDR + (size_t)tid * TRK_SLOT;
    const float* r_img = rec + (size_t)b * topk * 32;
    const double* A = aff + (size_t)b * T * topk;
    if (ego) ego += (size_t)b * 12;
    const double issued = hdr[0], frame = hdr[1] + 1.0, dropped = hdr[2];

#pragma unroll
    for (int w = 0; w < TRK_MAX / 32; ++w) { rowmask[tid][w] = 0u; if constexpr (!OPT) colmask[tid][w] = 0u; }
    if (tid < TRK_MAX / 32) { det_free[tid] = 0xffffffffu; trk_free[tid] = 0xffffffffu; }
    det_owner[tid] = -1; birth_det[tid] = -1; sid[tid] = 0;
    __syncthreads();

    // the slot of this lane, predicted
    const bool live = tid < T && s[0] != 0.0;
    double id = 0.0, cls = 0.0, age = 0.0, hits = 0.0, misses = 0.0, score = 0.0, slot = 0.0;
    double h = 0.0, w = 0.0, l = 0.0, Ppp = 0.0, Ppv = 0.0, Pvv = 0.0, Pry = 0.0, Pd = 0.0;
    TrkPose p;
    p.X = p.Y = p.Z = p.ry = p.vx = p.vy = p.vz = 0.0;
    if (live) {
        id = s[0]; cls = s[1]; age = s[2] + 1.0; hits = s[3]; misses = s[4]; score = s[5]; slot = -1.0;
        h = s[7]; w = s[8]; l = s[9];
        p = trk_predict_pose(s, dt, ego);
        const double a = s[17] + dt * s[18], bq = s[18] + dt * s[19];
        Ppp = (a + dt * bq) + P.q_pos * dt;
        Ppv = bq;
        Pvv = s[19] + P.q_vel * dt;
        Pry = s[20] + P.q_ry * dt;
        Pd = s[21] + P.q_dim * dt;
    }
    const bool isdet = tid < topk && trk_is_detection(r_img + (size_t)tid * 32, P.min_score);

    // candidate bit matrices from the affinity matrix
    const int npairs = T * topk;
    for (int q = tid; q < npairs; q += BO_LANES) {
        if (A[q] > TRK_NEG_INF) {
            const int t = q / topk, k = q - t * topk;
            atomicOr(&rowmask[t][k >> 5], 1u << (k & 31));
            if constexpr (!OPT) atomicOr(&colmask[k][t >> 5], 1u << (t & 31));
        }
    }
    __syncthreads();

    int match = -1;
    if constexpr (!OPT) {
        // rounds of mutual best
        for (;;) {
            int rb = -1;
            if (live && match < 0) {
                double rv = TRK_NEG_INF;
                for (int wd = 0; wd < TRK_MAX / 32; ++wd) {
                    uint32_t m = rowmask[tid][wd] & det_free[wd];
                    while (m) {
                        const int k = wd * 32 + __ffs(m) - 1;
                        m &= m - 1u;
                        const double v = A[(size_t)tid * topk + k];
                        if (v > rv) { rv = v; rb = k; }
                    }
                }
            }
            int cb = -1;
            if (isdet && det_owner[tid] < 0) {
                double cv = TRK_NEG_INF;
                for (int wd = 0; wd < TRK_MAX / 32; ++wd) {
                    uint32_t m = colmask[tid][wd] & trk_free[wd];
                    while (m) {
                        const int t = wd * 32 + __ffs(m) - 1;
                        m &= m - 1u;
                        const double v = A[(size_t)t * topk + tid];
                        if (v > cv) { cv = v; cb = t; }
                    }
                }
            }
            cbest[tid] = cb;
            __syncthreads();
            if (rb >= 0 && cbest[rb] == tid) {
                match = rb;
                det_owner[rb] = tid;
                atomicAnd(&det_free[rb >> 5], ~(1u << (rb & 31)));
                atomicAnd(&trk_free[tid >> 5], ~(1u << (tid & 31)));
            }
            if (!__syncthreads_or(rb >= 0 ? 1 : 0)) break;
        }
    } else {
        // shortest augmenting paths by wave 0 (assign_wave.h); lane wl owns the record slots 4 * wl + c, c = 0 .. 3
        bool has = false;
#pragma unroll
        for (int wd = 0; wd < TRK_MAX / 32; ++wd) has = has || rowmask[tid][wd] != 0u;
        const unsigned long long hb = __ballot(has);
        if (wl == 0) rowsel[wave] = hb;
        row_dual[tid] = 0.0; trk_det[tid] = -1;
        __syncthreads();
        if (wave == 0) {
            unsigned long long rs[BO_LANES / 64];
#pragma unroll
            for (int wv = 0; wv < BO_LANES / 64; ++wv) rs[wv] = rowsel[wv];
            auto pop_row = [&]() -> int {                         // the next row in slot order, -1 when there is none
                int r = -1;
#pragma unroll
                for (int wv = 0; wv < BO_LANES / 64; ++wv)
                    if (r < 0 && rs[wv]) { r = 64 * wv + __ffsll(rs[wv]) - 1; rs[wv] &= rs[wv] - 1ull; }
                return r;
            };
            // the candidate bits of this lane's four columns in row i and their affinities (read for set bits only)
            auto load_row = [&](int i, double (&a)[4], uint32_t& nib) {
                nib = (rowmask[i][wl >> 3] >> ((wl & 7) * 4)) & 0xfu;
                const double* Ai = A + (size_t)i * topk + 4 * wl;
#pragma unroll
                for (int c = 0; c < 4; ++c) a[c] = (nib >> c) & 1u ? Ai[c] : 0.0;
            };
            const AssignWave st{row_dual, trk_det, det_owner, pred};
            double v[4] = {0.0, 0.0, 0.0, 0.0};                   // column duals
            double an[4] = {0.0, 0.0, 0.0, 0.0};
            uint32_t nibn = 0u;
            int next = pop_row();
            if (next >= 0) load_row(next, an, nibn);
            for (int n = 0; n < T && next >= 0; ++n) {            // one augmentation per row: at most T
                const int cur = next;
                double a[4] = {an[0], an[1], an[2], an[3]};
                uint32_t nib = nibn;
                next = pop_row();
                if (next >= 0) load_row(next, an, nibn);          // the next root's row is fetched behind this path
                // a set bit of nib is a pair whose affinity is above thresh (track_affinity_kernel): a candidate, its gain > 0
                const auto gain = [&](int c, double& g) { g = a[c] - P.thresh; return true; };
                AwPath p = aw_path(cur);
                for (int step = 0; step <= topk; ++step) {        // every step scans another matched row or ends: at most topk + 1
                    aw_step<4>(st, p, v, wl, nib, gain);
                    if (p.sink != -2) break;
                    load_row(p.i, a, nib);
                }
                aw_finish<4>(st, p, v, cur, topk, wl);
            }
        }
        __syncthreads();
        match = trk_det[tid];
    }

    // update of matched tracks, misses and deaths of the others
    bool now_live = live;
    if (live && match >= 0) {
        const float* rr = r_img + (size_t)match * 32;
        const double zh = (double)rr[24], zw = (double)rr[25], zl = (double)rr[26], zX = (double)rr[27], zY = (double)rr[28],
                     zZ = (double)rr[29], zry = trk_wrap((double)rr[30]);
        const double S = Ppp + P.r_pos, Kp = Ppp / S, Kv = Ppv / S;
        const double yx = zX - p.X, yy = zY - p.Y, yz = zZ - p.Z;
        p.X = p.X + Kp * yx; p.Y = p.Y + Kp * yy; p.Z = p.Z + Kp * yz;
        p.vx = p.vx + Kv * yx; p.vy = p.vy + Kv * yy; p.vz = p.vz + Kv * yz;
        const double npp = Ppp - Kp * Ppp, npv = Ppv - Kp * Ppv, nvv = Pvv - Kv * Ppv;
        Ppp = npp; Ppv = npv; Pvv = nvv;
        if (fabs(trk_wrap(zry - p.ry)) > TRK_HALF_PI) p.ry = trk_wrap(p.ry + TRK_PI);
        const double yr = trk_wrap(zry - p.ry), Kr = Pry / (Pry + P.r_ry);
        p.ry = trk_wrap(p.ry + Kr * yr);
        Pry = Pry - Kr * Pry;
        const double Kd = Pd / (Pd + P.r_dim);
        h = h + Kd * (zh - h); w = w + Kd * (zw - w); l = l + Kd * (zl - l);
        Pd = Pd - Kd * Pd;
        hits = hits + 1.0; misses = 0.0; score = (double)rr[1]; slot = (double)match;
    } else if (live) {
        hits = 0.0; misses = misses + 1.0;
        if (misses > (double)P.max_misses) now_live = false;
    }

    // births: the unmatched detections in slot order into the free slots in slot order
    const bool wants = isdet && det_owner[tid] < 0;
    const bool is_free = tid < T && !now_live;
    const unsigned long long bal_b = __ballot(wants), bal_f = __ballot(is_free);
    if (wl == 0) { wave_births[wave] = __popcll(bal_b); wave_frees[wave] = __popcll(bal_f); }
    __syncthreads();
    int base_b = 0, base_f = 0, nb = 0, nf = 0;
#pragma unroll
    for (int wv = 0; wv < BO_LANES / 64; ++wv) {
        if (wv < wave) { base_b += wave_births[wv]; base_f += wave_frees[wv]; }
        nb += wave_births[wv]; nf += wave_frees[wv];
    }
    const unsigned long long below = (1ull << wl) - 1ull;
    if (is_free) freelist[base_f + __popcll(bal_f & below)] = tid;
    __syncthreads();
    if (wants) {
        const int rank = base_b + __popcll(bal_b & below);
        if (rank < nf) {
            const int t = freelist[rank];
            birth_det[t] = tid;
            birth_rank[t] = rank;
            det_owner[tid] = t;
        }
    }
    __syncthreads();
    if (tid < T) {
        const int k = birth_det[tid];
        if (k >= 0) {
            const float* rr = r_img + (size_t)k * 32;
            now_live = true;
            id = issued + (double)(birth_rank[tid] + 1);
            cls = (double)rr[0]; age = 1.0; hits = 1.0; misses = 0.0; score = (double)rr[1]; slot = (double)k;
            h = (double)rr[24]; w = (double)rr[25]; l = (double)rr[26];
            p.X = (double)rr[27]; p.Y = (double)rr[28]; p.Z = (double)rr[29]; p.ry = trk_wrap((double)rr[30]);
            p.vx = 0.0; p.vy = 0.0; p.vz = 0.0;
            Ppp = P.p0_pos; Ppv = 0.0; Pvv = P.p0_vel; Pry = P.p0_ry; Pd = P.p0_dim;
        }
        if (now_live) {
            s[0] = id; s[1] = cls; s[2] = age; s[3] = hits; s[4] = misses; s[5] = score; s[6] = slot;
            s[7] = h; s[8] = w; s[9] = l; s[10] = p.X; s[11] = p.Y; s[12] = p.Z; s[13] = p.ry;
            s[14] = p.vx; s[15] = p.vy; s[16] = p.vz; s[17] = Ppp; s[18] = Ppv; s[19] = Pvv; s[20] = Pry; s[21] = Pd;
            s[22] = 0.0; s[23] = 0.0;
            if (slot >= 0.0) {
                const bool confirmed = hits >= (double)P.min_hits || frame <= (double)P.min_hits;
                sid[tid] = confirmed ? (int)id : -(int)id;
            }
        } else if (live) {
#pragma unroll
            for (int e = 0; e < TRK_SLOT; ++e) s[e] = 0.0;
        }
    }
    if (tid == 0) {
        const int born = nb < nf ? nb : nf;
        hdr[0] = issued + (double)born;
        hdr[1] = frame;
        hdr[2] = dropped + (double)(nb - born);
    }
    __syncthreads();
    if (tid < topk) {
        const int t = det_owner[tid];
        ids[(size_t)b * topk + tid] = t >= 0 ? sid[t] : 0;
    }
}

extern void rt_set_error(const char* fmt, ...);

extern "C" int rtm3d_track_default_params(rtm3d_track_params* p) {
    if (!p) { rt_set_error("track_default_params: null pointer"); return 1; }
    p->metric = 1; p->class_aware = 0; p->max_misses = 2; p->min_hits = 3;
    p->thresh = 0.01; p->min_score = 0.0;
    p->p0_pos = 10.0; p->p0_vel = 1e4; p->p0_ry = 10.0; p->p0_dim = 10.0;
    p->q_pos = 0.0; p->q_vel = 0.01; p->q_ry = 0.0; p->q_dim = 0.0;
    p->r_pos = 1.0; p->r_ry = 1.0; p->r_dim = 1.0;
    return 0;
}

extern "C" size_t rtm3d_tracks_state_bytes(int B, int T) {
    if (B <= 0 || T < 1 || T > TRK_MAX) return 0;
    return (size_t)B * (TRK_HDR + (size_t)TRK_SLOT * T) * sizeof(double);
}

extern "C" size_t rtm3d_tracks_workspace_bytes(int B, int topk, int T) {
    if (B <= 0 || T < 1 || T > TRK_MAX || topk < 1 || topk > TRK_MAX) return 0;
    return (size_t)B * T * topk * sizeof(double);
}

static bool trk_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }

static int trk_update(void* stream, int B, int topk, int T, const float* d_rec, double dt, const double* d_ego,
                      const rtm3d_track_params* params, int assign, double* d_state, int32_t* d_ids, void* d_ws) {
    if (B <= 0) { rt_set_error("tracks_update: bad batch size B %d", B); return 1; }
    if (T < 1 || T > TRK_MAX) { rt_set_error("tracks_update: T %d track slots per stream (1..%d)", T, TRK_MAX); return 1; }
    if (topk < 1 || topk > TRK_MAX) { rt_set_error("tracks_update: topk %d record slots per image (1..%d)", topk, TRK_MAX); return 1; }
    if (!(dt > 0.0) || !(dt < __builtin_inf())) { rt_set_error("tracks_update: dt %g must be positive and finite", dt); return 1; }
    if (!params) { rt_set_error("tracks_update: params is NULL"); return 1; }
    if (!d_rec || !d_state || !d_ids || !d_ws) { rt_set_error("tracks_update: null pointer (d_rec, d_state, d_ids and d_ws are required)"); return 1; }
    const rtm3d_track_params& P = *params;
    if (P.metric < 0 || P.metric > 2) { rt_set_error("tracks_update: unknown metric %d (0 BEV IoU, 1 3D IoU, 2 centre distance)", P.metric); return 1; }
    if (P.max_misses < 0 || P.min_hits < 0) { rt_set_error("tracks_update: max_misses %d / min_hits %d must not be negative", P.max_misses, P.min_hits); return 1; }
    if (P.thresh != P.thresh || P.min_score != P.min_score) { rt_set_error("tracks_update: thresh or min_score is NaN"); return 1; }
    if (!trk_nonneg(P.p0_pos) || !trk_nonneg(P.p0_vel) || !trk_nonneg(P.p0_ry) || !trk_nonneg(P.p0_dim) || !trk_nonneg(P.q_pos) ||
        !trk_nonneg(P.q_vel) || !trk_nonneg(P.q_ry) || !trk_nonneg(P.q_dim)) {
        rt_set_error("tracks_update: initial variances and process noise must be finite and not negative"); return 1;
    }
    if (!(P.r_pos > 0.0) || !(P.r_ry > 0.0) || !(P.r_dim > 0.0) || !trk_nonneg(P.r_pos) || !trk_nonneg(P.r_ry) || !trk_nonneg(P.r_dim)) {
        rt_set_error("tracks_update: measurement noise must be positive and finite"); return 1;
    }
    if (assign == RTM3D_TRACK_ASSIGN_OPTIMAL && !(P.thresh > -__builtin_inf() && P.thresh < __builtin_inf())) {
        rt_set_error("tracks_update_assign: the optimal assignment needs a finite thresh (gain = affinity - thresh), got %g", P.thresh); return 1;
    }
    const long long total = (long long)B * T * topk;
    const long long blocks = (total + BO_LANES - 1) / BO_LANES;
    if (blocks > 0x7fffffffLL) { rt_set_error("tracks_update: %lld pairs are more than one launch holds", total); return 1; }
    hipLaunchKernelGGL(track_affinity_kernel, dim3((unsigned)blocks), dim3(BO_LANES), 0, (hipStream_t)stream, total, topk, T, d_rec, dt, d_ego, P,
                       (const double*)d_state, (double*)d_ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("tracks_update affinity launch: %s", hipGetErrorString(e)); return 1; }
    if (assign == RTM3D_TRACK_ASSIGN_OPTIMAL)
        hipLaunchKernelGGL(track_step_kernel<RTM3D_TRACK_ASSIGN_OPTIMAL>, dim3(B), dim3(BO_LANES), 0, (hipStream_t)stream, topk, T, d_rec, dt, d_ego,
                           P, d_state, d_ids, (const double*)d_ws);
    else
        hipLaunchKernelGGL(track_step_kernel<RTM3D_TRACK_ASSIGN_GREEDY>, dim3(B), dim3(BO_LANES), 0, (hipStream_t)stream, topk, T, d_rec, dt, d_ego,
                           P, d_state, d_ids, (const double*)d_ws);
    e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("tracks_update step launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int rtm3d_tracks_update(void* stream, int B, int topk, int T, const float* d_rec, double dt, const double* d_ego,
                                   const rtm3d_track_params* params, double* d_state, int32_t* d_ids, void* d_ws) {
    return trk_update(stream, B, topk, T, d_rec, dt, d_ego, params, RTM3D_TRACK_ASSIGN_GREEDY, d_state, d_ids, d_ws);
}

extern "C" int rtm3d_tracks_update_assign(void* stream, int B, int topk, int T, const float* d_rec, double dt, const double* d_ego,
                                          const rtm3d_track_params* params, int assign, double* d_state, int32_t* d_ids, void* d_ws) {
    if (assign != RTM3D_TRACK_ASSIGN_GREEDY && assign != RTM3D_TRACK_ASSIGN_OPTIMAL) {
        rt_set_error("tracks_update_assign: unknown assign %d (0 greedy, 1 optimal)", assign); return 1;
    }
    return trk_update(stream, B, topk, T, d_rec, dt, d_ego, params, assign, d_state, d_ids, d_ws);
}
