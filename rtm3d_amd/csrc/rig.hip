// Fusion of the kept 3D boxes of the C cameras of a rig into one set of boxes in the rig frame (include/rtm3d_hip.h, "rig
// fusion"): extrinsics, a score order, greedy clusters round representatives, a weighted merge, and the map back from every
// camera's record slot to the fused slot.  Three launches per rtm3d_rig_fuse, all into / out of the caller's workspace:
//   rig_prepare_kernel   one workgroup per rig: the candidates' keys (score descending by the fp32 compare, camera, slot) packed
//                        and sorted in LDS (bitonic over the candidates only; the keys are distinct, so the order is the rule's
//                        and no tie is left to the network), then every candidate's box taken to the rig frame and stored BY ITS
//                        POSITION in that order, with its half footprint diagonal (its term of `reach`);
//   rig_link_kernel      grid-wide, one lane per pair (position i, position j < i), one wave per row i of the `linked` matrix,
//                        64-bit word after word: a word is the wave's ballot, written by one lane - no atomics, every word the
//                        scan reads is rewritten by every call.  The affinity is the tracker's (box j as box a, box i as box b),
//                        its `reach` shortcut included, so almost no pair is clipped;
//   rig_cluster_kernel   one workgroup per rig: the sequential representative scan over the bit rows in chunks of 64 positions
//                        (wave 0 settles a chunk in rounds - a lane once all lanes it is linked to are settled - then every lane
//                        pushes the chunk's representatives to the later rows it owns, whose words were fetched a chunk ahead),
//                        the output slots by prefix popcount, the map, and one lane per output slot for the ordered merge sums.
// Nothing depends on the order in which lanes or atomics retire (there are no atomics): a row, an output slot and a map entry have
// one owner each.  The translation unit is compiled with -ffp-contract=off (Makefile), like track.hip.
#include "common.h"
#include "../../include/rtm3d_hip.h"
#include "box_geom.h"

#define RIG_MAX_N 2048              // record slots of one rig, C * topk, at most
#define RIG_MAX_C 16
#define RIG_MAX_TOPK 256
#define RIG_MAX_CAP 256
#define RIG_MAX_W (RIG_MAX_N / 64)  // 64-bit words of a row of the linked matrix, at most
#define RIG_PI 3.141592653589793
#define RIG_TWO_PI 6.283185307179586
#define RIG_HALF_PI 1.5707963267948966
#define RIG_NO_CAND 0xffffffffu     // high word of the key of a slot that is no candidate (no candidate's: see rig_key)

__device__ __forceinline__ double rig_wrap(double a) { return a - RIG_TWO_PI * floor((a + RIG_PI) / RIG_TWO_PI); }

// The workspace of one rig, in 8-byte units: [0] n (int32, the number of candidates) | order [N] int32: position -> record slot
// q = camera * topk + slot | cls [N] fp32 | score [N] fp32 | box [N][8] fp64: the box in the rig frame and [7] = its half footprint
// diagonal 0.5 * sqrt(w * w + l * l), the box's term of `reach` | link [N][W] 64-bit words.
struct RigWs {
    int32_t* n; int32_t* order; float* cls; float* score; double* box; unsigned long long* link;
};
__host__ __device__ __forceinline__ size_t rig_half(int N) { return (size_t)(N + 1) / 2; }
__host__ __device__ __forceinline__ size_t rig_ws_units(int N) { return 2 + 3 * rig_half(N) + (size_t)8 * N + (size_t)N * ((N + 63) / 64); }
__device__ __forceinline__ RigWs rig_ws(void* ws, int r, int N) {
    unsigned long long* base = (unsigned long long*)ws + (size_t)r * rig_ws_units(N);
    RigWs w;
    w.n = (int32_t*)base;
    w.order = (int32_t*)(base + 2);
    w.cls = (float*)(base + 2 + rig_half(N));
    w.score = (float*)(base + 2 + 2 * rig_half(N));
    w.box = (double*)(base + 2 + 3 * rig_half(N));
    w.link = base + 2 + 3 * rig_half(N) + (size_t)8 * N;
    return w;
}

// ascending 64-bit key of record slot q: score descending by the fp32 compare (-0 == +0), then q = camera * topk + slot ascending
__device__ __forceinline__ unsigned long long rig_key(const float* __restrict__ r, int q, double min_score) {
    const float s = r[1];
    if (!(r[31] == 2.0f && (double)s >= min_score)) return ((unsigned long long)RIG_NO_CAND << 32) | (unsigned)q;
    uint32_t u = s == 0.0f ? 0u : __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // ascending in the score; 0 only for a NaN, which is no candidate
    return ((unsigned long long)(~u) << 32) | (unsigned)q;
}

__global__ __launch_bounds__(BO_LANES) void rig_prepare_kernel(int C, int topk, const float* __restrict__ rec, const double* __restrict__ ext,
                                                              rtm3d_rig_params P, void* __restrict__ ws) {
    constexpr int ROUNDS = RIG_MAX_N / BO_LANES, WAVES = BO_LANES / 64;
    __shared__ unsigned long long key[RIG_MAX_N];
    __shared__ int wave_cnt[ROUNDS][WAVES], wave_off[ROUNDS][WAVES];
    __shared__ int n_sh;
    const int tid = threadIdx.x, wave = tid >> 6, wl = tid & 63, r = blockIdx.x, N = C * topk;
    const float* rr = rec + (size_t)r * N * 32;
    // the candidates' keys, packed to the front of the LDS array in slot order (any order would do: the keys are distinct)
    unsigned long long k[ROUNDS], bal[ROUNDS];
#pragma unroll
    for (int m = 0; m < ROUNDS; ++m) {
        const int q = tid + BO_LANES * m;
        k[m] = q < N ? rig_key(rr + (size_t)q * 32, q, P.min_score) : ~0ull;
        bal[m] = __ballot((uint32_t)(k[m] >> 32) != RIG_NO_CAND);
        if (wl == 0) wave_cnt[m][wave] = __popcll(bal[m]);
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int m = 0; m < ROUNDS; ++m)
            for (int wv = 0; wv < WAVES; ++wv) { wave_off[m][wv] = acc; acc += wave_cnt[m][wv]; }
        n_sh = acc;
    }
    __syncthreads();
    const int n = n_sh;
    int M = 64;
    while (M < n) M <<= 1;
#pragma unroll
    for (int m = 0; m < ROUNDS; ++m)
        if ((bal[m] >> wl) & 1ull) key[wave_off[m][wave] + __popcll(bal[m] & ((1ull << wl) - 1ull))] = k[m];
    for (int p = n + tid; p < M; p += BO_LANES) key[p] = ~0ull;
    __syncthreads();
    // bitonic network over M keys, one lane per pair (i, i | j).  The pairs of 64 consecutive t lie, for every j <= 32, in one
    // aligned block of 128 keys that no other wave touches in those stages: the stages j = 32 .. 1 of a merge run inside the wave,
    // in the order of its LDS instructions, and only the stages with j >= 64 and the end of a merge need the workgroup's barrier
    const auto exchange = [&](int t, int j, int kk) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;
        const unsigned long long a = key[i], b = key[o];
        if ((a > b) == ((i & kk) == 0)) { key[i] = b; key[o] = a; }
    };
    for (int kk = 2; kk <= M; kk <<= 1) {
        int j = kk >> 1;
        for (; j >= 64; j >>= 1) {
            for (int t = tid; t < (M >> 1); t += BO_LANES) exchange(t, j, kk);
            __syncthreads();
        }
        for (int t = tid; t < (M >> 1); t += BO_LANES) {
            for (int jj = j; jj > 0; jj >>= 1) {
                exchange(t, jj, kk);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        __syncthreads();
    }
    const RigWs w = rig_ws(ws, r, N);
    if (tid == 0) { w.n[0] = n; w.n[1] = 0; }
    for (int p = tid; p < n; p += BO_LANES) {
        const int q = (int)(uint32_t)key[p];
        const float* s = rr + (size_t)q * 32;
        const double* e = ext + ((size_t)r * C + q / topk) * 12;
        const double x = (double)s[27], y = (double)s[28], z = (double)s[29], ry = (double)s[30];
        const double c = cos(ry), sn = sin(ry);               // heading vector (c, 0, -sn), turned like the tracker's
        const double bw = (double)s[25], bl = (double)s[26];
        double* b = w.box + (size_t)p * 8;
        b[0] = (double)s[24]; b[1] = bw; b[2] = bl;
        b[3] = ((e[0] * x + e[1] * y) + e[2] * z) + e[3];
        b[4] = ((e[4] * x + e[5] * y) + e[6] * z) + e[7];
        b[5] = ((e[8] * x + e[9] * y) + e[10] * z) + e[11];
        b[6] = rig_wrap(atan2(-(e[8] * c - e[10] * sn), e[0] * c - e[2] * sn));
        b[7] = 0.5 * sqrt(bw * bw + bl * bl);
        w.order[p] = q;
        w.cls[p] = s[0];
        w.score[p] = s[1];
    }
}

// one wave per (rig, row i) of the linked matrix, word after word: lane = column j = 64 * wd + lane, the words with 64 * wd <= i
__global__ __launch_bounds__(BO_LANES) void rig_link_kernel(long long rows, int N, int topk, rtm3d_rig_params P, void* __restrict__ ws) {
    __shared__ double2 poly[2][BO_MAXV][BO_LANES];
    const int lane = threadIdx.x, wl = lane & 63;
    const long long g = (long long)blockIdx.x * (BO_LANES / 64) + (lane >> 6);
    if (g >= rows) return;
    const int W = (N + 63) / 64;
    const int r = (int)(g / N);
    const int i = (int)(g - (long long)r * N);
    const RigWs w = rig_ws(ws, r, N);
    if (i >= w.n[0]) return;                                  // wave-uniform
    const double* Bx = w.box + (size_t)i * 8;                 // box b: this row's
    const double bX = Bx[3], bY = Bx[4], bZ = Bx[5], bhalf = Bx[7];
    const BoxP bb = box_load(Bx);
    const int cam_i = w.order[i] / topk;
    const float cls_i = w.cls[i];
    for (int wd = 0; wd <= (i >> 6); ++wd) {
        const int j = 64 * wd + wl;
        bool linked = false;
        if (j < i) {
            linked = true;
            if (P.cross_only && cam_i == w.order[j] / topk) linked = false;
            if (P.class_aware && !(cls_i == w.cls[j])) linked = false;
        }
        if (linked) {
            const double* A = w.box + (size_t)j * 8;          // box a: the earlier one, the possible representative
            const double ex = A[3] - bX, ey = A[4] - bY, ez = A[5] - bZ;
            double a;
            if (P.metric == 2) {
                a = -sqrt((ex * ex + ey * ey) + ez * ez);
            } else {
                const double reach = A[7] + bhalf;
                a = 0.0;
                if (!(ex * ex + ez * ez > reach * reach)) {
                    const BoxP ba = box_load(A);
                    double inter, ov;
                    box_pair(ba, bb, poly[0], poly[1], lane, inter, ov);
                    a = P.metric == 0 ? overlap_ratio(inter, ba.area, bb.area, 0) : overlap_ratio(inter * ov, ba.area * ba.h, bb.area * bb.h, 0);
                }
            }
            linked = a > P.thresh;
        }
        const unsigned long long bal = __ballot(linked);
        if (wl == 0) w.link[(size_t)i * W + wd] = bal;
    }
}

__global__ __launch_bounds__(BO_LANES) void rig_cluster_kernel(int C, int topk, int cap, const float* __restrict__ rec, rtm3d_rig_params P,
                                                              float* __restrict__ out, double* __restrict__ obox, int32_t* __restrict__ info,
                                                              int32_t* __restrict__ map, int32_t* __restrict__ cnt, void* __restrict__ ws) {
    constexpr int ROUNDS = RIG_MAX_N / BO_LANES;
    __shared__ __attribute__((aligned(16))) int rep_of[RIG_MAX_N];   // position -> position of its representative (itself for one), -1 not yet
    __shared__ int lmap[RIG_MAX_N];                           // record slot q -> d_map
    __shared__ unsigned long long diag[RIG_MAX_N];            // position i -> word i / 64 of its row: the links inside its chunk
    __shared__ unsigned long long repmask[RIG_MAX_W];         // representatives by position
    __shared__ int prefix[RIG_MAX_W + 1];                     // representatives before word w
    __shared__ int rep_pos[RIG_MAX_CAP];                      // output slot -> position of its representative
    __shared__ int next_of[RIG_MAX_N];                        // position -> the next member of its cluster, -1 at the end
    const int tid = threadIdx.x, wl = tid & 63, r = blockIdx.x, N = C * topk, W = (N + 63) / 64;
    const RigWs w = rig_ws(ws, r, N);
    const int n = w.n[0], nch = (n + 63) >> 6;
    for (int q = tid; q < RIG_MAX_N; q += BO_LANES) { rep_of[q] = -1; lmap[q] = -1; }
    for (int i = tid; i < n; i += BO_LANES) diag[i] = w.link[(size_t)i * W + (i >> 6)];
    if (tid < RIG_MAX_W) repmask[tid] = 0ull;
    // the words of chunk c the later rows of this lane (i = tid + 256 m) will want, fetched one chunk ahead
    unsigned long long pw[ROUNDS];
    const auto fetch = [&](int c) {
#pragma unroll
        for (int m = 0; m < ROUNDS; ++m) {
            const int i = tid + BO_LANES * m;
            pw[m] = c < nch && i >= 64 * (c + 1) && i < n ? w.link[(size_t)i * W + c] : 0ull;
        }
    };
    fetch(0);
    __syncthreads();

    for (int c = 0; c < nch; ++c) {
        if (tid < 64) {
            // settle chunk c: position i is a representative iff no representative before it is linked to it.  A lane is settled
            // once every lane of the chunk it is linked to is; the lowest unsettled lane always is, so the rounds end (at most 64)
            const int i = 64 * c + wl;
            const bool open = i < n && rep_of[i] < 0;         // not taken by a representative of an earlier chunk
            const unsigned long long mine = open ? diag[i] & ((1ull << wl) - 1ull) : 0ull;
            unsigned long long settled = ~__ballot(open), reps = 0ull;
            while (~settled) {
                const bool ready = open && !((settled >> wl) & 1ull) && (mine & ~settled) == 0ull;
                const unsigned long long rb = __ballot(ready), pb = __ballot(ready && (mine & reps) == 0ull);
                reps |= pb;
                settled |= rb;
            }
            if (open) rep_of[i] = (reps >> wl) & 1ull ? i : 64 * c + __ffsll((long long)(mine & reps)) - 1;
            if (wl == 0) repmask[c] = reps;
        }
        __syncthreads();
        // push: the later rows this lane owns join the earliest representative of chunk c that is linked to them
        const unsigned long long reps = repmask[c];
#pragma unroll
        for (int m = 0; m < ROUNDS; ++m) {
            const unsigned long long x = pw[m] & reps;
            const int i = tid + BO_LANES * m;
            if (x && rep_of[i] < 0) rep_of[i] = 64 * c + __ffsll((long long)x) - 1;
        }
        fetch(c + 1);
        __syncthreads();
    }
    if (tid == 0) {
        int acc = 0;
        for (int c = 0; c < RIG_MAX_W; ++c) { prefix[c] = acc; acc += __popcll(repmask[c]); }
        prefix[RIG_MAX_W] = acc;
    }
    __syncthreads();
    const int ncl = prefix[RIG_MAX_W];
    for (int p = tid; p < n; p += BO_LANES) {
        const int j = rep_of[p];
        const int s = prefix[j >> 6] + __popcll(repmask[j >> 6] & ((1ull << (j & 63)) - 1ull));
        lmap[w.order[p]] = s < cap ? s : -2;
        if (j == p && s < cap) rep_pos[s] = p;
    }
    __syncthreads();
    for (int q = tid; q < N; q += BO_LANES) map[(size_t)r * N + q] = lmap[q];
    if (tid == 0) { cnt[2 * r] = ncl < cap ? ncl : cap; cnt[2 * r + 1] = ncl < cap ? 0 : ncl - cap; }

    // one lane per output slot: the merge sums in the order of the rule (representative first, members by position)
    if (tid >= cap) return;
    float* o = out + ((size_t)r * cap + tid) * 32;
    int32_t* oi = info + ((size_t)r * cap + tid) * 4;
    double* ob = obox ? obox + ((size_t)r * cap + tid) * 7 : nullptr;
    if (tid >= ncl) {
#pragma unroll
        for (int e = 0; e < 32; ++e) o[e] = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) oi[e] = 0;
        if (ob) {
#pragma unroll
            for (int e = 0; e < 7; ++e) ob[e] = 0.0;
        }
        return;
    }
    const int j = rep_pos[tid];
    const double* bj = w.box + (size_t)j * 8;
    const double ry_rep = bj[6];
    double v0 = bj[0], v1 = bj[1], v2 = bj[2], v3 = bj[3], v4 = bj[4], v5 = bj[5], v6 = ry_rep;
    const int qj = w.order[j];
    int members = 1;
    unsigned camera_mask = 1u << (qj / topk);
    const bool mean = P.merge == RTM3D_RIG_MERGE_MEAN;
    const double wj = (double)w.score[j];
    double Wsum = wj, s0 = wj * v0, s1 = wj * v1, s2 = wj * v2, s3 = wj * v3, s4 = wj * v4, s5 = wj * v5;
    double sd = wj * rig_wrap(ry_rep - ry_rep);
    const auto member = [&](int p) {
        ++members;
        camera_mask |= 1u << (w.order[p] / topk);
        if (mean) {
            const double* bp = w.box + (size_t)p * 8;
            const double wp = (double)w.score[p];
            double d = rig_wrap(bp[6] - ry_rep);
            if (d > RIG_HALF_PI) d = d - RIG_PI;
            else if (d < -RIG_HALF_PI) d = d + RIG_PI;
            Wsum = Wsum + wp;
            s0 = s0 + wp * bp[0]; s1 = s1 + wp * bp[1]; s2 = s2 + wp * bp[2];
            s3 = s3 + wp * bp[3]; s4 = s4 + wp * bp[4]; s5 = s5 + wp * bp[5];
            sd = sd + wp * d;
        }
    };
    // a member's position is behind its representative's; four positions per LDS read (positions from n on hold -1).  The scan
    // only threads the cluster's chain through next_of (this lane's own entries: no other lane reads or writes them); the walk
    // behind it then has the lanes of a wave load their k-th members together
    int last = j;
    const auto chain = [&](int p) { next_of[last] = p; last = p; };
    const int4* rep4 = (const int4*)rep_of;
    for (int p4 = j >> 2; 4 * p4 < n; ++p4) {
        const int4 v = rep4[p4];
        if (v.x == j && 4 * p4 != j) chain(4 * p4);
        if (v.y == j && 4 * p4 + 1 != j) chain(4 * p4 + 1);
        if (v.z == j && 4 * p4 + 2 != j) chain(4 * p4 + 2);
        if (v.w == j && 4 * p4 + 3 != j) chain(4 * p4 + 3);
    }
    next_of[last] = -1;
    for (int p = next_of[j]; p >= 0; p = next_of[p]) member(p);
    if (mean) {
        v0 = s0 / Wsum; v1 = s1 / Wsum; v2 = s2 / Wsum; v3 = s3 / Wsum; v4 = s4 / Wsum; v5 = s5 / Wsum;
        v6 = rig_wrap(ry_rep + sd / Wsum);
    }
    const float* rj = rec + ((size_t)r * N + qj) * 32;
    o[0] = rj[0]; o[1] = rj[1];
#pragma unroll
    for (int e = 2; e < 24; ++e) o[e] = 0.0f;
    o[24] = (float)v0; o[25] = (float)v1; o[26] = (float)v2; o[27] = (float)v3; o[28] = (float)v4; o[29] = (float)v5; o[30] = (float)v6;
    o[31] = 2.0f;
    oi[0] = qj / topk; oi[1] = qj - (qj / topk) * topk; oi[2] = members; oi[3] = (int32_t)camera_mask;
    if (ob) { ob[0] = v0; ob[1] = v1; ob[2] = v2; ob[3] = v3; ob[4] = v4; ob[5] = v5; ob[6] = v6; }
}

__global__ __launch_bounds__(BO_LANES) void rig_scatter_kernel(long long total, int per, int cap, const int32_t* __restrict__ map,
                                                              const int32_t* __restrict__ ids_rig, int32_t* __restrict__ ids_cam) {
    const long long t = (long long)blockIdx.x * BO_LANES + threadIdx.x;
    if (t >= total) return;
    const int m = map[t];
    ids_cam[t] = m >= 0 && m < cap ? ids_rig[(t / per) * cap + m] : 0;
}

extern void rt_set_error(const char* fmt, ...);

extern "C" int rtm3d_rig_default_params(rtm3d_rig_params* p) {
    if (!p) { rt_set_error("rig_default_params: null pointer"); return 1; }
    p->metric = 0; p->class_aware = 1; p->cross_only = 1; p->merge = RTM3D_RIG_MERGE_MEAN;
    p->thresh = 0.1; p->min_score = 0.0;
    return 0;
}

static bool rig_sizes_ok(int R, int C, int topk) {
    return R >= 1 && C >= 1 && C <= RIG_MAX_C && topk >= 1 && topk <= RIG_MAX_TOPK && C * topk <= RIG_MAX_N;
}

extern "C" size_t rtm3d_rig_workspace_bytes(int R, int C, int topk) {
    if (!rig_sizes_ok(R, C, topk)) return 0;
    return (size_t)R * rig_ws_units(C * topk) * 8;
}

extern "C" int rtm3d_rig_fuse(void* stream, int R, int C, int topk, int cap, const float* d_rec, const double* d_ext,
                              const rtm3d_rig_params* params, float* d_out, double* d_box, int32_t* d_info, int32_t* d_map,
                              int32_t* d_n, void* d_ws) {
    if (R < 1) { rt_set_error("rig_fuse: bad number of rigs R %d", R); return 1; }
    if (C < 1 || C > RIG_MAX_C) { rt_set_error("rig_fuse: C %d cameras per rig (1..%d)", C, RIG_MAX_C); return 1; }
    if (topk < 1 || topk > RIG_MAX_TOPK) { rt_set_error("rig_fuse: topk %d record slots per image (1..%d)", topk, RIG_MAX_TOPK); return 1; }
    if (C * topk > RIG_MAX_N) { rt_set_error("rig_fuse: C * topk %d record slots per rig (at most %d)", C * topk, RIG_MAX_N); return 1; }
    if (cap < 1 || cap > RIG_MAX_CAP) { rt_set_error("rig_fuse: cap %d output slots per rig (1..%d)", cap, RIG_MAX_CAP); return 1; }
    if (!params) { rt_set_error("rig_fuse: params is NULL"); return 1; }
    if (!d_rec || !d_ext || !d_out || !d_info || !d_map || !d_n || !d_ws) {
        rt_set_error("rig_fuse: null pointer (d_rec, d_ext, d_out, d_info, d_map, d_n and d_ws are required)"); return 1;
    }
    const rtm3d_rig_params& P = *params;
    if (P.metric < 0 || P.metric > 2) { rt_set_error("rig_fuse: unknown metric %d (0 BEV IoU, 1 3D IoU, 2 centre distance)", P.metric); return 1; }
    if (P.merge < 0 || P.merge > 1) { rt_set_error("rig_fuse: unknown merge %d (0 best, 1 mean)", P.merge); return 1; }
    if (P.thresh != P.thresh || P.min_score != P.min_score) { rt_set_error("rig_fuse: thresh or min_score is NaN"); return 1; }
    const int N = C * topk;
    const long long rows = (long long)R * N;
    const long long blocks = (rows + BO_LANES / 64 - 1) / (BO_LANES / 64);
    if (blocks > 0x7fffffffLL) { rt_set_error("rig_fuse: %lld record slots are more than one launch holds", rows); return 1; }
    hipLaunchKernelGGL(rig_prepare_kernel, dim3(R), dim3(BO_LANES), 0, (hipStream_t)stream, C, topk, d_rec, d_ext, P, d_ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("rig_fuse prepare launch: %s", hipGetErrorString(e)); return 1; }
    hipLaunchKernelGGL(rig_link_kernel, dim3((unsigned)blocks), dim3(BO_LANES), 0, (hipStream_t)stream, rows, N, topk, P, d_ws);
    e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("rig_fuse link launch: %s", hipGetErrorString(e)); return 1; }
    hipLaunchKernelGGL(rig_cluster_kernel, dim3(R), dim3(BO_LANES), 0, (hipStream_t)stream, C, topk, cap, d_rec, P, d_out, d_box, d_info,
                       d_map, d_n, d_ws);
    e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("rig_fuse cluster launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int rtm3d_rig_scatter_ids(void* stream, int R, int C, int topk, int cap, const int32_t* d_map, const int32_t* d_ids_rig,
                                     int32_t* d_ids_cam) {
    if (!rig_sizes_ok(R, C, topk)) {
        rt_set_error("rig_scatter_ids: R %d, C %d, topk %d (R >= 1, C 1..%d, topk 1..%d, C * topk at most %d)", R, C, topk, RIG_MAX_C,
                     RIG_MAX_TOPK, RIG_MAX_N);
        return 1;
    }
    if (cap < 1 || cap > RIG_MAX_CAP) { rt_set_error("rig_scatter_ids: cap %d output slots per rig (1..%d)", cap, RIG_MAX_CAP); return 1; }
    if (!d_map || !d_ids_rig || !d_ids_cam) { rt_set_error("rig_scatter_ids: null pointer (d_map, d_ids_rig and d_ids_cam are required)"); return 1; }
    const long long total = (long long)R * C * topk;
    const long long blocks = (total + BO_LANES - 1) / BO_LANES;
    if (blocks > 0x7fffffffLL) { rt_set_error("rig_scatter_ids: %lld slots are more than one launch holds", total); return 1; }
    hipLaunchKernelGGL(rig_scatter_kernel, dim3((unsigned)blocks), dim3(BO_LANES), 0, (hipStream_t)stream, total, C * topk, cap, d_map,
                       d_ids_rig, d_ids_cam);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("rig_scatter_ids launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
