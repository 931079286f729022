// Optimiser step (include/rtm3d_hip.h, "optimiser step"): Adamax with torch's arithmetic order, an optional weight EMA and a
// non-finite-loss guard, over every parameter of a model in ONE launch.  The host plans once (rtm3d_optim_plan: a segment
// table and a table of fixed-size chunks, no chunk across a segment); per step the host passes the scalars by value and the
// workgroups stride over the chunk table.  One streaming pass: 4 reads + 3 writes of fp32 per element (5 + 4 with the EMA).
// Every element has one writer and there is no atomic: two runs on equal inputs leave equal bytes.
// Built with -ffp-contract=off (Makefile): each operation of the rule is its own correctly rounded fp32 operation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/rtm3d_hip.h"

#define OPT_CHUNK RTM3D_OPTIM_CHUNK
#define OPT_THREADS 1024                    // one access of 16 B per lane covers a whole chunk
#define OPT_GRID_PER_CU 1
static_assert(OPT_CHUNK % 256 == 0 && OPT_CHUNK == 4 * OPT_THREADS, "a chunk is one pass of 16 B per lane");
static_assert(sizeof(rtm3d_optim_segment) == 56 && sizeof(rtm3d_optim_chunk) == 8, "table entries as the header lays them out");

typedef float f32x4 __attribute__((ext_vector_type(4)));
// The table's pointers are loaded from memory, where the compiler knows no address space and would issue flat accesses; they
// are device addresses by contract.
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// Gradients are read once and never again: non-temporal loads.  p, m, u and e are read and written back at once; plain loads
// measured no slower for them (profiles/optim.txt; -DOPT_NT_ALL is the diagnostic build that makes them non-temporal too).
#ifdef OPT_NT_ALL
#define OPT_LOAD(ptr) __builtin_nontemporal_load(ptr)
#else
#define OPT_LOAD(ptr) (*(ptr))
#endif

struct OptScalars {                       // the uniform scalars of one segment's class
    float nclr, wd, w, omw, beta2, eps, d, omd;
    bool has_wd, lerp_lo;
};

// m, u, p of one element; g is consumed.  The order and the branches are the rule's.
__device__ __forceinline__ void opt_update(const OptScalars& k, float g, float& p, float& m, float& u) {
    const float g1 = k.has_wd ? g + k.wd * p : g;
    const float diff = g1 - m;
    const float m1 = k.lerp_lo ? m + k.w * diff : g1 - diff * k.omw;
    const float a = u * k.beta2, b = fabsf(g1) + k.eps;
    const float u1 = (a > b || a != a) ? a : b;                    // a NaN operand wins (fmaxf would drop it)
    p = p + k.nclr * (m1 / u1);
    m = m1; u = u1;
}
__device__ __forceinline__ float opt_ema(const OptScalars& k, float e, float p) { return e * k.d + k.omd * p; }

// KIND 0: update + EMA, 1: update only, 2: EMA only (p is read, never written).  VEC: 16 B per lane, every pointer the kind
// uses is 16-byte aligned at the chunk's first element; the (cnt & 3) last elements take the scalar statements.
template <int KIND, bool VEC>
__device__ __forceinline__ void opt_chunk(const rtm3d_optim_segment& s, long long base, int cnt, const OptScalars& k) {
    gf32* p = (gf32*)s.p + base;
    const gf32* g = (const gf32*)s.g + base;
    gf32* m = (gf32*)s.m + base;
    gf32* u = (gf32*)s.u + base;
    gf32* e = (gf32*)s.e + base;
    int done = 0;
    if (VEC) {
        const int nv = cnt >> 2;
        for (int i = threadIdx.x; i < nv; i += OPT_THREADS) {
            f32x4 pv = OPT_LOAD((const gf32x4*)p + i), ev;
            if (KIND != 2) {
                const f32x4 gv = __builtin_nontemporal_load((const gf32x4*)g + i);
                f32x4 mv = OPT_LOAD((const gf32x4*)m + i), uv = OPT_LOAD((const gf32x4*)u + i);
                if (KIND == 0) ev = OPT_LOAD((const gf32x4*)e + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) { float pj = pv[j], mj = mv[j], uj = uv[j]; opt_update(k, gv[j], pj, mj, uj); pv[j] = pj; mv[j] = mj; uv[j] = uj; }
                ((gf32x4*)p)[i] = pv; ((gf32x4*)m)[i] = mv; ((gf32x4*)u)[i] = uv;
            } else {
                ev = OPT_LOAD((const gf32x4*)e + i);
            }
            if (KIND != 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ev[j] = opt_ema(k, ev[j], pv[j]);
                ((gf32x4*)e)[i] = ev;
            }
        }
        done = nv << 2;
    }
    for (int i = done + threadIdx.x; i < cnt; i += OPT_THREADS) {
        float pj = p[i];
        if (KIND != 2) {
            float mj = m[i], uj = u[i];
            opt_update(k, __builtin_nontemporal_load(g + i), pj, mj, uj);
            p[i] = pj; m[i] = mj; u[i] = uj;
        }
        if (KIND != 1) e[i] = opt_ema(k, e[i], pj);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const rtm3d_optim_segment* __restrict__ segs,
                                                                 const rtm3d_optim_chunk* __restrict__ chunks, int n_chunks,
                                                                 rtm3d_optim_hyper h, const float* __restrict__ loss,
                                                                 unsigned* __restrict__ skipped) {
    if (loss) {                                                   // the guard: a NaN or +-Inf loss leaves every byte as it is
        const float L = *loss;
        if (!(fabsf(L) <= 3.4028234663852886e38f)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) skipped[0] = skipped[0] + 1u;
            return;
        }
    }
    OptScalars k;
    k.w = h.w; k.omw = 1.0f - h.w; k.lerp_lo = h.w < 0.5f; k.beta2 = h.beta2; k.eps = h.eps; k.d = h.ema_d; k.omd = h.ema_omd;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const rtm3d_optim_chunk ck = chunks[c];
        const rtm3d_optim_segment s = segs[ck.segment];
        const long long base = (long long)ck.index * OPT_CHUNK;
        const long long left = s.n - base;
        const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
        const int cls = s.cls & (RTM3D_OPTIM_MAX_CLASSES - 1);
        k.nclr = h.nclr[cls]; k.wd = h.wd[cls]; k.has_wd = k.wd != 0.0f;
        // (base is a multiple of 16 bytes: a chunk is as aligned as its segment)
        uintptr_t bits = (uintptr_t)s.p;
        if (s.kind != 2) bits |= (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.u;
        if (s.kind != 1) bits |= (uintptr_t)s.e;
        const bool vec = (bits & 15) == 0;
        if (s.kind == 0) { if (vec) opt_chunk<0, true>(s, base, cnt, k); else opt_chunk<0, false>(s, base, cnt, k); }
        else if (s.kind == 1) { if (vec) opt_chunk<1, true>(s, base, cnt, k); else opt_chunk<1, false>(s, base, cnt, k); }
        else { if (vec) opt_chunk<2, true>(s, base, cnt, k); else opt_chunk<2, false>(s, base, cnt, k); }
    }
}

// ---------------------------------------------------------------------------------------------------- host
extern void rt_set_error(const char* fmt, ...);

#define OPT_MAX_ELEMS (1LL << 40)          // per segment; keeps every byte range and the chunk count far from overflow
static long long chunks_of(long long n) { return n / OPT_CHUNK + (n % OPT_CHUNK != 0); }

extern "C" int rtm3d_optim_table_bytes(int n_segments, const long long* sizes, size_t* segment_bytes, size_t* chunk_bytes, int* n_chunks) {
    const char* who = "optim_table_bytes";
    if (!sizes || !segment_bytes || !chunk_bytes || !n_chunks) { rt_set_error("%s: null pointer", who); return RTM3D_OPTIM_E_NULL; }
    if (n_segments < 1) { rt_set_error("%s: %d segments", who, n_segments); return RTM3D_OPTIM_E_COUNT; }
    long long total = 0;
    for (int i = 0; i < n_segments; ++i) {
        if (sizes[i] < 0 || sizes[i] > OPT_MAX_ELEMS) { rt_set_error("%s: segment %d has %lld elements", who, i, sizes[i]); return RTM3D_OPTIM_E_SIZE; }
        total += chunks_of(sizes[i]);
        if (total > 0x7fffffffLL) { rt_set_error("%s: more than 2^31 - 1 chunks", who); return RTM3D_OPTIM_E_TOO_MANY; }
    }
    *segment_bytes = (size_t)n_segments * sizeof(rtm3d_optim_segment);
    *chunk_bytes = (size_t)total * sizeof(rtm3d_optim_chunk);
    *n_chunks = (int)total;
    return 0;
}

extern "C" int rtm3d_optim_plan(int n_segments, const rtm3d_optim_segment* segments, rtm3d_optim_segment* segment_table,
                                rtm3d_optim_chunk* chunk_table, int* n_chunks) {
    const char* who = "optim_plan";
    if (!segments || !segment_table || !chunk_table || !n_chunks) { rt_set_error("%s: null pointer", who); return RTM3D_OPTIM_E_NULL; }
    if (n_segments < 1) { rt_set_error("%s: %d segments", who, n_segments); return RTM3D_OPTIM_E_COUNT; }
    struct Range { uintptr_t lo, hi; int seg; char name; };
    std::vector<Range> ranges;
    ranges.reserve((size_t)n_segments * 5);
    long long total = 0;
    for (int i = 0; i < n_segments; ++i) {
        const rtm3d_optim_segment& s = segments[i];
        if (s.n < 0 || s.n > OPT_MAX_ELEMS) { rt_set_error("%s: segment %d has %lld elements", who, i, s.n); return RTM3D_OPTIM_E_SIZE; }
        if (s.kind < 0 || s.kind > 2) { rt_set_error("%s: segment %d: kind %d is none of 0 (update + EMA), 1 (update), 2 (EMA)", who, i, s.kind); return RTM3D_OPTIM_E_KIND; }
        if (s.cls < 0 || s.cls >= RTM3D_OPTIM_MAX_CLASSES) { rt_set_error("%s: segment %d: class %d, a launch takes %d", who, i, s.cls, RTM3D_OPTIM_MAX_CLASSES); return RTM3D_OPTIM_E_CLASS; }
        total += chunks_of(s.n);
        if (total > 0x7fffffffLL) { rt_set_error("%s: more than 2^31 - 1 chunks", who); return RTM3D_OPTIM_E_TOO_MANY; }
        if (s.n == 0) continue;                                            // no chunk, no access
        const void* ptr[5] = {s.p, s.g, s.m, s.u, s.e};
        const bool used[5] = {true, s.kind != 2, s.kind != 2, s.kind != 2, s.kind != 1};
        for (int j = 0; j < 5; ++j) {
            if (!used[j]) continue;
            if (!ptr[j]) { rt_set_error("%s: segment %d: %c is a NULL pointer", who, i, "pgmue"[j]); return RTM3D_OPTIM_E_NULL; }
            if ((uintptr_t)ptr[j] & 3) { rt_set_error("%s: segment %d: the address of %c is no multiple of 4", who, i, "pgmue"[j]); return RTM3D_OPTIM_E_ALIGN; }
            ranges.push_back({(uintptr_t)ptr[j], (uintptr_t)ptr[j] + (uintptr_t)s.n * 4u, i, "pgmue"[j]});
        }
    }
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    for (size_t r = 1; r < ranges.size(); ++r)                             // (sorted by start: any overlap shows between neighbours)
        if (ranges[r].lo < ranges[r - 1].hi) {
            rt_set_error("%s: %c of segment %d overlaps %c of segment %d", who, ranges[r].name, ranges[r].seg, ranges[r - 1].name, ranges[r - 1].seg);
            return RTM3D_OPTIM_E_OVERLAP;
        }
    int c = 0;
    for (int i = 0; i < n_segments; ++i) {
        segment_table[i] = segments[i];
        const int nc = (int)chunks_of(segments[i].n);
        for (int j = 0; j < nc; ++j) { chunk_table[c].segment = i; chunk_table[c].index = j; ++c; }
    }
    *n_chunks = c;
    return 0;
}

static int grid_limit() {
    static int cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return OPT_GRID_PER_CU * 64;
    if (!cached[dev]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 64;
        cached[dev] = OPT_GRID_PER_CU * cus;
    }
    return cached[dev];
}

extern "C" int rtm3d_optim_step(void* stream, const rtm3d_optim_segment* d_segment_table, const rtm3d_optim_chunk* d_chunk_table,
                                int n_chunks, const rtm3d_optim_hyper* hyper, const float* d_loss, unsigned* d_skipped) {
    const char* who = "optim_step";
    if (!d_segment_table || !d_chunk_table || !hyper || !d_skipped) { rt_set_error("%s: null pointer", who); return RTM3D_OPTIM_E_NULL; }
    if (n_chunks < 1) { rt_set_error("%s: %d chunks", who, n_chunks); return RTM3D_OPTIM_E_COUNT; }
    if (((uintptr_t)d_segment_table & 7) || ((uintptr_t)d_chunk_table & 7) || ((uintptr_t)d_loss & 3) || ((uintptr_t)d_skipped & 3)) {
        rt_set_error("%s: a table, the loss or the counter is misaligned", who); return RTM3D_OPTIM_E_ALIGN;
    }
    const int limit = grid_limit();
    const int grid = n_chunks < limit ? n_chunks : limit;
    hipLaunchKernelGGL(optim_step_kernel, dim3((unsigned)grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, d_segment_table, d_chunk_table,
                       n_chunks, *hyper, d_loss, d_skipped);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("%s launch: %s", who, hipGetErrorString(e)); return RTM3D_OPTIM_E_LAUNCH; }
    return 0;
}
