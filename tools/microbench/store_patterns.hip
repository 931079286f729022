// Calibration: what the ADDRESS PATTERN of a conv epilogue's stores (and of its residual loads) costs on this chip, at equal bytes.
// Every conv kernel of the library writes its 16 x 16 accumulator tiles with the pixel on `lane & 15`: one global_store_dwordx4
// carries 16 pixels x 64 B, the four 16-B pieces of a 64-B run from lanes 16 apart, and a pixel is out_C * 2 bytes from the next
// (the 256 x 256 tile's epilogue is store-issue-bound at ~25 B / clk / CU).  Would lane-contiguous whole cache
// lines be cheaper?  The kernel below is the epilogue alone: 8 waves per workgroup, one workgroup per CU, every workgroup stores a
// 256-pixel x 256-channel fp16 tile (128 KB) from 64 packed registers per lane, all CUs together (a workgroup barrier in front of the
// burst, the same MFMA work in every workgroup between two bursts: `gap` x 8 MFMAs per wave = gap x 256 cycles per SIMD, the K loop
// of a 16-K-tile tile at the default 128), every burst to another tile of a 512 MB tensor of C channels (pixel pitch C * 2 * scale
// bytes; scale 2 = the transposed convs' every-other-pixel phases).  Patterns, per store instruction of a wave:
//   a    today's: 16 pixels x 64 B, dwordx4, lane (fk, frow) -> pixel frow, bytes (fk & 1) * 32 + (fk >> 1) * 16 of the run
//   a8   the same fragment without the permlane16 swap: 16 pixels x 32 B, dwordx2 (what the residual LOADS do today)
//   b    dwordx2, lanes 16 k .. 16 k + 15 = one pixel's 128 contiguous bytes: 4 pixels x 128 B
//   c    dwordx4, 16 adjacent lanes = 256 contiguous bytes of one pixel: 4 pixels x 256 B (wave tile 64 pixels x 128 channels)
//   d    dwordx4, the even and the odd lanes of a 16-lane group one pixel's 128 B each: 8 pixels x 128 B
//   none no memory instruction (the MFMA gap alone: what to subtract from the wall times)
// and the same address patterns as loads of the tile (a8 = today's residual loads; b 8 bytes per lane; c and d 16 bytes per lane: a
// lane's two adjacent 8-byte loads are merged by hipcc into one global_load_dwordx4 - built and checked in the ISA - and kept apart
// with `volatile` they get a vmcnt(0) each, so an 8-byte form of c and d is not something a HIP kernel would run), from a 64 MB
// window that stays in the Infinity Cache
// (a residual is the input of the layer before: HBM would hide the pattern behind its own 6.4 us per 32 MB).
// Per pattern: cycles (s_memtime) from the barrier to the last store ISSUED, to this wave's vmcnt(0), and to the barrier behind it
// (= the workgroup's burst), mean over bursts, median over workgroups; the in-kernel clock (s_memtime / s_memrealtime over the
// launch); ms per launch and us of wall per burst over the `none` launch.  >= 2 s of back-to-back launches before each timed batch.
// Measured (profiles/store_patterns.txt; cycles per burst at 256 / 1024 channels): stores a 8.6k / 8.7k, a8 16.8k (one cycle per piece,
// whatever its size), b 5.2k / 5.4k, c 3.2k / 3.4k, d 5.3k / 5.2k; loads a8 17.2k / 17.3k, b 6.8k / 7.3k, c 4.4k / 5.0k, d 6.9k / 6.8k.
// Pattern b is what the 256 x 256 conv kernels store in now (rtm3d_amd/csrc/conv_mfma256.hip, "Store layout").
// Before any timing every store pattern is run once on a 0xFF-filled tensor and the image checked: the 256 tiles written exactly,
// every other byte untouched.
// build: hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -o tools/microbench/store_patterns.out
//        tools/microbench/store_patterns.hip ; run on the GPU box under a time limit: store_patterns.out [warm_s [bursts [gap]]]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

enum { PAT_A = 0, PAT_B = 1, PAT_C = 2, PAT_D = 3, PAT_A8 = 4, PAT_NONE = 5 };
constexpr size_t TENSOR_BYTES = (size_t)512 << 20, TILE_BYTES = 128 << 10;
constexpr int N_WG = 256, N_RND = 8 << 20;                 // workgroups = CUs; random dwords (32 MB)

// Where lane `lane` of wave `wave` sits in the 256-pixel x 512-byte tile (pixel, byte of the pixel's 512), and what instruction q
// of its burst adds to that.  Host and device: main() checks on the host that every pattern covers the tile exactly once.
__host__ __device__ constexpr int pat_bytes(int pat) { return pat == PAT_B || pat == PAT_A8 ? 8 : 16; }
__host__ __device__ constexpr int pat_instr(int pat) { return (16 << 10) / (64 * pat_bytes(pat)); }
__host__ __device__ inline void lane_geom(int pat, int wave, int lane, int& px, int& chb) {
    const int frow = lane & 15, fk = lane >> 4, wp = wave & 1, wc = wave >> 1;
    switch (pat) {
    case PAT_A:  px = wp * 64 + frow;                 chb = wc * 64 + (fk & 1) * 32 + (fk >> 1) * 16; break;
    case PAT_A8: px = wp * 64 + frow;                 chb = wc * 64 + fk * 8; break;
    case PAT_B:  px = wp * 64 + fk;                   chb = wc * 128 + frow * 8; break;
    case PAT_C:  px = (wave & 3) * 64 + fk;           chb = (wave >> 2) * 256 + frow * 16; break;
    default:     px = wp * 64 + fk * 2 + (lane & 1);  chb = wc * 128 + (frow >> 1) * 16; break;
    }
}
__host__ __device__ constexpr int instr_px(int pat, int q) {
    return pat == PAT_A ? (q >> 3) * 128 + ((q >> 1) & 3) * 16 : pat == PAT_A8 ? (q >> 4) * 128 + ((q >> 2) & 3) * 16
         : pat == PAT_B ? (q >> 4) * 128 + (q & 15) * 4 : pat == PAT_C ? q * 4 : (q >> 3) * 128 + (q & 7) * 8;
}
__host__ __device__ constexpr int instr_chb(int pat, int q) {
    return pat == PAT_A ? (q & 1) * 256 : pat == PAT_A8 ? ((q >> 1) & 1) * 256 + (q & 1) * 32 : 0;
}

struct Stamp { unsigned long long issue, done, wg, cyc, real; };

template <int PAT, int LOAD>
__global__ __launch_bounds__(512) void store_pattern_kernel(const uint32_t* rnd, char* tensor, unsigned pitch, unsigned ntc, unsigned ntiles,
                                                            int bursts, int gap, uint32_t fill, Stamp* stamps, float* out) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t u[64];                                        // the wave's 16 KB of the tile: 64 packed registers per lane
#pragma unroll
    for (int i = 0; i < 64; ++i) u[i] = rnd[(blockIdx.x * 64 + i) * 512 + tid];
    if (fill) {                                            // the image check: one known word everywhere
#pragma unroll
        for (int i = 0; i < 64; ++i) u[i] = fill;
    }
    const f16x8 wa = *(const f16x8*)(rnd + tid * 4), xa = *(const f16x8*)(rnd + 4096 + tid * 4);
    f32x4 acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int px0 = 0, chb0 = 0;
    if (PAT != PAT_NONE) lane_geom(PAT, wave, lane, px0, chb0);
    const size_t lane_off = (size_t)px0 * pitch + chb0;
    unsigned long long s_issue = 0, s_done = 0, s_wg = 0;
    uint32_t keep = 0;
    const unsigned long long c_begin = __builtin_amdgcn_s_memtime(), r_begin = __builtin_amdgcn_s_memrealtime();
    for (int s = 0; s < bursts; ++s) {
        for (int g = 0; g < gap; ++g)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, xa, acc[k], 0, 0, 0);
        const unsigned tile = ((unsigned)s * N_WG + blockIdx.x) % ntiles;
        char* base = tensor + (size_t)(tile / ntc) * 256 * pitch + (size_t)(tile % ntc) * 512 + lane_off;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        uint32_t r[64];                                    // LOAD: registers of the burst's own (folded into `keep` behind the stamps)
        if (PAT != PAT_NONE) {
#pragma unroll
            for (int q = 0; q < pat_instr(PAT); ++q) {
                char* p = base + (size_t)instr_px(PAT, q) * pitch + instr_chb(PAT, q);
                if (pat_bytes(PAT) == 8) {
                    if (LOAD) { const u32x2 v = *(const u32x2*)p; r[2 * q] = v[0]; r[2 * q + 1] = v[1]; }
                    else *(u32x2*)p = (u32x2){u[2 * q], u[2 * q + 1]};
                } else {
                    if (LOAD) { const u32x4 v = *(const u32x4*)p; r[4 * q] = v[0]; r[4 * q + 1] = v[1]; r[4 * q + 2] = v[2]; r[4 * q + 3] = v[3]; }
                    else *(u32x4*)p = (u32x4){u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]};
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const unsigned long long t2 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        const unsigned long long t3 = __builtin_amdgcn_s_memtime();
        s_issue += t1 - t0; s_done += t2 - t0; s_wg += t3 - t0;
        __builtin_amdgcn_sched_barrier(0);
        if (LOAD && PAT != PAT_NONE) {
#pragma unroll
            for (int i = 0; i < 64; ++i) keep ^= r[i];
        }
    }
    const unsigned long long c_end = __builtin_amdgcn_s_memtime(), r_end = __builtin_amdgcn_s_memrealtime();
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) sum += acc[k][0] + acc[k][1] + acc[k][2] + acc[k][3];
#pragma unroll
    for (int i = 0; i < 64; ++i) keep ^= u[i];
    out[(size_t)blockIdx.x * 512 + tid] = sum + (float)(keep & 1u);
    if (lane == 0) stamps[blockIdx.x * 8 + wave] = Stamp{s_issue, s_done, s_wg, c_end - c_begin, r_end - r_begin};
}

typedef void (*Launch)(const uint32_t*, char*, unsigned, unsigned, unsigned, int, int, uint32_t, Stamp*, float*, hipStream_t);
template <int PAT, int LOAD>
static void launch(const uint32_t* rnd, char* tensor, unsigned pitch, unsigned ntc, unsigned ntiles, int bursts, int gap, uint32_t fill, Stamp* st, float* out, hipStream_t s) {
    hipLaunchKernelGGL((store_pattern_kernel<PAT, LOAD>), dim3(N_WG), dim3(512), 0, s, rnd, tensor, pitch, ntc, ntiles, bursts, gap, fill, st, out);
}
struct Variant { const char* name; int pat, load; Launch launch; };

// every (wave, lane, instruction, byte) of a pattern hits each byte of the 256 x 512 tile exactly once
static bool host_cover(int pat) {
    std::vector<unsigned char> hit(256 * 512, 0);
    for (int wave = 0; wave < 8; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
            int px, chb;
            lane_geom(pat, wave, lane, px, chb);
            for (int q = 0; q < pat_instr(pat); ++q)
                for (int b = 0; b < pat_bytes(pat); ++b) {
                    const int p = px + instr_px(pat, q), c = chb + instr_chb(pat, q) + b;
                    if (p < 0 || p >= 256 || c < 0 || c >= 512 || hit[p * 512 + c]++) return false;
                }
        }
    return std::count(hit.begin(), hit.end(), 1) == 256 * 512;
}

int main(int argc, char** argv) {
    const double warm_s = argc > 1 ? atof(argv[1]) : 2.0;
    const int bursts = argc > 2 ? atoi(argv[2]) : 16;
    const int gap = argc > 3 ? atoi(argv[3]) : 128;
    for (int pat = PAT_A; pat <= PAT_A8; ++pat)
        if (!host_cover(pat)) { printf("pattern %d does not cover the tile exactly once\n", pat); return 1; }
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    printf("# device %s, %d CUs; %d workgroups x 8 waves, %d bursts of 128 KB per workgroup and launch, %d x 8 MFMAs per wave between bursts;\n"
           "# %.1f s of back-to-back launches before each timed batch; random fp16 bits in the registers\n", prop.name, prop.multiProcessorCount, N_WG, bursts, gap, warm_s);
    std::vector<uint32_t> h(N_RND);
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (auto& v : h) {          // two random halves per word: random sign and mantissa, exponent field <= 14, so |v| < 1
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t a = (uint32_t)(x >> 33) & 0xBBFFu, b = (uint32_t)(x >> 17) & 0xBBFFu;
        v = a | (b << 16);
    }
    uint32_t* d_rnd; char* d_t; float* d_out; Stamp* d_st;
    CK(hipMalloc(&d_rnd, (size_t)N_RND * 4));
    CK(hipMalloc(&d_t, TENSOR_BYTES));
    CK(hipMalloc(&d_out, (size_t)N_WG * 512 * 4));
    CK(hipMalloc(&d_st, (size_t)N_WG * 8 * sizeof(Stamp)));
    CK(hipMemcpy(d_rnd, h.data(), (size_t)N_RND * 4, hipMemcpyHostToDevice));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

    const Variant vs[] = {
        {"none    (the MFMA gap alone)", PAT_NONE, 0, launch<PAT_NONE, 0>},
        {"store a  16 px x  64 B  x4 (today)", PAT_A, 0, launch<PAT_A, 0>},
        {"store a8 16 px x  32 B  x2 (no swap)", PAT_A8, 0, launch<PAT_A8, 0>},
        {"store b   4 px x 128 B  x2", PAT_B, 0, launch<PAT_B, 0>},
        {"store c   4 px x 256 B  x4", PAT_C, 0, launch<PAT_C, 0>},
        {"store d   8 px x 128 B  x4 (even/odd)", PAT_D, 0, launch<PAT_D, 0>},
        {"load  a8 16 px x  32 B  x2 (today)", PAT_A8, 1, launch<PAT_A8, 1>},
        {"load  b   4 px x 128 B  x2", PAT_B, 1, launch<PAT_B, 1>},
        {"load  c   4 px x 256 B  x4", PAT_C, 1, launch<PAT_C, 1>},
        {"load  d   8 px x 128 B  x4 (even/odd)", PAT_D, 1, launch<PAT_D, 1>},
    };
    struct Shape { int C, scale; } shapes[] = {{256, 1}, {1024, 1}, {256, 2}};
    std::vector<uint32_t> img;
    for (const Shape& sh : shapes) {
        const unsigned pitch = (unsigned)(sh.C * 2 * sh.scale), ntc = (unsigned)(sh.C / 256);
        const unsigned ntiles = (unsigned)(TENSOR_BYTES / ((size_t)256 * pitch)) * ntc;          // whole pixel tiles inside the tensor
        const unsigned win_tiles = std::min(ntiles, (unsigned)(((size_t)64 << 20) / ((size_t)256 * pitch)) * ntc);
        // ---- the image each store pattern leaves: tiles 0..255 written with the fill word, everything else still 0xFF
        const size_t chk_bytes = (size_t)(N_WG / ntc) * 256 * pitch;
        const uint32_t fill = 0x3C003C00u;
        for (const Variant& v : vs) {
            if (v.load || v.pat == PAT_NONE) continue;
            CK(hipMemset(d_t, 0xFF, chk_bytes + (1 << 20)));
            v.launch(d_rnd, d_t, pitch, ntc, ntiles, 1, 0, fill, d_st, d_out, s);
            CK(hipStreamSynchronize(s));
            img.resize((chk_bytes + (1 << 20)) / 4);
            CK(hipMemcpy(img.data(), d_t, img.size() * 4, hipMemcpyDeviceToHost));
            size_t n_fill = 0, n_bad = 0;
            for (size_t i = 0; i < img.size(); ++i) {
                const size_t byte = i * 4, px = byte / pitch, in_px = byte % pitch;
                const bool inside = byte < chk_bytes && in_px < (size_t)sh.C * 2;               // scale 2: the odd pixels stay untouched
                if (img[i] == fill) ++n_fill;
                if (img[i] != (inside ? fill : 0xFFFFFFFFu)) ++n_bad;
                (void)px;
            }
            if (n_bad || n_fill != (size_t)N_WG * TILE_BYTES / 4) { printf("%s: wrong image at C=%d scale=%d (%zu words written, %zu wrong)\n", v.name, sh.C, sh.scale, n_fill, n_bad); return 1; }
        }
        printf("\n## C = %d channels, pixel pitch %u B (scale %d): every store pattern writes its 256 tiles exactly; stores walk %u tiles (%.0f MB), loads %u (%.0f MB)\n",
               sh.C, pitch, sh.scale, ntiles, ntiles / ntc * 256.0 * pitch / 1048576.0, win_tiles, win_tiles / ntc * 256.0 * pitch / 1048576.0);
        printf("%-40s %9s %9s %9s %7s %9s %9s %9s\n", "pattern", "cyc issue", "cyc wave", "cyc burst", "vs a", "clock GHz", "ms/launch", "us/burst");
        double ms_none = 0.0, cyc_a[2] = {0.0, 0.0};
        for (const Variant& v : vs) {
            const unsigned nt = v.load ? win_tiles : ntiles;
            const auto t0 = std::chrono::steady_clock::now();
            int warm = 0;
            for (;;) {
                for (int i = 0; i < 20; ++i) v.launch(d_rnd, d_t, pitch, ntc, nt, bursts, gap, 0u, d_st, d_out, s);
                warm += 20;
                CK(hipStreamSynchronize(s));
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= warm_s) break;
            }
            const int timed = 100;
            CK(hipEventRecord(e0, s));
            for (int i = 0; i < timed; ++i) v.launch(d_rnd, d_t, pitch, ntc, nt, bursts, gap, 0u, d_st, d_out, s);
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, e0, e1));
            ms /= timed;
            std::vector<Stamp> st((size_t)N_WG * 8);
            CK(hipMemcpy(st.data(), d_st, st.size() * sizeof(Stamp), hipMemcpyDeviceToHost));
            std::vector<double> is, dn, wg, ghz;
            for (auto& q : st) {
                is.push_back((double)q.issue / bursts); dn.push_back((double)q.done / bursts); wg.push_back((double)q.wg / bursts);
                ghz.push_back((double)q.cyc / (double)q.real * 0.1);
            }
            for (auto* a : {&is, &dn, &wg, &ghz}) std::sort(a->begin(), a->end());
            const size_t mid = st.size() / 2;
            if (v.pat == PAT_NONE) ms_none = ms;
            if (v.pat == PAT_A && !v.load) cyc_a[0] = wg[mid];
            if (v.pat == PAT_A8 && v.load) cyc_a[1] = wg[mid];
            const double ref = cyc_a[v.load];
            printf("%-40s %9.0f %9.0f %9.0f %7.2f %9.3f %9.4f %9.2f   (%d warm-up launches; burst cycles min %.0f max %.0f over workgroups)\n", v.name, is[mid], dn[mid], wg[mid],
                   v.pat == PAT_NONE || ref == 0.0 ? 0.0 : wg[mid] / ref, ghz[mid], ms, (ms - ms_none) * 1e3 / bursts, warm, wg.front(), wg.back());
            fflush(stdout);
        }
    }
    return 0;
}
