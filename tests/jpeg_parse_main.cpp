// Stand-alone robustness run of the JPEG host decoder (rtm3d_amd/csrc/jpeg_host.cpp, the only other file it links).
//
//   jpeg_parse_main <streams file>
//
// The file holds the fixture streams: uint32 count, then per stream uint32 length and the bytes (an entry of length 0 separates
// the streams that must decode from those that must not crash).  For every stream the program
// decodes every truncation 0 .. length and a fixed number of seeded mutations (one byte, and a burst of up to four), each through
// rtm3d_jpeg_info and rtm3d_jpeg_entropy_decode.  The input copy and the coefficient buffer stand between canaries of 64 bytes;
// a call must return 0 (decoded) or 1 (refused), leave every canary as it was, write nothing when it refuses for capacity, and
// the untouched stream must decode.  Built with -fsanitize=address the input copy is an allocation of exactly the stream's
// length instead, so that a read past its end is caught too.  Exit status 0 and a line of counts, or 1 and the first failure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/rtm3d_hip.h"

static char g_error[512];
void rt_set_error(const char* fmt, ...) {             // the library's error channel (csrc/runtime.hip), for this program
    (void)fmt;
    snprintf(g_error, sizeof(g_error), "set");
}

#if defined(__SANITIZE_ADDRESS__)
#define EXACT_INPUT 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define EXACT_INPUT 1
#endif
#endif
#ifndef EXACT_INPUT
#define EXACT_INPUT 0
#endif

enum { CANARY = 64, CANARY_BYTE = 0xC7, MUTATIONS = 400 };

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                                // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}

static long n_calls = 0, n_ok = 0, n_refused = 0;

static bool canaries_intact(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < CANARY; ++i)
        if (p[i] != CANARY_BYTE || p[CANARY + n + i] != CANARY_BYTE) return false;
    return true;
}

// one stream of n bytes through both entry points; false on a failure (reported)
static bool run(const uint8_t* bytes, size_t n, const char* what, bool must_decode) {
#if EXACT_INPUT
    uint8_t* in_alloc = (uint8_t*)malloc(n ? n : 1);
    uint8_t* in = in_alloc;
#else
    uint8_t* in_alloc = (uint8_t*)malloc(n + 2 * CANARY);
    memset(in_alloc, CANARY_BYTE, n + 2 * CANARY);
    uint8_t* in = in_alloc + CANARY;
#endif
    if (n) memcpy(in, bytes, n);
    bool good = true;
    rtm3d_jpeg_stream_info I;
    const int rc_info = rtm3d_jpeg_info(in, n, &I);
    ++n_calls;
    if (rc_info != 0 && rc_info != 1) { printf("FAIL %s: jpeg_info returned %d\n", what, rc_info); good = false; }
    if (good && rc_info == 0 && (I.h < 1 || I.w < 1 || I.h > 16384 || I.w > 16384 || I.coef_count % 64 || I.coef_count < 256)) {
        printf("FAIL %s: jpeg_info accepted %d x %d with %zu coefficients\n", what, I.h, I.w, I.coef_count); good = false;
    }
    if (good) {
        // a frame the mutation made huge is decoded into a buffer that is too small: it must be refused and written nowhere
        const size_t want = rc_info == 0 ? I.coef_count : 256;
        const size_t cap = want > ((size_t)1 << 22) ? 4096 : (rnd() % 16 == 0 && want > 64 ? want - 64 : want);
        std::vector<uint8_t> out(cap * 2 + 2 * CANARY, CANARY_BYTE);
        const int rc = rtm3d_jpeg_entropy_decode(in, n, (int16_t*)(out.data() + CANARY), cap);
        ++n_calls;
        if (rc == 0) ++n_ok; else ++n_refused;
        if (rc != 0 && rc != 1) { printf("FAIL %s: jpeg_entropy_decode returned %d\n", what, rc); good = false; }
        if (good && !canaries_intact(out.data(), cap * 2)) { printf("FAIL %s: a canary of the coefficient buffer changed\n", what); good = false; }
        if (good && rc == 0 && (rc_info != 0 || cap < I.coef_count)) { printf("FAIL %s: decoded what jpeg_info or the capacity refuses\n", what); good = false; }
        if (good && cap < want) {
            for (size_t i = 0; i < cap * 2 && good; ++i)
                if (out[CANARY + i] != CANARY_BYTE) { printf("FAIL %s: a refusal for capacity wrote to the buffer\n", what); good = false; }
        }
        if (good && must_decode && cap >= want && rc != 0) { printf("FAIL %s: the untouched stream was refused\n", what); good = false; }
    }
#if !EXACT_INPUT
    if (good && (!canaries_intact(in_alloc, n) || (n && memcmp(in, bytes, n) != 0))) { printf("FAIL %s: the input or its canaries changed\n", what); good = false; }
#endif
    free(in_alloc);
    return good;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <streams file>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count == 0 || count > 4096) { fprintf(stderr, "bad streams file\n"); return 2; }
    char what[96];
    for (uint32_t s = 0; s < count; ++s) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1 || len > (1u << 24)) { fprintf(stderr, "bad streams file\n"); return 2; }
        std::vector<uint8_t> d(len);
        if (len && fread(d.data(), 1, len, f) != len) { fprintf(stderr, "bad streams file\n"); return 2; }
        // the streams that must decode come first; an entry of length 0 separates them from those that are there to be refused
        static bool must_decode = true;
        if (len == 0) { must_decode = false; continue; }
        snprintf(what, sizeof(what), "stream %u whole", s);
        if (!run(d.data(), len, what, must_decode)) return 1;
        for (uint32_t n = 0; n < len; ++n) {
            snprintf(what, sizeof(what), "stream %u cut to %u bytes", s, n);
            if (!run(d.data(), n, what, false)) return 1;
        }
        std::vector<uint8_t> m;
        for (int i = 0; i < MUTATIONS; ++i) {
            m = d;
            const int burst = i % 2 ? 1 + (int)(rnd() % 4) : 1;
            const uint32_t at = rnd() % len;
            for (int j = 0; j < burst && at + j < len; ++j) m[at + j] = (i % 8 == 7) ? 0xFF : (uint8_t)rnd();
            snprintf(what, sizeof(what), "stream %u mutation %d at byte %u", s, i, at);
            if (!run(m.data(), len, what, false)) return 1;
        }
    }
    fclose(f);
    printf("jpeg_parse_main: %u streams, %ld calls, %ld decoded, %ld refused, no failure\n", count, n_calls, n_ok, n_refused);
    return 0;
}
