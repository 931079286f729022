// Stand-alone check of rtm3d_jpeg_encode_bound and of the writes of rtm3d_jpeg_entropy_encode (rtm3d_amd/csrc/jpeg_host.cpp, the
// only other file it links), in the manner of jpeg_parse_main.cpp.
//
// For a list of sizes x the four modes x restart intervals 0, 1 and 3, adversarial coefficient buffers are encoded into an
// output that stands between canaries of 64 bytes:
//   kind 0  every AC coefficient +-1023 with alternating signs, DC alternating +-1016 (every DC difference has category 11);
//   kind 1  every AC coefficient +1023 - ten 1-bits behind a code that begins with nine - so that the stream is full of 0xFF
//           bytes, each followed by a stuffed 0x00; DC as above;
//   kind 2  every AC coefficient -1023, DC +-1016 the other way round.
// The coefficient buffer is an allocation of exactly coef_count values.  Required: the call succeeds, *bytes <= the bound, no
// canary changes, the stream decodes (rtm3d_jpeg_entropy_decode) to the same values on every real block; a capacity of
// bound - 1 is refused and leaves the output untouched; kind 1 stuffed at least one byte per block.  Exit status 0 and a line
// of counts, or 1 and the first failure.
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

enum { CANARY = 64, CANARY_BYTE = 0xC7 };

static int fail(const char* what, int h, int w, int mode, int restart, int kind) {
    printf("FAILED: %s (%d x %d, mode %d, restart %d, kind %d)\n", what, h, w, mode, restart, kind);
    return 1;
}

int main() {
    static const int sizes[][2] = {{1, 1}, {8, 8}, {9, 17}, {16, 16}, {17, 33}, {20, 40}, {37, 53}, {72, 136}};
    static const int restarts[] = {0, 1, 3};
    unsigned long long cases = 0, stuffed_total = 0;
    double max_fill = 0;
    for (const auto& hw : sizes) {
        for (int mode = RTM3D_JPEG_GREY; mode <= RTM3D_JPEG_420; ++mode) {
            const int h = hw[0], w = hw[1];
            rtm3d_jpeg_stream_info I;
            if (rtm3d_jpeg_frame_layout(h, w, mode, &I)) return fail("frame_layout", h, w, mode, 0, 0);
            for (int restart : restarts) {
                size_t bound = 0;
                if (rtm3d_jpeg_encode_bound(h, w, mode, restart, &bound)) return fail("encode_bound", h, w, mode, restart, 0);
                for (int kind = 0; kind < 3; ++kind) {
                    std::vector<int16_t> coef(I.coef_count);                   // exactly: a read past it is a sanitizer's catch
                    for (int k = 0; k < 192; ++k) coef[k] = k < 64 * I.components ? (int16_t)(1 + ((k < 128 ? k : k - 64) * 37) % 255) : 0;   // Cb and Cr share a table
                    for (size_t i = 192; i < I.coef_count; ++i) {
                        const size_t blk = (i - 192) / 64, k = i % 64;
                        if (k == 0) coef[i] = (int16_t)(((blk & 1) != (size_t)(kind == 2)) ? 1016 : -1016);
                        else coef[i] = (int16_t)(kind == 1 ? 1023 : kind == 2 ? -1023 : (k & 1) ? 1023 : -1023);
                    }
                    std::vector<uint8_t> out(CANARY + bound + CANARY, CANARY_BYTE);
                    size_t bytes = 0;
                    // one byte short: refused, nothing written
                    if (rtm3d_jpeg_entropy_encode(coef.data(), h, w, mode, restart, out.data() + CANARY, bound - 1, &bytes) != 1)
                        return fail("a capacity of bound - 1 was not refused", h, w, mode, restart, kind);
                    for (uint8_t b : out)
                        if (b != CANARY_BYTE) return fail("a refused call wrote", h, w, mode, restart, kind);
                    if (rtm3d_jpeg_entropy_encode(coef.data(), h, w, mode, restart, out.data() + CANARY, bound, &bytes) != 0)
                        return fail("the encode was refused", h, w, mode, restart, kind);
                    if (bytes > bound) return fail("the stream is longer than the bound", h, w, mode, restart, kind);
                    for (size_t i = 0; i < CANARY; ++i)
                        if (out[i] != CANARY_BYTE || out[CANARY + bound + i] != CANARY_BYTE) return fail("a canary changed", h, w, mode, restart, kind);
                    for (size_t i = CANARY + bytes; i < CANARY + bound; ++i)
                        if (out[i] != CANARY_BYTE) return fail("bytes behind the stream were written", h, w, mode, restart, kind);
                    if ((double)bytes / (double)bound > max_fill) max_fill = (double)bytes / (double)bound;
                    size_t stuffed = 0;
                    for (size_t i = CANARY; i + 1 < CANARY + bytes; ++i) stuffed += out[i] == 0xFF && out[i + 1] == 0x00;
                    const size_t blocks = (I.coef_count - 192) / 64;
                    if (kind == 1 && stuffed < blocks) return fail("no stuffed bytes", h, w, mode, restart, kind);
                    stuffed_total += stuffed;
                    // and back: the decoder finds the same values on every real block
                    std::vector<int16_t> back(I.coef_count, 0x5A5A);
                    if (rtm3d_jpeg_entropy_decode(out.data() + CANARY, bytes, back.data(), back.size()) != 0) return fail("the stream does not decode", h, w, mode, restart, kind);
                    const int H = I.bw[0] / I.mcus_x, V = I.bh[0] / I.mcus_y;
                    for (int c = 0; c < I.components; ++c) {
                        const int hc = c == 0 ? H : 1, vc = c == 0 ? V : 1;
                        const int rw = ((w * hc + H - 1) / H + 7) / 8, rh = ((h * vc + V - 1) / V + 7) / 8;
                        for (int by = 0; by < rh; ++by)
                            for (int bx = 0; bx < rw; ++bx) {
                                const size_t at = I.plane_offset[c] + ((size_t)by * I.bw[c] + bx) * 64;
                                if (memcmp(&coef[at], &back[at], 128) != 0) return fail("a real block came back different", h, w, mode, restart, kind);
                            }
                    }
                    if (memcmp(coef.data(), back.data(), 64 * I.components * sizeof(int16_t)) != 0) return fail("the tables came back different", h, w, mode, restart, kind);
                    ++cases;
                }
            }
        }
    }
    // what the bound refuses
    size_t n = 0;
    if (rtm3d_jpeg_encode_bound(8, 8, 4, 0, &n) != 1 || rtm3d_jpeg_encode_bound(0, 8, 0, 0, &n) != 1 || rtm3d_jpeg_encode_bound(8, 16385, 0, 0, &n) != 1 ||
        rtm3d_jpeg_encode_bound(8, 8, 0, 65536, &n) != 1 || rtm3d_jpeg_encode_bound(8, 8, 0, -1, &n) != 1 || rtm3d_jpeg_encode_bound(8, 8, 0, 0, NULL) != 1)
        return fail("a bad argument of encode_bound was accepted", 0, 0, 0, 0, 0);
    printf("%llu cases, fullest stream %.3f of its bound, %llu stuffed bytes, no failure\n", cases, max_fill, stuffed_total);
    return 0;
}
