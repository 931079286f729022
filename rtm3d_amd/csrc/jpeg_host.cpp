// JPEG frames, host side (include/rtm3d_hip.h, "JPEG frames"): the parser of the accepted baseline streams and the Huffman
// decoder that fills a frame's coefficient buffer.  Plain C++17, no HIP header, no global state: every function here may run
// on several threads at once (rtm3d_frames_jpeg does that), and reports through a message buffer of the caller; only the
// extern "C" wrappers touch the library's error string.
//
// Safety.  Every read of the stream goes through a position that is compared with `bytes` (the marker walk) or with the end of
// a segment whose length was compared with `bytes` first; the bit reader feeds zeros once it meets a marker or the end of the
// data and counts them, and a block that consumed one of those zeros is refused.  Every write goes to plane + block * 64 +
// natural index with block inside the component's padded grid, below coef_count <= capacity by construction.
//
// Speed.  A Huffman symbol is one lookup of the next 9 bits (length and symbol in a 512-entry table per Huffman table; longer
// codes, rare by design of the code, walk the canonical maxcode list from 10 bits on), fed from a 64-bit accumulator that is
// refilled once per symbol-and-value pair.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rtm3d_hip.h"

extern void rt_set_error(const char* fmt, ...);

#define JPEG_MAX_SIDE 16384
#define JPEG_LOOK 9
#define JFAIL(...) do { snprintf(msg, msg_len, __VA_ARGS__); return 1; } while (0)

namespace {

const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU-T T.81 Annex K, tables K.3 - K.6: the 16 code counts, then the symbols in code order
const uint8_t kStdDcLumaCounts[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kStdDcChromaCounts[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kStdDcSymbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kStdAcLumaCounts[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
const uint8_t kStdAcLumaSymbols[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209,
    240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
    71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
    122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
    168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
    213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248,
    249, 250};
const uint8_t kStdAcChromaCounts[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
const uint8_t kStdAcChromaSymbols[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82,
    240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68,
    69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
    120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
    165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
    210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247,
    248, 249, 250};

struct Huff {
    bool defined;
    uint16_t look[1 << JPEG_LOOK];       // length << 8 | symbol of the code the 9 bits begin with; 0: a longer code, or none
    int32_t maxcode[17];                 // largest code of a length, -1 when the length has none
    int32_t valoff[17];                  // index of a length's first symbol minus its first code
    uint8_t sym[256];
};

// a table from its counts and n symbols; false when the counts do not describe a prefix code
bool huff_build(Huff& H, const uint8_t counts[16], const uint8_t* symbols, int n) {
    memset(&H, 0, sizeof(H));
    int total = 0;
    for (int i = 0; i < 16; ++i) total += counts[i];
    if (total != n || n > 256) return false;
    memcpy(H.sym, symbols, (size_t)n);
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        H.valoff[len] = k - code;
        for (int i = 0; i < counts[len - 1]; ++i, ++code, ++k) {
            if (len <= JPEG_LOOK) {
                const int first = code << (JPEG_LOOK - len), span = 1 << (JPEG_LOOK - len);
                if (first + span > (1 << JPEG_LOOK)) return false;
                for (int j = 0; j < span; ++j) H.look[first + j] = (uint16_t)((len << 8) | symbols[k]);
            }
        }
        H.maxcode[len] = counts[len - 1] ? code - 1 : -1;
        if (code > (1 << len)) return false;
        code <<= 1;
    }
    H.defined = true;
    return true;
}

struct Parsed {
    rtm3d_jpeg_stream_info info;
    uint16_t q[4][64];                   // natural order
    bool q_defined[4];
    Huff huff[2][4];                     // [class: 0 DC, 1 AC][id]
    int tq[3], td[3], ta[3];             // per component
    int hs[3], vs[3];                    // sampling as decoded (grey: 1 x 1)
    size_t scan;                         // first byte of the entropy-coded data
};

void fill_layout(rtm3d_jpeg_stream_info& I) {
    const int H = I.mode == RTM3D_JPEG_422 || I.mode == RTM3D_JPEG_420 ? 2 : 1, V = I.mode == RTM3D_JPEG_420 ? 2 : 1;
    I.mcus_x = (I.w + 8 * H - 1) / (8 * H);
    I.mcus_y = (I.h + 8 * V - 1) / (8 * V);
    size_t at = 192;
    for (int c = 0; c < 3; ++c) {
        I.table_offset[c] = (size_t)64 * c;
        I.bw[c] = I.bh[c] = 0;
        I.plane_offset[c] = at;
        if (c >= I.components) continue;
        I.bw[c] = I.mcus_x * (c == 0 ? H : 1);
        I.bh[c] = I.mcus_y * (c == 0 ? V : 1);
        at += (size_t)I.bw[c] * I.bh[c] * 64;
    }
    I.coef_count = at;
}

const char* sof_name(int m) {
    if (m == 0xC2) return "progressive coding (SOF2)";
    if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) return "lossless coding";
    if (m == 0xC5 || m == 0xC6 || m == 0xDE) return "hierarchical coding";
    return "arithmetic coding";          // SOF9, SOF10, SOF13, SOF14, DAC
}

// the headers up to and including SOS
int parse(const uint8_t* d, size_t bytes, Parsed& P, char* msg, size_t msg_len) {
    memset(&P.info, 0, sizeof(P.info));
    memset(P.q_defined, 0, sizeof(P.q_defined));
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 4; ++i) P.huff[t][i].defined = false;
    if (!d) JFAIL("null pointer");
    if (bytes < 4 || d[0] != 0xFF || d[1] != 0xD8) JFAIL("no SOI marker: not a JPEG stream");
    size_t pos = 2;
    bool have_frame = false;
    int comp_id[3] = {0, 0, 0};
    for (;;) {
        if (pos + 2 > bytes) JFAIL("the stream ends before its scan (no SOS)");
        if (d[pos] != 0xFF) JFAIL("byte 0x%02X at offset %zu where a marker must stand", d[pos], pos);
        while (pos + 1 < bytes && d[pos + 1] == 0xFF) ++pos;           // fill bytes
        if (pos + 2 > bytes) JFAIL("the stream ends before its scan (no SOS)");
        const int m = d[pos + 1];
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;           // markers without a segment
        if (m == 0xD8) JFAIL("a second SOI: several frames");
        if (m == 0xD9) JFAIL("EOI before any scan");
        if (m == 0x00) JFAIL("byte 0xFF00 at offset %zu where a marker must stand", pos - 2);
        if (pos + 2 > bytes) JFAIL("segment length of marker 0x%02X runs past the end of the buffer", m);
        const size_t L = ((size_t)d[pos] << 8) | d[pos + 1];
        if (L < 2 || L > bytes - pos) JFAIL("segment length %zu of marker 0x%02X runs past the end of the buffer", L, m);
        const uint8_t* s = d + pos + 2;                                // the segment's body, n bytes
        const size_t n = L - 2;
        pos += L;
        if (m == 0xC0 || m == 0xC1) {
            if (have_frame) JFAIL("a second SOF: several frames");
            if (n < 6) JFAIL("SOF segment of %zu bytes", n);
            const int prec = s[0], h = (s[1] << 8) | s[2], w = (s[3] << 8) | s[4], nf = s[5];
            if (prec == 12) JFAIL("12-bit sample precision");
            if (prec != 8) JFAIL("sample precision %d, not 8", prec);
            if (h == 0 || w == 0 || h > JPEG_MAX_SIDE || w > JPEG_MAX_SIDE) JFAIL("a frame of %d x %d; a side must lie in 1..%d", h, w, JPEG_MAX_SIDE);
            if (nf != 1 && nf != 3) JFAIL("%d components; 1 (grey) or 3 (Y Cb Cr)", nf);
            if (n != (size_t)(6 + 3 * nf)) JFAIL("SOF segment of %zu bytes for %d components", n, nf);
            for (int c = 0; c < nf; ++c) {
                comp_id[c] = s[6 + 3 * c];
                P.hs[c] = s[7 + 3 * c] >> 4; P.vs[c] = s[7 + 3 * c] & 15; P.tq[c] = s[8 + 3 * c];
                if (P.hs[c] < 1 || P.hs[c] > 4 || P.vs[c] < 1 || P.vs[c] > 4) JFAIL("component %d has the sampling factors %d x %d", c, P.hs[c], P.vs[c]);
                if (P.tq[c] > 3) JFAIL("component %d names the quantisation table %d", c, P.tq[c]);
            }
            int mode = RTM3D_JPEG_GREY;
            if (nf == 1) {
                P.hs[0] = P.vs[0] = 1;                                 // a single component is not interleaved: one block per MCU
            } else {
                const bool chroma_1x1 = P.hs[1] == 1 && P.vs[1] == 1 && P.hs[2] == 1 && P.vs[2] == 1;
                if (chroma_1x1 && P.hs[0] == 1 && P.vs[0] == 1) mode = RTM3D_JPEG_444;
                else if (chroma_1x1 && P.hs[0] == 2 && P.vs[0] == 1) mode = RTM3D_JPEG_422;
                else if (chroma_1x1 && P.hs[0] == 2 && P.vs[0] == 2) mode = RTM3D_JPEG_420;
                else JFAIL("sampling %dx%d %dx%d %dx%d; luma 1x1, 2x1 or 2x2 over chroma 1x1", P.hs[0], P.vs[0], P.hs[1], P.vs[1], P.hs[2], P.vs[2]);
            }
            P.info.h = h; P.info.w = w; P.info.components = nf; P.info.mode = mode;
            have_frame = true;
        } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8) || m == 0xDE) {
            JFAIL("%s", sof_name(m));
        } else if (m == 0xC4) {
            size_t p = 0;
            while (p < n) {
                if (n - p < 17) JFAIL("DHT segment ends inside a table");
                const int tc = s[p] >> 4, th = s[p] & 15;
                if (tc > 1 || th > 3) JFAIL("DHT defines table class %d id %d", tc, th);
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += s[p + 1 + i];
                if (cnt > 256 || n - p - 17 < (size_t)cnt) JFAIL("DHT segment ends inside a table");
                if (!huff_build(P.huff[tc][th], s + p + 1, s + p + 17, cnt)) JFAIL("DHT: the code counts of table class %d id %d describe no prefix code", tc, th);
                p += 17 + (size_t)cnt;
            }
        } else if (m == 0xDB) {
            size_t p = 0;
            while (p < n) {
                const int pq = s[p] >> 4, tq = s[p] & 15;
                if (pq > 1 || tq > 3) JFAIL("DQT defines table %d with precision %d", tq, pq);
                const size_t need = pq ? 128 : 64;
                if (n - p - 1 < need) JFAIL("DQT segment ends inside a table");
                for (int i = 0; i < 64; ++i)
                    P.q[tq][kZigzag[i]] = pq ? (uint16_t)((s[p + 1 + 2 * i] << 8) | s[p + 2 + 2 * i]) : (uint16_t)s[p + 1 + i];
                P.q_defined[tq] = true;
                p += 1 + need;
            }
        } else if (m == 0xDD) {
            if (n != 2) JFAIL("DRI segment of %zu bytes", n);
            P.info.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0 && s[11] == 0) JFAIL("Adobe APP14 segment with transform 0 (RGB or CMYK samples, not Y Cb Cr)");
        } else if (m == 0xDA) {
            if (!have_frame) JFAIL("SOS before SOF");
            if (n < 1) JFAIL("SOS segment of %zu bytes", n);
            const int ns = s[0];
            if (ns != P.info.components) JFAIL("a scan of %d of the %d components: several scans", ns, P.info.components);
            if (n != (size_t)(4 + 2 * ns)) JFAIL("SOS segment of %zu bytes for %d components", n, ns);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) JFAIL("the scan names component %d where the frame has %d", s[1 + 2 * c], comp_id[c]);
                P.td[c] = s[2 + 2 * c] >> 4; P.ta[c] = s[2 + 2 * c] & 15;
                if (P.td[c] > 3 || P.ta[c] > 3) JFAIL("component %d names the Huffman tables %d / %d", c, P.td[c], P.ta[c]);
            }
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahal = s[3 + 2 * ns];
            if (ss != 0 || se != 63 || ahal != 0) JFAIL("a scan with Ss %d Se %d Ah/Al 0x%02X: a progressive scan", ss, se, ahal);
            for (int c = 0; c < ns; ++c) {
                if (!P.q_defined[P.tq[c]]) JFAIL("quantisation table %d of component %d was never defined", P.tq[c], c);
                for (int t = 0; t < 2; ++t) {
                    const int id = t ? P.ta[c] : P.td[c];
                    Huff& H = P.huff[t][id];
                    if (H.defined) continue;
                    if (id > 1) JFAIL("%s Huffman table %d of component %d was never defined (Annex K has tables 0 and 1)", t ? "AC" : "DC", id, c);
                    if (!t) huff_build(H, id ? kStdDcChromaCounts : kStdDcLumaCounts, kStdDcSymbols, 12);
                    else huff_build(H, id ? kStdAcChromaCounts : kStdAcLumaCounts, id ? kStdAcChromaSymbols : kStdAcLumaSymbols, 162);
                }
            }
            P.scan = pos;
            fill_layout(P.info);
            return 0;
        }
        // everything else (APPn, COM, DNL, EXP, reserved): skipped
    }
}

struct Bits {
    const uint8_t* d;
    size_t pos, end;
    uint64_t acc;                        // the low n bits are unread
    int n;
    int fake;                            // how many of them are zeros fed behind a marker or the end of the data (the last ones)

    inline void fill() {
        while (n <= 56) {
            unsigned b = 0;
            if (pos < end && d[pos] != 0xFF) {
                b = d[pos++];
            } else if (pos + 1 < end && d[pos + 1] == 0x00) {          // a stuffed 0xFF
                b = 0xFF; pos += 2;
            } else {
                fake += 8;                                             // a marker, or the end: pos stays
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
};

// one symbol; -1 when the bits are no code of the table.  The caller has filled the reader.
inline int huff_symbol(Bits& b, const Huff& H) {
    const unsigned e = H.look[b.peek(JPEG_LOOK)];
    if (e) { b.n -= (int)(e >> 8); return (int)(e & 255u); }
    for (int len = JPEG_LOOK + 1; len <= 16; ++len) {
        const int32_t code = (int32_t)b.peek(len);
        if (code <= H.maxcode[len]) { b.n -= len; return H.sym[(code + H.valoff[len]) & 255]; }
    }
    return -1;
}

// s bits (1..15) as the signed value they stand for
inline int receive_extend(Bits& b, int s) {
    const int v = (int)b.peek(s);
    b.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

int decode_scan(const uint8_t* d, size_t bytes, const Parsed& P, int16_t* coef, char* msg, size_t msg_len) {
    const rtm3d_jpeg_stream_info& I = P.info;
    memset(coef, 0, I.coef_count * sizeof(int16_t));
    for (int c = 0; c < I.components; ++c) memcpy(coef + I.table_offset[c], P.q[P.tq[c]], 64 * sizeof(uint16_t));
    Bits b = {d, P.scan, bytes, 0, 0, 0};
    const int n_mcu = I.mcus_x * I.mcus_y, ri = I.restart_interval;
    uint32_t pred[3] = {0, 0, 0};
    int rst = 0, mx = 0, my = 0;
    for (int mcu = 0; mcu < n_mcu; ++mcu) {
        if (ri && mcu && mcu % ri == 0) {
            // what is left of the last byte is padding; a whole unread byte in front of the marker is not
            if ((b.n - b.fake) / 8 > 0) JFAIL("restart marker RST%d missing: entropy-coded data goes on behind MCU %d", rst, mcu - 1);
            b.acc = 0; b.n = 0; b.fake = 0;
            size_t p = b.pos;
            if (p + 2 > bytes || d[p] != 0xFF) JFAIL("restart marker RST%d missing behind MCU %d", rst, mcu - 1);
            while (p + 2 < bytes && d[p + 1] == 0xFF) ++p;
            if (d[p + 1] != 0xD0 + rst) JFAIL("restart marker RST%d missing or out of sequence behind MCU %d (found marker 0x%02X)", rst, mcu - 1, d[p + 1]);
            b.pos = p + 2;
            rst = (rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < I.components; ++c) {
            const Huff& dc = P.huff[0][P.td[c]];
            const Huff& ac = P.huff[1][P.ta[c]];
            for (int v = 0; v < P.vs[c]; ++v) {
                for (int u = 0; u < P.hs[c]; ++u) {
                    int16_t* blk = coef + I.plane_offset[c] + ((size_t)(my * P.vs[c] + v) * I.bw[c] + (size_t)(mx * P.hs[c] + u)) * 64;
                    b.fill();
                    int s = huff_symbol(b, dc);
                    if (s < 0) JFAIL("a Huffman code that is not in DC table %d (MCU %d)", P.td[c], mcu);
                    if (s > 15) JFAIL("a DC coefficient of %d bits (MCU %d)", s, mcu);
                    if (s) pred[c] += (uint32_t)receive_extend(b, s);
                    blk[0] = (int16_t)(uint16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        b.fill();
                        const int rs = huff_symbol(b, ac);
                        if (rs < 0) JFAIL("a Huffman code that is not in AC table %d (MCU %d)", P.ta[c], mcu);
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;                        // end of block
                            k += 16;
                            if (k > 64) JFAIL("a zero run that passes coefficient 63 (MCU %d)", mcu);
                            continue;
                        }
                        k += r;
                        if (k > 63) JFAIL("a zero run that passes coefficient 63 (MCU %d)", mcu);
                        blk[kZigzag[k]] = (int16_t)receive_extend(b, s);
                        ++k;
                    }
                    if (b.n < b.fake) JFAIL("the entropy-coded data ends before the last MCU (in MCU %d of %d)", mcu, n_mcu);
                }
            }
        }
        if (++mx == I.mcus_x) { mx = 0; ++my; }
    }
    // behind the scan: EOI, nothing at all, or bytes nobody reads - but not one more scan
    size_t p = b.pos;
    while (p + 1 < bytes) {
        if (d[p] != 0xFF) { ++p; continue; }
        const int m = d[p + 1];
        if (m == 0xD9) break;
        if (m == 0xDA) JFAIL("a second SOS: several scans");
        if (m == 0x00 || m == 0xFF || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { p += (m == 0xFF) ? 1 : 2; continue; }
        if (p + 4 > bytes) break;
        const size_t L = ((size_t)d[p + 2] << 8) | d[p + 3];           // a segment between scans (tables for the next one)
        if (L < 2 || L > bytes - (p + 2)) break;
        p += 2 + L;
    }
    return 0;
}

}  // namespace

// ---- the library's own callers (jpeg.hip, engine.cpp): the same two steps with the refusal in msg
int rt_jpeg_info(const uint8_t* data, size_t bytes, rtm3d_jpeg_stream_info* out, char* msg, size_t msg_len) {
    Parsed* P = new Parsed;
    const int rc = parse(data, bytes, *P, msg, msg_len);
    if (!rc) *out = P->info;
    delete P;
    return rc;
}

int rt_jpeg_entropy_decode(const uint8_t* data, size_t bytes, int16_t* h_coef, size_t capacity, char* msg, size_t msg_len) {
    Parsed* P = new Parsed;
    int rc = parse(data, bytes, *P, msg, msg_len);
    if (!rc && !h_coef) { snprintf(msg, msg_len, "null pointer"); rc = 1; }
    if (!rc && capacity < P->info.coef_count) {
        snprintf(msg, msg_len, "the coefficient buffer holds %zu int16, the frame needs %zu", capacity, P->info.coef_count);
        rc = 1;
    }
    if (!rc) rc = decode_scan(data, bytes, *P, h_coef, msg, msg_len);
    delete P;
    return rc;
}

extern "C" int rtm3d_jpeg_info(const uint8_t* data, size_t bytes, rtm3d_jpeg_stream_info* out) {
    char msg[200];
    if (!out) { rt_set_error("jpeg_info: null pointer"); return 1; }
    if (rt_jpeg_info(data, bytes, out, msg, sizeof(msg))) { rt_set_error("jpeg_info: %s", msg); return 1; }
    return 0;
}

extern "C" int rtm3d_jpeg_entropy_decode(const uint8_t* data, size_t bytes, int16_t* h_coef, size_t capacity) {
    char msg[200];
    if (rt_jpeg_entropy_decode(data, bytes, h_coef, capacity, msg, sizeof(msg))) { rt_set_error("jpeg_entropy_decode: %s", msg); return 1; }
    return 0;
}

extern "C" int rtm3d_jpeg_workspace_bytes(int B, const uint8_t* const* h_data, const size_t* h_bytes, size_t* bytes) {
    char msg[200];
    if (B < 1) { rt_set_error("jpeg_workspace_bytes: B = %d", B); return 1; }
    if (!h_data || !h_bytes || !bytes) { rt_set_error("jpeg_workspace_bytes: null pointer"); return 1; }
    size_t total = 0;
    for (int b = 0; b < B; ++b) {
        rtm3d_jpeg_stream_info I;
        if (rt_jpeg_info(h_data[b], h_bytes[b], &I, msg, sizeof(msg))) { rt_set_error("jpeg_workspace_bytes: frame %d: %s", b, msg); return 1; }
        total += I.coef_count * sizeof(int16_t);
    }
    *bytes = total;
    return 0;
}

// ==================================================================== JPEG encoding, host side (include/rtm3d_hip.h, "JPEG encoding")
// The quality tables, the size bound and the Huffman encoder that turns a frame's coefficient buffer - what the device stage
// (jpeg_enc.hip) wrote - into a baseline stream with libjpeg's marker layout.  Host only, no global state, thread-safe.
//
// Safety.  The encoder refuses a capacity below rtm3d_jpeg_encode_bound before it writes a byte; the bound's derivation (in the
// header) covers every coefficient buffer that passes the category checks, so no write needs a check of its own - one is made
// per block all the same.  Reads: the two tables and plane + block * 64 + k with the block inside the component's REAL grid,
// below coef_count by construction.
namespace {

const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

#define JPEG_ENC_BLOCK_BYTES 416         // the most one block adds to the stream, stuffing included (see the header)

struct EncHuff { uint16_t code[256]; uint8_t len[256]; };

void enc_build(EncHuff& T, const uint8_t counts[16], const uint8_t* symbols) {
    memset(&T, 0, sizeof(T));
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < counts[len - 1]; ++i, ++code, ++k) { T.code[symbols[k]] = (uint16_t)code; T.len[symbols[k]] = (uint8_t)len; }
        code <<= 1;
    }
}

struct EncOut {
    uint8_t* p;
    uint64_t acc;                        // the low n bits are not written yet
    int n;                               // 0..7 between calls

    inline void put(uint32_t bits, int len) {                              // len <= 16 + 11
        acc = (acc << len) | bits;
        n += len;
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            *p++ = b;
            if (b == 0xFF) *p++ = 0;
            n -= 8;
        }
    }
    inline void flush() { if (n) put((1u << (8 - n)) - 1u, 8 - n); }      // the last byte is padded with 1-bits
};

inline int category(int v) { const unsigned a = (unsigned)(v < 0 ? -v : v); return a ? 32 - __builtin_clz(a) : 0; }

uint8_t* put_segment(uint8_t* p, int marker, const uint8_t* body, size_t n) {
    *p++ = 0xFF; *p++ = (uint8_t)marker; *p++ = (uint8_t)((n + 2) >> 8); *p++ = (uint8_t)((n + 2) & 255);
    memcpy(p, body, n);
    return p + n;
}

int enc_frame_info(int h, int w, int mode, rtm3d_jpeg_stream_info& I, char* msg, size_t msg_len) {
    if (mode < RTM3D_JPEG_GREY || mode > RTM3D_JPEG_420) JFAIL("the unknown mode %d", mode);
    if (h < 1 || w < 1 || h > JPEG_MAX_SIDE || w > JPEG_MAX_SIDE) JFAIL("a frame of %d x %d; a side must lie in 1..%d", h, w, JPEG_MAX_SIDE);
    memset(&I, 0, sizeof(I));
    I.h = h; I.w = w; I.mode = mode; I.components = mode == RTM3D_JPEG_GREY ? 1 : 3;
    fill_layout(I);
    return 0;
}

size_t enc_header_bytes(int components, int restart) {
    const size_t nt = components == 3 ? 2 : 1;
    return 2 + 18 + 69 * nt + (10 + 3 * (size_t)components) + (33 + 183) * nt + (restart ? 6 : 0) + (8 + 2 * (size_t)components);
}

}  // namespace

int rt_jpeg_frame_layout(int h, int w, int mode, rtm3d_jpeg_stream_info* out, char* msg, size_t msg_len) {
    return enc_frame_info(h, w, mode, *out, msg, msg_len);
}

int rt_jpeg_encode_bound(int h, int w, int mode, int restart, size_t* bytes, char* msg, size_t msg_len) {
    rtm3d_jpeg_stream_info I;
    if (enc_frame_info(h, w, mode, I, msg, msg_len)) return 1;
    if (restart < 0 || restart > 65535) JFAIL("a restart interval of %d MCUs; 0 (none) .. 65535", restart);
    const size_t mcus = (size_t)I.mcus_x * I.mcus_y;
    const size_t per_mcu = (size_t)(I.bw[0] / I.mcus_x) * (size_t)(I.bh[0] / I.mcus_y) + (I.components == 3 ? 2 : 0);
    const size_t n_rst = restart ? (mcus - 1) / (size_t)restart : 0;
    *bytes = enc_header_bytes(I.components, restart) + JPEG_ENC_BLOCK_BYTES * mcus * per_mcu + 2 * n_rst + 2;
    return 0;
}

int rt_jpeg_entropy_encode(const int16_t* h_coef, int h, int w, int mode, int restart, uint8_t* out, size_t capacity, size_t* bytes, char* msg,
                           size_t msg_len) {
    rtm3d_jpeg_stream_info I;
    size_t bound = 0;
    if (rt_jpeg_encode_bound(h, w, mode, restart, &bound, msg, msg_len)) return 1;
    if (!h_coef || !out || !bytes) JFAIL("null pointer");
    if (capacity < bound) JFAIL("the output holds %zu bytes, a stream of this frame may need %zu (rtm3d_jpeg_encode_bound)", capacity, bound);
    enc_frame_info(h, w, mode, I, msg, msg_len);
    const int nt = I.components == 3 ? 2 : 1, H = I.bw[0] / I.mcus_x, V = I.bh[0] / I.mcus_y;
    for (int t = 0; t < nt; ++t)
        for (int k = 0; k < 64; ++k) {
            const unsigned q = (uint16_t)h_coef[64 * t + k];
            if (q < 1 || q > 255) JFAIL("entry %d of quantisation table %d is %u; a baseline table holds 1..255", k, t, q);
        }
    EncHuff dc[2], ac[2];
    enc_build(dc[0], kStdDcLumaCounts, kStdDcSymbols); enc_build(ac[0], kStdAcLumaCounts, kStdAcLumaSymbols);
    enc_build(dc[1], kStdDcChromaCounts, kStdDcSymbols); enc_build(ac[1], kStdAcChromaCounts, kStdAcChromaSymbols);
    // ---- the headers, in libjpeg's order: SOI APP0 DQT.. SOF0 DHT.. [DRI] SOS
    uint8_t* p = out;
    uint8_t body[200];
    *p++ = 0xFF; *p++ = 0xD8;
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    p = put_segment(p, 0xE0, jfif, sizeof(jfif));
    for (int t = 0; t < nt; ++t) {
        body[0] = (uint8_t)t;
        for (int i = 0; i < 64; ++i) body[1 + i] = (uint8_t)h_coef[64 * t + kZigzag[i]];
        p = put_segment(p, 0xDB, body, 65);
    }
    body[0] = 8; body[1] = (uint8_t)(h >> 8); body[2] = (uint8_t)(h & 255); body[3] = (uint8_t)(w >> 8); body[4] = (uint8_t)(w & 255);
    body[5] = (uint8_t)I.components;
    for (int c = 0; c < I.components; ++c) {
        body[6 + 3 * c] = (uint8_t)(c + 1);
        body[7 + 3 * c] = (uint8_t)(c == 0 && I.components == 3 ? (H << 4) | V : 0x11);
        body[8 + 3 * c] = (uint8_t)(c ? 1 : 0);
    }
    p = put_segment(p, 0xC0, body, 6 + 3 * (size_t)I.components);
    for (int t = 0; t < nt; ++t) {
        body[0] = (uint8_t)t;
        memcpy(body + 1, t ? kStdDcChromaCounts : kStdDcLumaCounts, 16); memcpy(body + 17, kStdDcSymbols, 12);
        p = put_segment(p, 0xC4, body, 29);
        body[0] = (uint8_t)(0x10 | t);
        memcpy(body + 1, t ? kStdAcChromaCounts : kStdAcLumaCounts, 16); memcpy(body + 17, t ? kStdAcChromaSymbols : kStdAcLumaSymbols, 162);
        p = put_segment(p, 0xC4, body, 179);
    }
    if (restart) { body[0] = (uint8_t)(restart >> 8); body[1] = (uint8_t)(restart & 255); p = put_segment(p, 0xDD, body, 2); }
    body[0] = (uint8_t)I.components;
    for (int c = 0; c < I.components; ++c) { body[1 + 2 * c] = (uint8_t)(c + 1); body[2 + 2 * c] = (uint8_t)(c ? 0x11 : 0x00); }
    body[1 + 2 * I.components] = 0; body[2 + 2 * I.components] = 63; body[3 + 2 * I.components] = 0;
    p = put_segment(p, 0xDA, body, 4 + 2 * (size_t)I.components);
    // ---- the scan
    int rw[3], rh[3];                                                       // the REAL block grid of every component
    for (int c = 0; c < I.components; ++c) {
        const int hc = c == 0 ? H : 1, vc = c == 0 ? V : 1;
        rw[c] = (((w * hc + H - 1) / H) + 7) / 8; rh[c] = (((h * vc + V - 1) / V) + 7) / 8;
    }
    EncOut o = {p, 0, 0};
    const uint8_t* const end = out + capacity;
    const int n_mcu = I.mcus_x * I.mcus_y;
    int pred[3] = {0, 0, 0}, rst = 0, mx = 0, my = 0;
    for (int mcu = 0; mcu < n_mcu; ++mcu) {
        if (restart && mcu && mcu % restart == 0) {
            o.flush();
            *o.p++ = 0xFF; *o.p++ = (uint8_t)(0xD0 + rst);
            rst = (rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < I.components; ++c) {
            const int hc = c == 0 ? H : 1, vc = c == 0 ? V : 1, t = c ? 1 : 0;
            for (int v = 0; v < vc; ++v) {
                for (int u = 0; u < hc; ++u) {
                    if ((size_t)(end - o.p) < JPEG_ENC_BLOCK_BYTES) JFAIL("the output is full at MCU %d (a bound that does not hold)", mcu);
                    const int bx = mx * hc + u, by = my * vc + v;
                    if (bx >= rw[c] || by >= rh[c]) {                       // a padding block: difference 0, end of block; the buffer is not read
                        o.put(dc[t].code[0], dc[t].len[0]);
                        o.put(ac[t].code[0], ac[t].len[0]);
                        continue;
                    }
                    const int16_t* blk = h_coef + I.plane_offset[c] + ((size_t)by * I.bw[c] + (size_t)bx) * 64;
                    const int diff = (int)blk[0] - pred[c];
                    pred[c] = blk[0];
                    int s = category(diff);
                    if (s > 11) JFAIL("a DC difference of %d (MCU %d, component %d): category %d, baseline has 0..11", diff, mcu, c, s);
                    o.put(dc[t].code[s], dc[t].len[s]);
                    if (s) o.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
                    int run = 0;
                    for (int k = 1; k < 64; ++k) {
                        const int a = blk[kZigzag[k]];
                        if (a == 0) { ++run; continue; }
                        for (; run > 15; run -= 16) o.put(ac[t].code[0xF0], ac[t].len[0xF0]);
                        s = category(a);
                        if (s > 10) JFAIL("an AC coefficient of %d (MCU %d, component %d): category %d, baseline has 1..10", a, mcu, c, s);
                        o.put(ac[t].code[(run << 4) | s], ac[t].len[(run << 4) | s]);
                        o.put((uint32_t)(a < 0 ? a - 1 : a) & ((1u << s) - 1u), s);
                        run = 0;
                    }
                    if (run) o.put(ac[t].code[0], ac[t].len[0]);
                }
            }
        }
        if (++mx == I.mcus_x) { mx = 0; ++my; }
    }
    o.flush();
    *o.p++ = 0xFF; *o.p++ = 0xD9;
    *bytes = (size_t)(o.p - out);
    return 0;
}

extern "C" int rtm3d_jpeg_quality_tables(int quality, uint16_t* q_luma, uint16_t* q_chroma) {
    if (!q_luma || !q_chroma) { rt_set_error("jpeg_quality_tables: null pointer"); return 1; }
    if (quality < 1 || quality > 100) { rt_set_error("jpeg_quality_tables: quality %d; 1..100", quality); return 1; }
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        const int a = (kBaseLuma[k] * scale + 50) / 100, b = (kBaseChroma[k] * scale + 50) / 100;
        q_luma[k] = (uint16_t)(a < 1 ? 1 : a > 255 ? 255 : a);
        q_chroma[k] = (uint16_t)(b < 1 ? 1 : b > 255 ? 255 : b);
    }
    return 0;
}

extern "C" int rtm3d_jpeg_frame_layout(int h, int w, int mode, rtm3d_jpeg_stream_info* out) {
    char msg[200];
    if (!out) { rt_set_error("jpeg_frame_layout: null pointer"); return 1; }
    if (rt_jpeg_frame_layout(h, w, mode, out, msg, sizeof(msg))) { rt_set_error("jpeg_frame_layout: %s", msg); return 1; }
    return 0;
}

extern "C" int rtm3d_jpeg_encode_bound(int h, int w, int mode, int restart, size_t* bytes) {
    char msg[200];
    if (!bytes) { rt_set_error("jpeg_encode_bound: null pointer"); return 1; }
    if (rt_jpeg_encode_bound(h, w, mode, restart, bytes, msg, sizeof(msg))) { rt_set_error("jpeg_encode_bound: %s", msg); return 1; }
    return 0;
}

extern "C" int rtm3d_jpeg_entropy_encode(const int16_t* h_coef, int h, int w, int mode, int restart, uint8_t* out, size_t capacity, size_t* bytes) {
    char msg[200];
    if (rt_jpeg_entropy_encode(h_coef, h, w, mode, restart, out, capacity, bytes, msg, sizeof(msg))) { rt_set_error("jpeg_entropy_encode: %s", msg); return 1; }
    return 0;
}
