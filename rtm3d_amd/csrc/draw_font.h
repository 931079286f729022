// The font and the label text of rtm3d_records_draw_tracks (include/rtm3d_hip.h, "drawing tracks"): the library's ONE copy of
// the 5 x 7 bitmaps and the ONE function that composes a label, used by the kernel (draw_tracks.hip) and by the host helpers
// rtm3d_draw_font_rows / rtm3d_draw_label_text.  The glyphs are the project's own drawing; tests/draw_tracks_ref.py holds them
// once more as '#' / '.' art.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DRAW_HD __host__ __device__ inline
#else
#define DRAW_HD inline
#endif

#define DRAW_FONT_GLYPHS 44
#define DRAW_LABEL_MAX 28              // characters of the longest label: 8 + 1 + 7 + 1 + 3 + 1 + 6 = 27
// seven rows, top first, 5 low bits each, bit 4 the LEFT column: glyph pixel (column c, row r) is bit 5 r + 4 - c of the mask
#define DRAW_GLYPH(a, b, c, d, e, f, g) \
    ((uint64_t)(a) | (uint64_t)(b) << 5 | (uint64_t)(c) << 10 | (uint64_t)(d) << 15 | (uint64_t)(e) << 20 | (uint64_t)(f) << 25 | (uint64_t)(g) << 30)

// the 35-bit mask of glyph g (draw_font_index)
DRAW_HD uint64_t draw_font_mask(int g) {
    static constexpr uint64_t table[DRAW_FONT_GLYPHS] = {
        DRAW_GLYPH(0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00),   /*   */
        DRAW_GLYPH(0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E),   /* 0 */
        DRAW_GLYPH(0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),   /* 1 */
        DRAW_GLYPH(0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),   /* 2 */
        DRAW_GLYPH(0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),   /* 3 */
        DRAW_GLYPH(0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02),   /* 4 */
        DRAW_GLYPH(0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),   /* 5 */
        DRAW_GLYPH(0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E),   /* 6 */
        DRAW_GLYPH(0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),   /* 7 */
        DRAW_GLYPH(0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),   /* 8 */
        DRAW_GLYPH(0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),   /* 9 */
        DRAW_GLYPH(0x0E, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11),   /* A */
        DRAW_GLYPH(0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E),   /* B */
        DRAW_GLYPH(0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E),   /* C */
        DRAW_GLYPH(0x1C, 0x12, 0x11, 0x11, 0x11, 0x12, 0x1C),   /* D */
        DRAW_GLYPH(0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F),   /* E */
        DRAW_GLYPH(0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10),   /* F */
        DRAW_GLYPH(0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0F),   /* G */
        DRAW_GLYPH(0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11),   /* H */
        DRAW_GLYPH(0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E),   /* I */
        DRAW_GLYPH(0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C),   /* J */
        DRAW_GLYPH(0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11),   /* K */
        DRAW_GLYPH(0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F),   /* L */
        DRAW_GLYPH(0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11),   /* M */
        DRAW_GLYPH(0x11, 0x11, 0x19, 0x15, 0x13, 0x11, 0x11),   /* N */
        DRAW_GLYPH(0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),   /* O */
        DRAW_GLYPH(0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10),   /* P */
        DRAW_GLYPH(0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D),   /* Q */
        DRAW_GLYPH(0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11),   /* R */
        DRAW_GLYPH(0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E),   /* S */
        DRAW_GLYPH(0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04),   /* T */
        DRAW_GLYPH(0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),   /* U */
        DRAW_GLYPH(0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04),   /* V */
        DRAW_GLYPH(0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0A),   /* W */
        DRAW_GLYPH(0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11),   /* X */
        DRAW_GLYPH(0x11, 0x11, 0x11, 0x0A, 0x04, 0x04, 0x04),   /* Y */
        DRAW_GLYPH(0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F),   /* Z */
        DRAW_GLYPH(0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A),   /* # */
        DRAW_GLYPH(0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04),   /* ? */
        DRAW_GLYPH(0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C),   /* . */
        DRAW_GLYPH(0x19, 0x19, 0x02, 0x04, 0x08, 0x13, 0x13),   /* % */
        DRAW_GLYPH(0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00),   /* - */
        DRAW_GLYPH(0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00),   /* : */
        DRAW_GLYPH(0x01, 0x01, 0x02, 0x04, 0x08, 0x10, 0x10),   /* / */
    };
    return table[g];
}

// position of a character in the set (space, 0-9, A-Z, # ? . % - : /), -1 outside it
DRAW_HD int draw_font_index(int ch) {
    if (ch == ' ') return 0;
    if (ch >= '0' && ch <= '9') return 1 + (ch - '0');
    if (ch >= 'A' && ch <= 'Z') return 11 + (ch - 'A');
    return ch == '#' ? 37 : ch == '?' ? 38 : ch == '.' ? 39 : ch == '%' ? 40 : ch == '-' ? 41 : ch == ':' ? 42 : ch == '/' ? 43 : -1;
}

// a byte of a class name as the character that is drawn: lower case as upper case, anything outside the set as '?'
DRAW_HD int draw_font_fold(int byte) {
    if (byte >= 'a' && byte <= 'z') byte -= 'a' - 'A';
    return draw_font_index(byte) < 0 ? '?' : byte;
}

DRAW_HD int draw_digits(int v) {                                 // 0 <= v < 10^7
    return v >= 1000000 ? 7 : v >= 100000 ? 6 : v >= 10000 ? 5 : v >= 1000 ? 4 : v >= 100 ? 3 : v >= 10 ? 2 : 1;
}
DRAW_HD int draw_digit_at(int v, int nd, int i) {                // digit i from the left of the nd-digit number v
    for (int k = nd - 1 - i; k > 0; --k) v /= 10;
    return '0' + v % 10;
}

// Character j of the label of a slot, 0 at and beyond its end; *len = the length of the whole text (<= 27).  fields = the mask
// label_fields (the caller clears bit 8 for a slot whose flag is not 2), id = the track id of the slot, name = the class name
// (read only with bit 2).  No array is written: every lane of the kernel asks for ONE character.
DRAW_HD int draw_label_char(int fields, int id, const char* name, float score, float z, int j, int* len) {
    int pos = 0, ch = 0;
    if ((fields & 1) && id != 0) {
        const int a = (int)((id < 0 ? 0u - (unsigned)id : (unsigned)id) % 10000000u), nd = draw_digits(a);
        if (j == 0) ch = id < 0 ? '?' : '#';
        else if (j <= nd) ch = draw_digit_at(a, nd, j - 1);
        pos = 1 + nd;
    }
    if (fields & 2) {
        int nl = 0;
        while (nl < 7 && name[nl] != 0) ++nl;
        if (nl > 0) {
            if (pos > 0) { if (j == pos) ch = ' '; ++pos; }
            if (j >= pos && j < pos + nl) ch = draw_font_fold((int)(unsigned char)name[j - pos]);
            pos += nl;
        }
    }
    if (fields & 4) {
        const double v = (double)score * 100.0;
        const int n = !(v >= 0.0) ? 0 : v >= 99.0 ? 99 : (int)v;
        if (pos > 0) { if (j == pos) ch = ' '; ++pos; }
        if (j == pos) ch = '0' + n / 10;
        else if (j == pos + 1) ch = '0' + n % 10;
        else if (j == pos + 2) ch = '%';
        pos += 3;
    }
    if (fields & 8) {
        const double v = (double)z * 10.0;
        const int n = !(v >= 0.0) ? 0 : v >= 9999.0 ? 9999 : (int)v, whole = n / 10, nd = draw_digits(whole);
        if (pos > 0) { if (j == pos) ch = ' '; ++pos; }
        if (j >= pos && j < pos + nd) ch = draw_digit_at(whole, nd, j - pos);
        else if (j == pos + nd) ch = '.';
        else if (j == pos + nd + 1) ch = '0' + n % 10;
        else if (j == pos + nd + 2) ch = 'M';
        pos += nd + 3;
    }
    *len = pos;
    return ch;
}
