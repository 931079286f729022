// Drawing of tracks (include/rtm3d_hip.h, "drawing tracks"):
//   rtm3d_records_draw_tracks   rtm3d_records_draw with id colours, a text label per slot and a panel painted from the track table
//   rtm3d_draw_font_rows, rtm3d_draw_label_text   host views of the font and of the label text (draw_font.h)
// Compiled with -ffp-contract=off (Makefile), like draw.hip: the fp64 mappings behind the integer pixels are fixed sequences of
// IEEE operations.
//
// The kernel is the GATHER of draw.hip's records_draw_kernel - one workgroup per 64 x 16 tile, four pixels per thread, rounds
// of 256 items binned ORDER-PRESERVING into an LDS list and painted before the next round - with these differences:
//   * a list entry has a KIND (bits 0..1 of l_h): 0 thick segment, 1 face, 2 filled rectangle (l_a = x0 y0 x1 y1, inclusive),
//     3 glyph (l_a = anchor x, anchor y, scale; l_b.x / .y = the low / high word of the 35-bit mask).  A glyph is ONE entry; its
//     cover test is two integer divisions by the scale and a bit test.
//   * a frame is painted in TWO passes of rounds: the 18 geometric items of every slot, last slot first; then, with the label
//     layer, 1 + DRAW_LABEL_MAX items per slot - the background, the glyphs - last slot first.  Each lane asks
//     draw_label_char for ONE character, so no text is ever stored.  The second pass starts its own round: item 256 of the label
//     pass is where a label can straddle two rounds.
//   * a track-driven panel takes DT_TRACK_ITEMS items per table slot: 4 outline segments, heading, velocity, 8 id characters.
//   * with bev_fade < 256 a panel tile loads its pixels up front, fades them and is always stored.
// Integer ranges beyond draw.hip's: label extents lie within 8192 + (6 * 27 + 1) * 4 of the origin; a glyph's (x - gx) / s is
// taken for x >= gx only and the bit index 5 r + 4 - c lies in [0, 34] after c < 5, r < 7.
#include <string.h>

#include "draw_prims.h"
#include "draw_font.h"

#define DT_LABEL_ITEMS (1 + DRAW_LABEL_MAX)
#define DT_TRACK_ITEMS 14
#define DT_ALL_LAYERS (DRAW_FRAME_LAYERS | RTM3D_DRAW_BEV | RTM3D_DRAW_LABEL | RTM3D_DRAW_TRACK_BEV)

__device__ __forceinline__ bool dt_lim(int v) { return v >= -DRAW_MAX_SIDE && v <= DRAW_MAX_SIDE; }

// colour word (bits 8..31) of a track id != 0
__device__ __forceinline__ uint32_t dt_id_colour(const rtm3d_draw_tracks_params& Q, int id, bool tentative) {
    const unsigned a = id < 0 ? 0u - (unsigned)id : (unsigned)id;
    const int k = (int)((a - 1u) % (unsigned)Q.npal);
    int r = Q.palette[k][0], g = Q.palette[k][1], b = Q.palette[k][2];
    if (tentative) { r = (r + 1) >> 1; g = (g + 1) >> 1; b = (b + 1) >> 1; }
    return ((uint32_t)r << 8) | ((uint32_t)g << 16) | ((uint32_t)b << 24);
}

__global__ __launch_bounds__(DRAW_THREADS) void draw_tracks_kernel(const DrawBatch fb, int nb, int topk, const float* __restrict__ rec,
                                                                  const int32_t* __restrict__ ids, int T, const double* __restrict__ state,
                                                                  const double* __restrict__ K, const rtm3d_draw_tracks_params Q,
                                                                  uint8_t* __restrict__ bev, int bev_tiles) {
    __shared__ int4 l_a[DRAW_THREADS];
    __shared__ int4 l_b[DRAW_THREADS];
    __shared__ uint32_t l_h[DRAW_THREADS];         // bits 0..1: kind; bits 8..31: colour
    __shared__ int wave_n[DRAW_THREADS / 64];
    const rtm3d_draw_params& P = Q.base;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int bid = blockIdx.x;

    // ---- which surface, which tile (uniform)
    int img = 0, tile, H, W;
    uint8_t* base;
    const bool panel = bid >= fb.tile0[nb];
    if (panel) {
        const int j = bid - fb.tile0[nb];
        img = j / bev_tiles; tile = j - img * bev_tiles;
        H = P.bev_h; W = P.bev_w;
        base = bev + (size_t)img * H * W * 3;
    } else {
        while (img + 1 < nb && bid >= fb.tile0[img + 1]) ++img;
        tile = bid - fb.tile0[img];
        H = fb.h[img]; W = fb.w[img];
        base = fb.img[img];
    }
    const int tiles_x = (W + DRAW_TW - 1) / DRAW_TW;
    const int ty0 = (tile / tiles_x) * DRAW_TH, tx0 = (tile % tiles_x) * DRAW_TW;
    const int tx1 = imin(tx0 + DRAW_TW, W) - 1, ty1 = imin(ty0 + DRAW_TH, H) - 1;     // last column / row of the tile
    const float* rimg = rec + (size_t)img * topk * 32;
    const int32_t* iimg = ids + (size_t)img * topk;
    const double* kimg = K ? K + (size_t)img * 9 : nullptr;
    const bool tpanel = panel && (P.layers & RTM3D_DRAW_TRACK_BEV) != 0;
    const double* simg = tpanel ? state + (size_t)img * (RTM3D_TRACK_HEADER_DOUBLES + (size_t)T * RTM3D_TRACK_SLOT_DOUBLES) + RTM3D_TRACK_HEADER_DOUBLES
                                : nullptr;
    const int fs = Q.font_scale;

    // ---- this thread's four pixels
    const int py = ty0 + (tid >> 4), px = tx0 + 4 * (tid & 15);
    const bool row_in = py < H;
    uint8_t* pp = base + ((size_t)py * W + px) * 3;
    const bool wide = row_in && px + 3 < W && (((uintptr_t)pp) & 3u) == 0;
    int c00 = 0, c01 = 0, c02 = 0, c10 = 0, c11 = 0, c12 = 0, c20 = 0, c21 = 0, c22 = 0, c30 = 0, c31 = 0, c32 = 0;
    bool loaded = false, dirty = false;
    auto load = [&]() {
        loaded = true;
        if (wide) {
            const uint32_t* q = (const uint32_t*)pp;
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
            c00 = d0 & 255; c01 = (d0 >> 8) & 255; c02 = (d0 >> 16) & 255; c10 = d0 >> 24;
            c11 = d1 & 255; c12 = (d1 >> 8) & 255; c20 = (d1 >> 16) & 255; c21 = d1 >> 24;
            c22 = d2 & 255; c30 = (d2 >> 8) & 255; c31 = (d2 >> 16) & 255; c32 = d2 >> 24;
        } else if (row_in) {
            if (px < W) { c00 = pp[0]; c01 = pp[1]; c02 = pp[2]; }
            if (px + 1 < W) { c10 = pp[3]; c11 = pp[4]; c12 = pp[5]; }
            if (px + 2 < W) { c20 = pp[6]; c21 = pp[7]; c22 = pp[8]; }
            if (px + 3 < W) { c30 = pp[9]; c31 = pp[10]; c32 = pp[11]; }
        }
    };
    if (panel && Q.bev_fade < 256) {               // the trails: every panel pixel fades before anything is painted
        const int f = Q.bev_fade;
        load();
        c00 = (c00 * f + 128) >> 8; c01 = (c01 * f + 128) >> 8; c02 = (c02 * f + 128) >> 8;
        c10 = (c10 * f + 128) >> 8; c11 = (c11 * f + 128) >> 8; c12 = (c12 * f + 128) >> 8;
        c20 = (c20 * f + 128) >> 8; c21 = (c21 * f + 128) >> 8; c22 = (c22 * f + 128) >> 8;
        c30 = (c30 * f + 128) >> 8; c31 = (c31 * f + 128) >> 8; c32 = (c32 * f + 128) >> 8;
        dirty = true;
    }

    const int npass = (!panel && (P.layers & RTM3D_DRAW_LABEL)) ? 2 : 1;
    for (int pass = (!panel && !(P.layers & DRAW_FRAME_LAYERS)) ? 1 : 0; pass < npass; ++pass) {
    const int nprim = tpanel ? DT_TRACK_ITEMS : panel ? DRAW_BEV_PRIMS : pass == 1 ? DT_LABEL_ITEMS : DRAW_PRIMS;
    const int items = (tpanel ? T : topk) * nprim;
    for (int i0 = 0; i0 < items; i0 += DRAW_THREADS) {
        // ---- binning: one item per thread, in painter's order
        const int i = i0 + tid;
        bool hit = false;
        int4 ea = make_int4(0, 0, 0, 0), eb = make_int4(0, 0, 0, 0);
        uint32_t eh = 0;
        if (i < items) {
            const int s = i / nprim, p = i - s * nprim;
            bool ok = false;
            int x0 = 0, y0 = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0, x3 = 0, y3 = 0, t = P.thickness;
            if (tpanel) {
                const double* sl = simg + (size_t)(T - 1 - s) * RTM3D_TRACK_SLOT_DOUBLES;
                const double idd = sl[0];
                if (idd >= 1.0 && idd < 2147483648.0) {
                    const int id = (int)idd;
                    const bool tentative = sl[3] < 1.0;
                    eh = dt_id_colour(Q, id, tentative);
                    t = 1;
                    const double ry = sl[13], c = cos(ry), sn = sin(ry), hl = sl[9] / 2.0, hw = sl[8] / 2.0, X = sl[10], Z = sl[12];
                    if (p < 4) {                                         // outline: corner p to corner p + 1
                        const int kb = (p + 1) & 3;
                        const bool a = draw_bev_point(c, sn, (p == 0 || p == 3) ? hl : -hl, p < 2 ? hw : -hw, X, Z, P.bev_h, P.bev_w, P.bev_m_per_px, x0, y0);
                        const bool b = draw_bev_point(c, sn, (kb == 0 || kb == 3) ? hl : -hl, kb < 2 ? hw : -hw, X, Z, P.bev_h, P.bev_w, P.bev_m_per_px, x1, y1);
                        ok = a && b;
                    } else {
                        const bool a = draw_bev_point(c, sn, 0.0, 0.0, X, Z, P.bev_h, P.bev_w, P.bev_m_per_px, x0, y0);
                        if (p == 4) {                                    // heading mark
                            ok = draw_bev_point(c, sn, hl, 0.0, X, Z, P.bev_h, P.bev_w, P.bev_m_per_px, x1, y1) && a;
                        } else if (p == 5) {                             // velocity mark
                            if (Q.vel_horizon > 0.0) {
                                const double ex = X + sl[14] * Q.vel_horizon, ez = Z + sl[16] * Q.vel_horizon;
                                const double u = (double)P.bev_w / 2.0 + ex / P.bev_m_per_px, v = (double)P.bev_h - ez / P.bev_m_per_px;
                                const bool b = draw_coord(u, x1), d = draw_coord(v, y1);
                                ok = a && b && d;
                            }
                        } else if ((Q.label_fields & 1) && a) {          // character p - 6 of the id text
                            int len;
                            const int ch = draw_label_char(1, tentative ? -id : id, nullptr, 0.0f, 0.0f, p - 6, &len);
                            if (ch != 0) {
                                const uint64_t m = draw_font_mask(draw_font_index(ch));
                                x0 += 6 * fs * (p - 6);
                                ok = m != 0 && dt_lim(x0) && dt_lim(x0 + 5 * fs - 1) && dt_lim(y0 + 7 * fs - 1);
                                ea = make_int4(x0, y0, fs, 0); eb = make_int4((int)(uint32_t)m, (int)(uint32_t)(m >> 32), 0, 0);
                                eh |= 3u;
                            }
                        }
                    }
                }
            } else {
            const float* r = rimg + (size_t)(topk - 1 - s) * 32;
            const float flag = r[31], fc = r[0];
            const bool kept = flag == 2.0f;
            if (flag >= (float)P.min_flag && fc >= 0.0f && fc < (float)P.ncls) {
                const int ci = (int)fc, id = iimg[topk - 1 - s];
                if (id == 0) eh = ((uint32_t)P.color[ci][0] << 8) | ((uint32_t)P.color[ci][1] << 16) | ((uint32_t)P.color[ci][2] << 24);
                else eh = dt_id_colour(Q, id, id < 0);
                if (pass == 1) {                                             // label: 0 the background, 1.. the glyphs
                    const bool a = draw_coord((double)r[20], x0), b = draw_coord((double)r[21], y0);
                    if (a && b) {
                        int len;
                        const int ch = draw_label_char(Q.label_fields & (kept ? 15 : 7), id, Q.names[ci], r[1], r[29], p - 1, &len);
                        if (y0 - 9 * fs >= 0) y0 -= 9 * fs;                  // above the box, or inside it
                        if (p == 0) {
                            x1 = x0 + (6 * len + 1) * fs - 1; y1 = y0 + 9 * fs - 1;
                            ok = len > 0 && dt_lim(y0) && dt_lim(x1) && dt_lim(y1);
                            ea = make_int4(x0, y0, x1, y1);
                            eh |= 2u;
                        } else if (ch != 0) {
                            const uint64_t m = draw_font_mask(draw_font_index(ch));
                            x0 += fs + 6 * fs * (p - 1); y0 += fs;
                            ok = m != 0 && dt_lim(x0) && dt_lim(y0) && dt_lim(x0 + 5 * fs - 1) && dt_lim(y0 + 7 * fs - 1);
                            ea = make_int4(x0, y0, fs, 0); eb = make_int4((int)(uint32_t)m, (int)(uint32_t)(m >> 32), 0, 0);
                            const int lum = 299 * (int)((eh >> 8) & 255) + 587 * (int)((eh >> 16) & 255) + 114 * (int)(eh >> 24);
                            eh = (lum >= 128000 ? 0u : 0xFFFFFF00u) | 3u;
                        }
                    }
                } else if (panel) {
                    if (kept) {
                        const double ry = (double)r[30], c = cos(ry), sn = sin(ry);
                        const double hl = (double)r[26] / 2.0, hw = (double)r[25] / 2.0, X = (double)r[27], Z = (double)r[29];
                        // end points a, b of item p: corners k = 0..3 at local (+,+), (-,+), (-,-), (+,-); 4: the centre, 5: mid +x edge
                        const int ka = p, kb = p == 4 ? 5 : ((p + 1) & 3);
                        const bool a = draw_bev_point(c, sn, ka == 4 ? 0.0 : ((ka == 0 || ka == 3) ? hl : -hl), ka == 4 ? 0.0 : (ka < 2 ? hw : -hw), X, Z,
                                                      P.bev_h, P.bev_w, P.bev_m_per_px, x0, y0);
                        const bool b = draw_bev_point(c, sn, (kb == 0 || kb == 3 || kb == 5) ? hl : -hl, kb == 5 ? 0.0 : (kb < 2 ? hw : -hw), X, Z,
                                                      P.bev_h, P.bev_w, P.bev_m_per_px, x1, y1);
                        ok = a && b;
                        t = 1;
                    }
                } else if (p >= 1 && p <= 4) {                               // 2D box: sides 1-2, 2-3, 3-4, 4-1 of its corners
                    if (P.layers & RTM3D_DRAW_BOX2D) {
                        int bx1 = 0, by1 = 0, bx2 = 0, by2 = 0;
                        const bool a = draw_coord((double)r[20], bx1), b = draw_coord((double)r[21], by1);
                        const bool c = draw_coord((double)r[22], bx2), d = draw_coord((double)r[23], by2);
                        x0 = (p == 1 || p == 4) ? bx1 : bx2; y0 = p <= 2 ? by1 : by2;
                        x1 = p <= 2 ? bx2 : bx1;             y1 = (p == 1 || p == 4) ? by1 : by2;
                        // a side needs the three coordinates it uses
                        ok = (p == 1) ? (a && b && c) : (p == 2) ? (b && c && d) : (p == 3) ? (a && c && d) : (a && b && d);
                    }
                } else if (p == 17) {                                        // key-point disc = the segment P == Q of thickness 2 r
                    if (P.layers & RTM3D_DRAW_KEYPOINT) {
                        const bool a = draw_coord((double)r[2], x0), b = draw_coord((double)r[3], y0);
                        ok = a && b;
                        x1 = x0; y1 = y0; t = 2 * P.radius;
                    }
                } else if ((P.layers & (p == 0 ? RTM3D_DRAW_FACE : RTM3D_DRAW_WIREFRAME)) && (P.source == 0 || kept)) {
                    double xs[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sn = 0.0, cs = 0.0;
                    bool front = true;
                    if (P.source == 1) {
                        const double ry = (double)r[30];
                        sn = sin(ry); cs = cos(ry);
                        xs[2] = (double)r[26]; xs[3] = (double)r[24]; xs[4] = (double)r[25];
                        xs[5] = (double)r[27]; xs[6] = (double)r[28]; xs[7] = (double)r[29];
                        // camera depth of the corners (box_project_corner's Z; it does not depend on the sign along y)
                        const double dx = xs[2] / 2, dz = xs[4] / 2;
                        const double za = (-sn * dx) + (cs * dz) + xs[7], zb = (-sn * dx) + (cs * dz) * -1.0 + xs[7];
                        const double zc = (-sn * dx) * -1.0 + (cs * dz) + xs[7], zd = (-sn * dx) * -1.0 + (cs * dz) * -1.0 + xs[7];
                        front = za >= 0.1 && zb >= 0.1 && zc >= 0.1 && zd >= 0.1;
                    }
                    if (front) {
                        if (p == 0) {
                            const bool a = draw_vertex(r, xs, kimg, sn, cs, P.source, 0, x0, y0);
                            const bool b = draw_vertex(r, xs, kimg, sn, cs, P.source, 1, x1, y1);
                            const bool c = draw_vertex(r, xs, kimg, sn, cs, P.source, 3, x2, y2);
                            const bool d = draw_vertex(r, xs, kimg, sn, cs, P.source, 2, x3, y3);
                            ok = a && b && c && d;
                            eh |= 1u;
                        } else {                                              // edge p - 5 of 01 13 32 20 04 45 57 76 64 51 37 62
                            const int e = (p - 5) * 4;
                            const int va = (int)((0x635675402310ull >> e) & 15ull), vb = (int)((0x271467540231ull >> e) & 15ull);
                            const bool a = draw_vertex(r, xs, kimg, sn, cs, P.source, va, x0, y0);
                            const bool b = draw_vertex(r, xs, kimg, sn, cs, P.source, vb, x1, y1);
                            ok = a && b;
                        }
                    }
                }
            }
            }
            if (ok) {
                const uint32_t kind = eh & 3u;
                int bx0, bx1, by0, by1;
                if (kind == 1u) {
                    bx0 = imin(imin(x0, x1), imin(x2, x3)); bx1 = imax(imax(x0, x1), imax(x2, x3));
                    by0 = imin(imin(y0, y1), imin(y2, y3)); by1 = imax(imax(y0, y1), imax(y2, y3));
                    ea = make_int4(x0, y0, x1, y1); eb = make_int4(x2, y2, x3, y3);
                } else if (kind == 2u) {
                    bx0 = ea.x; by0 = ea.y; bx1 = ea.z; by1 = ea.w;
                } else if (kind == 3u) {
                    bx0 = ea.x; by0 = ea.y; bx1 = ea.x + 5 * fs - 1; by1 = ea.y + 7 * fs - 1;
                } else {
                    const int inf = (t + 1) >> 1;
                    bx0 = imin(x0, x1) - inf; bx1 = imax(x0, x1) + inf; by0 = imin(y0, y1) - inf; by1 = imax(y0, y1) + inf;
                    ea = make_int4(x0, y0, x1, y1); eb = make_int4(t * t, inf, 0, 0);
                }
                hit = bx0 <= tx1 && bx1 >= tx0 && by0 <= ty1 && by1 >= ty0;
            }
        }
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
        if ((tid & 63) == 0) wave_n[wave] = __builtin_popcountll(bal);
        __syncthreads();
        int before = 0, n = 0;
#pragma unroll
        for (int w = 0; w < DRAW_THREADS / 64; ++w) { if (w < wave) before += wave_n[w]; n += wave_n[w]; }
        if (hit) {
            const int k = before + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
            l_a[k] = ea; l_b[k] = eb; l_h[k] = eh;
        }
        __syncthreads();                             // (the next round's wave_n is written after every wave has read this one's)
        if (n == 0) continue;

        // ---- painting
        if (!loaded) load();
        for (int e = 0; e < n; ++e) {
            const int4 a = l_a[e], b = l_b[e];
            const uint32_t h = l_h[e], kind = h & 3u;
            const int r0 = (h >> 8) & 255, r1 = (h >> 16) & 255, r2 = h >> 24;
            bool m0, m1, m2, m3;
            if (kind == 1u) {
                if (py < imin(imin(a.y, a.w), imin(b.y, b.w)) || py > imax(imax(a.y, a.w), imax(b.y, b.w))) continue;
                m0 = tri_covers(px, py, a.x, a.y, a.z, a.w, b.x, b.y) || tri_covers(px, py, a.x, a.y, b.x, b.y, b.z, b.w);
                m1 = tri_covers(px + 1, py, a.x, a.y, a.z, a.w, b.x, b.y) || tri_covers(px + 1, py, a.x, a.y, b.x, b.y, b.z, b.w);
                m2 = tri_covers(px + 2, py, a.x, a.y, a.z, a.w, b.x, b.y) || tri_covers(px + 2, py, a.x, a.y, b.x, b.y, b.z, b.w);
                m3 = tri_covers(px + 3, py, a.x, a.y, a.z, a.w, b.x, b.y) || tri_covers(px + 3, py, a.x, a.y, b.x, b.y, b.z, b.w);
                const int al = P.face_alpha, na = 256 - al;
                if (m0) { c00 = (c00 * na + r0 * al + 128) >> 8; c01 = (c01 * na + r1 * al + 128) >> 8; c02 = (c02 * na + r2 * al + 128) >> 8; }
                if (m1) { c10 = (c10 * na + r0 * al + 128) >> 8; c11 = (c11 * na + r1 * al + 128) >> 8; c12 = (c12 * na + r2 * al + 128) >> 8; }
                if (m2) { c20 = (c20 * na + r0 * al + 128) >> 8; c21 = (c21 * na + r1 * al + 128) >> 8; c22 = (c22 * na + r2 * al + 128) >> 8; }
                if (m3) { c30 = (c30 * na + r0 * al + 128) >> 8; c31 = (c31 * na + r1 * al + 128) >> 8; c32 = (c32 * na + r2 * al + 128) >> 8; }
                dirty = dirty || m0 || m1 || m2 || m3;
                continue;
            }
            if (kind == 2u) {
                const bool row = py >= a.y && py <= a.w;
                m0 = row && px >= a.x && px <= a.z;         m1 = row && px + 1 >= a.x && px + 1 <= a.z;
                m2 = row && px + 2 >= a.x && px + 2 <= a.z; m3 = row && px + 3 >= a.x && px + 3 <= a.z;
            } else if (kind == 3u) {
                const int sc = a.z, dy = py - a.y, dx = px - a.x;
                if (dy < 0 || dx + 3 < 0 || dx >= 5 * sc) continue;
                const int gr = dy / sc;
                if (gr >= 7) continue;
                const uint32_t row = (uint32_t)((((uint64_t)(uint32_t)b.y << 32) | (uint64_t)(uint32_t)b.x) >> (5 * gr)) & 31u;
                const int g0 = dx >= 0 ? dx / sc : 5, g1 = dx + 1 >= 0 ? (dx + 1) / sc : 5, g2 = dx + 2 >= 0 ? (dx + 2) / sc : 5, g3 = (dx + 3) / sc;
                m0 = g0 < 5 && ((row >> (4 - g0)) & 1u); m1 = g1 < 5 && ((row >> (4 - g1)) & 1u);
                m2 = g2 < 5 && ((row >> (4 - g2)) & 1u); m3 = g3 < 5 && ((row >> (4 - g3)) & 1u);
            } else {
                // (t + 1) / 2 >= t / 2: outside the inflated box of the segment nothing is covered
                const int t2 = b.x, inf = b.y;
                if (py < imin(a.y, a.w) - inf || py > imax(a.y, a.w) + inf || px > imax(a.x, a.z) + inf || px + 3 < imin(a.x, a.z) - inf) continue;
                m0 = seg_covers(px, py, a.x, a.y, a.z, a.w, t2);
                m1 = seg_covers(px + 1, py, a.x, a.y, a.z, a.w, t2);
                m2 = seg_covers(px + 2, py, a.x, a.y, a.z, a.w, t2);
                m3 = seg_covers(px + 3, py, a.x, a.y, a.z, a.w, t2);
            }
            if (m0) { c00 = r0; c01 = r1; c02 = r2; }
            if (m1) { c10 = r0; c11 = r1; c12 = r2; }
            if (m2) { c20 = r0; c21 = r1; c22 = r2; }
            if (m3) { c30 = r0; c31 = r1; c32 = r2; }
            dirty = dirty || m0 || m1 || m2 || m3;
        }
    }
    }

    if (!dirty) return;
    if (wide) {
        uint32_t* q = (uint32_t*)pp;
        q[0] = (uint32_t)c00 | ((uint32_t)c01 << 8) | ((uint32_t)c02 << 16) | ((uint32_t)c10 << 24);
        q[1] = (uint32_t)c11 | ((uint32_t)c12 << 8) | ((uint32_t)c20 << 16) | ((uint32_t)c21 << 24);
        q[2] = (uint32_t)c22 | ((uint32_t)c30 << 8) | ((uint32_t)c31 << 16) | ((uint32_t)c32 << 24);
    } else if (row_in) {
        if (px < W) { pp[0] = (uint8_t)c00; pp[1] = (uint8_t)c01; pp[2] = (uint8_t)c02; }
        if (px + 1 < W) { pp[3] = (uint8_t)c10; pp[4] = (uint8_t)c11; pp[5] = (uint8_t)c12; }
        if (px + 2 < W) { pp[6] = (uint8_t)c20; pp[7] = (uint8_t)c21; pp[8] = (uint8_t)c22; }
        if (px + 3 < W) { pp[9] = (uint8_t)c30; pp[10] = (uint8_t)c31; pp[11] = (uint8_t)c32; }
    }
}

extern void rt_set_error(const char* fmt, ...);

extern "C" int rtm3d_draw_font_rows(int ch, uint8_t rows[7]) {
    const int g = draw_font_index(ch);
    if (g < 0 || !rows) return 1;
    const uint64_t m = draw_font_mask(g);
    for (int r = 0; r < 7; ++r) rows[r] = (uint8_t)((m >> (5 * r)) & 31u);
    return 0;
}

extern "C" int rtm3d_draw_label_text(const rtm3d_draw_tracks_params* p, int id, int cls, float score, float z, char out[32]) {
    if (!p || !out) { rt_set_error("draw_label_text: null pointer"); return 1; }
    if (p->label_fields < 0 || p->label_fields > 15) { rt_set_error("draw_label_text: label_fields %d is outside 0..15", p->label_fields); return 1; }
    if (cls < 0 || cls >= p->base.ncls || cls >= RTM3D_ENGINE_MAX_CLASSES) { rt_set_error("draw_label_text: class %d is outside the table of %d classes", cls, p->base.ncls); return 1; }
    int len = 0;
    for (int j = 0; j < 31; ++j) out[j] = (char)draw_label_char(p->label_fields, id, p->names[cls], score, z, j, &len);
    out[31] = 0;
    return 0;
}

extern "C" int rtm3d_draw_tracks_default_params(rtm3d_draw_tracks_params* p) {
    if (!p) { rt_set_error("draw_tracks_default_params: null pointer"); return 1; }
    // 32 id colours: the eight hues of the class palette, then each of them lighter, then two further turns of the hue wheel
    static const uint8_t palette[32][3] = {
        {255, 64, 64}, {64, 224, 64}, {64, 128, 255}, {255, 208, 0}, {255, 64, 224}, {0, 224, 224}, {255, 144, 32}, {176, 112, 255},
        {255, 160, 160}, {160, 240, 160}, {160, 192, 255}, {255, 232, 128}, {255, 160, 240}, {128, 240, 240}, {255, 200, 144}, {216, 184, 255},
        {200, 0, 48}, {0, 160, 72}, {0, 72, 200}, {184, 144, 0}, {176, 0, 160}, {0, 144, 160}, {200, 88, 0}, {104, 48, 200},
        {255, 112, 0}, {144, 255, 0}, {0, 200, 255}, {255, 255, 96}, {255, 0, 128}, {0, 255, 160}, {224, 176, 96}, {128, 128, 255}};
    memset(p, 0, sizeof *p);
    if (rtm3d_draw_default_params(&p->base) != 0) return 1;
    p->npal = 32;
    memcpy(p->palette, palette, sizeof palette);
    p->label_fields = 3; p->font_scale = 1;
    for (int c = 0; c < RTM3D_ENGINE_MAX_CLASSES; ++c) {
        p->names[c][0] = 'C';
        if (c >= 10) { p->names[c][1] = '1'; p->names[c][2] = (char)('0' + c - 10); }
        else p->names[c][1] = (char)('0' + c);
    }
    p->bev_fade = 256; p->vel_horizon = 1.0;
    return 0;
}

extern "C" int rtm3d_records_draw_tracks(void* stream, int B, int topk, const float* d_rec, const int32_t* d_ids, int T, const double* d_state,
                                         uint8_t* const* h_imgs, const int* h_hw, const double* d_K_camera,
                                         const rtm3d_draw_tracks_params* params, uint8_t* d_bev) {
    if (!params) { rt_set_error("records_draw: null pointer"); return 1; }
    const rtm3d_draw_tracks_params& Q = *params;
    const rtm3d_draw_params& P = Q.base;
    const bool panels = (P.layers & (RTM3D_DRAW_BEV | RTM3D_DRAW_TRACK_BEV)) != 0, tpanel = (P.layers & RTM3D_DRAW_TRACK_BEV) != 0;
    if (draw_check_args(B, topk, d_rec, h_imgs, h_hw, d_K_camera, &P, d_bev, DT_ALL_LAYERS, "seven", panels)) return 1;
    if ((P.layers & RTM3D_DRAW_BEV) && tpanel) { rt_set_error("records_draw_tracks: layers %d sets both RTM3D_DRAW_BEV and RTM3D_DRAW_TRACK_BEV", P.layers); return 1; }
    if (Q.npal < 1 || Q.npal > 32) { rt_set_error("records_draw_tracks: npal %d is outside 1..32", Q.npal); return 1; }
    if (Q.font_scale < 1 || Q.font_scale > 4) { rt_set_error("records_draw_tracks: font_scale %d is outside 1..4", Q.font_scale); return 1; }
    if (Q.label_fields < 0 || Q.label_fields > 15) { rt_set_error("records_draw_tracks: label_fields %d is outside 0..15", Q.label_fields); return 1; }
    if ((P.layers & RTM3D_DRAW_LABEL) && Q.label_fields == 0) { rt_set_error("records_draw_tracks: RTM3D_DRAW_LABEL with label_fields 0"); return 1; }
    if (Q.bev_fade < 0 || Q.bev_fade > 256) { rt_set_error("records_draw_tracks: bev_fade %d is outside 0..256", Q.bev_fade); return 1; }
    if (!(Q.vel_horizon >= 0.0) || !(Q.vel_horizon < 1e300)) { rt_set_error("records_draw_tracks: vel_horizon %g is negative or not finite", Q.vel_horizon); return 1; }
    if (!d_ids) { rt_set_error("records_draw_tracks: d_ids is NULL"); return 1; }
    if (tpanel) {
        if (!d_state) { rt_set_error("records_draw_tracks: RTM3D_DRAW_TRACK_BEV is set and d_state is NULL"); return 1; }
        if (T < 1 || T > 256) { rt_set_error("records_draw_tracks: T %d is outside 1..256", T); return 1; }
    }
    const bool frames = (P.layers & (DRAW_FRAME_LAYERS | RTM3D_DRAW_LABEL)) != 0;
    const int bev_tiles = panels ? ((P.bev_w + DRAW_TW - 1) / DRAW_TW) * ((P.bev_h + DRAW_TH - 1) / DRAW_TH) : 0;
    const size_t stream_doubles = RTM3D_TRACK_HEADER_DOUBLES + (size_t)(tpanel ? T : 0) * RTM3D_TRACK_SLOT_DOUBLES;
    for (int b0 = 0; b0 < B; b0 += DRAW_MAX_BATCH) {
        const int nb = B - b0 < DRAW_MAX_BATCH ? B - b0 : DRAW_MAX_BATCH;
        DrawBatch fb;
        const int tiles = draw_fill_batch(fb, h_imgs, h_hw, b0, nb, frames);
        const int grid = tiles + nb * bev_tiles;                   // <= 64 * 65536 * 2
        hipLaunchKernelGGL(draw_tracks_kernel, dim3((unsigned)grid), dim3(DRAW_THREADS), 0, (hipStream_t)stream, fb, nb, topk,
                           d_rec + (size_t)b0 * topk * 32, d_ids + (size_t)b0 * topk, T, tpanel ? d_state + (size_t)b0 * stream_doubles : nullptr,
                           d_K_camera ? d_K_camera + (size_t)b0 * 9 : nullptr, Q,
                           panels ? d_bev + (size_t)b0 * P.bev_h * P.bev_w * 3 : nullptr, bev_tiles > 0 ? bev_tiles : 1);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("records_draw_tracks launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
