// Drawing of detection records into the camera frames and a bird's-eye panel (include/rtm3d_hip.h, "drawing"):
//   rtm3d_records_draw     paints key points, 2D boxes, box wireframes with a shaded front face and a bird's-eye view, in place.
// The drawing rule - integer coordinates, exact integer coverage tests, painter's order - is the header's; this file is its one
// device statement.  Compiled with -ffp-contract=off (Makefile): the fp64 projection of source 1 and the bird's-eye mapping
// are fixed sequences of IEEE operations.
//
// A GATHER: one workgroup owns one DRAW_TW x DRAW_TH tile of one frame or panel, one thread four adjacent pixels of a row, and
// nobody else writes those bytes - the painter's order holds without atomics.  Per round the 256 threads take the next 256
// (slot, primitive) items in painter's order (slot topk - 1 first; face, box sides, edges, disc), make the primitive's integer
// coordinates from the record and test its bounding box against the tile; the hits are compacted ORDER-PRESERVING into an LDS
// list (ballot + mbcnt rank inside the wave, the waves' counts through LDS) and painted before the next round is binned: the list
// holds one round (DRAW_THREADS entries), so no tile can overflow it whatever the number of slots.  Painting walks the list in
// order with the pixels in registers; the list address is uniform, so the reads are LDS broadcasts.  The pixels are loaded at
// the first non-empty list and stored once at the end: a tile no primitive touches neither reads nor writes the frame.
// Frame rows are 3 * w bytes: a thread whose four pixels all lie inside the row and start on a dword boundary moves three
// dwords of its OWN bytes; every other thread moves single bytes.  Plain vector stores only.
//
// Integer ranges (int32 unless said): coordinates lie in [-8192, 8192], pixels in [0, 8191], so d = Q - P has |d.| <= 2^14 and
// v = p - P lies in [-8192, 16383].  d.d <= 2^29, v.d and v x d <= 2^29, |v|^2 < 2^29 (4|v|^2 in int64), 2 (v x d) <= 2^30 and its
// square <= 2^60 (int64), t^2 (d.d) <= 2^16 * 2^29 (int64; t <= 128 = twice the largest radius).  Edge functions of the face:
// (b - a) x (p - a) with factors <= 2^14, < 2^29.
#include "draw_prims.h"                 // tile geometry, DrawBatch, draw_coord, the coverage tests (shared with draw_tracks.hip)

__global__ __launch_bounds__(DRAW_THREADS) void records_draw_kernel(const DrawBatch fb, int nb, int topk, const float* __restrict__ rec,
                                                                   const double* __restrict__ K, const rtm3d_draw_params P,
                                                                   uint8_t* __restrict__ bev, int bev_tiles) {
    __shared__ int4 l_a[DRAW_THREADS];             // segment: P, Q; face: vertices 0, 1
    __shared__ int4 l_b[DRAW_THREADS];             // segment: t^2, ceil(t / 2); face: vertices 3, 2
    __shared__ uint32_t l_h[DRAW_THREADS];         // bit 0: face; bits 8..31: colour
    __shared__ int wave_n[DRAW_THREADS / 64];
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
    const double* kimg = K ? K + (size_t)img * 9 : nullptr;

    // ---- this thread's four pixels
    const int py = ty0 + (tid >> 4), px = tx0 + 4 * (tid & 15);
    const bool row_in = py < H;
    uint8_t* pp = base + ((size_t)py * W + px) * 3;
    const bool wide = row_in && px + 3 < W && (((uintptr_t)pp) & 3u) == 0;
    int c00 = 0, c01 = 0, c02 = 0, c10 = 0, c11 = 0, c12 = 0, c20 = 0, c21 = 0, c22 = 0, c30 = 0, c31 = 0, c32 = 0;
    bool loaded = false, dirty = false;

    const int nprim = panel ? DRAW_BEV_PRIMS : DRAW_PRIMS;
    const int items = topk * nprim;
    for (int i0 = 0; i0 < items; i0 += DRAW_THREADS) {
        // ---- binning: one item per thread, in painter's order
        const int i = i0 + tid;
        bool hit = false;
        int4 ea = make_int4(0, 0, 0, 0), eb = make_int4(0, 0, 0, 0);
        uint32_t eh = 0;
        if (i < items) {
            const int s = i / nprim, p = i - s * nprim;
            const float* r = rimg + (size_t)(topk - 1 - s) * 32;
            const float flag = r[31], fc = r[0];
            const bool kept = flag == 2.0f;
            if (flag >= (float)P.min_flag && fc >= 0.0f && fc < (float)P.ncls) {
                const int ci = (int)fc;
                eh = ((uint32_t)P.color[ci][0] << 8) | ((uint32_t)P.color[ci][1] << 16) | ((uint32_t)P.color[ci][2] << 24);
                bool ok = false;
                int x0 = 0, y0 = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0, x3 = 0, y3 = 0, t = P.thickness;
                if (panel) {
                    if (kept) {
                        const double ry = (double)r[30], c = cos(ry), sn = sin(ry);
                        const double hl = (double)r[26] / 2.0, hw = (double)r[25] / 2.0, X = (double)r[27], Z = (double)r[29];
                        // end points a, b of item p: corners k = 0..3 at local (+,+), (-,+), (-,-), (+,-); 4: the centre, 5: mid +x edge
                        const int ka = p, kb = p == 4 ? 5 : ((p + 1) & 3);
                        double u, v;
                        bool oka, okb;
                        {
                            const double lx = ka == 4 ? 0.0 : ((ka == 0 || ka == 3) ? hl : -hl), lz = ka == 4 ? 0.0 : (ka < 2 ? hw : -hw);
                            const double wx = (c * lx + sn * lz) + X, wz = (c * lz - sn * lx) + Z;
                            u = (double)P.bev_w / 2.0 + wx / P.bev_m_per_px; v = (double)P.bev_h - wz / P.bev_m_per_px;
                            const bool a = draw_coord(u, x0), b = draw_coord(v, y0);
                            oka = a && b;
                        }
                        {
                            const double lx = (kb == 0 || kb == 3 || kb == 5) ? hl : -hl, lz = kb == 5 ? 0.0 : (kb < 2 ? hw : -hw);
                            const double wx = (c * lx + sn * lz) + X, wz = (c * lz - sn * lx) + Z;
                            u = (double)P.bev_w / 2.0 + wx / P.bev_m_per_px; v = (double)P.bev_h - wz / P.bev_m_per_px;
                            const bool a = draw_coord(u, x1), b = draw_coord(v, y1);
                            okb = a && b;
                        }
                        ok = oka && okb;
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
                if (ok) {
                    int bx0, bx1, by0, by1;
                    if (eh & 1u) {
                        bx0 = imin(imin(x0, x1), imin(x2, x3)); bx1 = imax(imax(x0, x1), imax(x2, x3));
                        by0 = imin(imin(y0, y1), imin(y2, y3)); by1 = imax(imax(y0, y1), imax(y2, y3));
                        ea = make_int4(x0, y0, x1, y1); eb = make_int4(x2, y2, x3, y3);
                    } else {
                        const int inf = (t + 1) >> 1;
                        bx0 = imin(x0, x1) - inf; bx1 = imax(x0, x1) + inf; by0 = imin(y0, y1) - inf; by1 = imax(y0, y1) + inf;
                        ea = make_int4(x0, y0, x1, y1); eb = make_int4(t * t, inf, 0, 0);
                    }
                    hit = bx0 <= tx1 && bx1 >= tx0 && by0 <= ty1 && by1 >= ty0;
                }
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
        if (!loaded) {
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
        }
        for (int e = 0; e < n; ++e) {
            const int4 a = l_a[e], b = l_b[e];
            const uint32_t h = l_h[e];
            const int r0 = (h >> 8) & 255, r1 = (h >> 16) & 255, r2 = h >> 24;
            bool m0, m1, m2, m3;
            if (h & 1u) {
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
            } else {
                // (t + 1) / 2 >= t / 2: outside the inflated box of the segment nothing is covered
                const int t2 = b.x, inf = b.y;
                if (py < imin(a.y, a.w) - inf || py > imax(a.y, a.w) + inf || px > imax(a.x, a.z) + inf || px + 3 < imin(a.x, a.z) - inf) continue;
                m0 = seg_covers(px, py, a.x, a.y, a.z, a.w, t2);
                m1 = seg_covers(px + 1, py, a.x, a.y, a.z, a.w, t2);
                m2 = seg_covers(px + 2, py, a.x, a.y, a.z, a.w, t2);
                m3 = seg_covers(px + 3, py, a.x, a.y, a.z, a.w, t2);
                if (m0) { c00 = r0; c01 = r1; c02 = r2; }
                if (m1) { c10 = r0; c11 = r1; c12 = r2; }
                if (m2) { c20 = r0; c21 = r1; c22 = r2; }
                if (m3) { c30 = r0; c31 = r1; c32 = r2; }
            }
            dirty = dirty || m0 || m1 || m2 || m3;
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

extern "C" int rtm3d_draw_default_params(rtm3d_draw_params* p) {
    if (!p) { rt_set_error("draw_default_params: null pointer"); return 1; }
    static const uint8_t palette[8][3] = {{255, 64, 64}, {64, 224, 64}, {64, 128, 255}, {255, 208, 0},
                                          {255, 64, 224}, {0, 224, 224}, {255, 144, 32}, {176, 112, 255}};
    p->layers = DRAW_FRAME_LAYERS;
    p->source = 0; p->min_flag = 1; p->thickness = 1; p->radius = 5; p->face_alpha = 77;
    p->ncls = RTM3D_ENGINE_MAX_CLASSES;
    for (int c = 0; c < RTM3D_ENGINE_MAX_CLASSES; ++c)
        for (int k = 0; k < 3; ++k) p->color[c][k] = palette[c & 7][k];
    p->bev_h = 0; p->bev_w = 0; p->bev_m_per_px = 0.0;
    return 0;
}

int draw_check_args(int B, int topk, const float* d_rec, uint8_t* const* h_imgs, const int* h_hw, const double* d_K_camera,
                    const rtm3d_draw_params* params, const uint8_t* d_bev, int max_layers, const char* layer_words, bool panels) {
    if (B < 1 || topk < 1 || topk > 65536) { rt_set_error("records_draw: bad sizes (B %d, topk %d)", B, topk); return 1; }
    if (!d_rec || !h_imgs || !h_hw || !params) { rt_set_error("records_draw: null pointer"); return 1; }
    const rtm3d_draw_params& P = *params;
    if (P.layers < 1 || P.layers > max_layers) { rt_set_error("records_draw: layers %d is not a mask of the %s layers", P.layers, layer_words); return 1; }
    if (P.source != 0 && P.source != 1) { rt_set_error("records_draw: unknown source %d (0 regressed vertices, 1 solved box)", P.source); return 1; }
    if (P.min_flag != 1 && P.min_flag != 2) { rt_set_error("records_draw: min_flag %d (1 every detection, 2 3D-kept only)", P.min_flag); return 1; }
    if (P.thickness < 1 || P.thickness > 15) { rt_set_error("records_draw: thickness %d is outside 1..15", P.thickness); return 1; }
    if (P.radius < 0 || P.radius > DRAW_MAX_RADIUS) { rt_set_error("records_draw: radius %d is outside 0..%d", P.radius, DRAW_MAX_RADIUS); return 1; }
    if (P.face_alpha < 0 || P.face_alpha > 256) { rt_set_error("records_draw: face_alpha %d is outside 0..256", P.face_alpha); return 1; }
    if (P.ncls < 1 || P.ncls > RTM3D_ENGINE_MAX_CLASSES) {
        rt_set_error("records_draw: a colour table of %d classes (1..%d)", P.ncls, RTM3D_ENGINE_MAX_CLASSES); return 1;
    }
    if (P.source == 1 && !d_K_camera) { rt_set_error("records_draw: source 1 projects the solved boxes and needs d_K_camera"); return 1; }
    if (panels) {
        if (!d_bev) { rt_set_error("records_draw: the bird's-eye layer is set and d_bev is NULL"); return 1; }
        if (P.bev_h < 1 || P.bev_w < 1 || P.bev_h > DRAW_MAX_SIDE || P.bev_w > DRAW_MAX_SIDE) {
            rt_set_error("records_draw: a bird's-eye panel of %d x %d (sides 1..%d)", P.bev_h, P.bev_w, DRAW_MAX_SIDE); return 1;
        }
        if (!(P.bev_m_per_px > 0.0) || !(P.bev_m_per_px < 1e300)) { rt_set_error("records_draw: bev_m_per_px %g is not a positive finite scale", P.bev_m_per_px); return 1; }
    }
    for (int b = 0; b < B; ++b) {                                // the whole batch is checked before anything is painted
        const int h = h_hw[2 * b], w = h_hw[2 * b + 1];
        if (h < 1 || w < 1 || h > DRAW_MAX_SIDE || w > DRAW_MAX_SIDE) {
            rt_set_error("records_draw: frame %d is %d x %d; a side must lie in 1..%d", b, h, w, DRAW_MAX_SIDE); return 1;
        }
        if (!h_imgs[b]) { rt_set_error("records_draw: frame %d is a NULL pointer", b); return 1; }
    }
    return 0;
}

extern "C" int rtm3d_records_draw(void* stream, int B, int topk, const float* d_rec, uint8_t* const* h_imgs, const int* h_hw,
                                  const double* d_K_camera, const rtm3d_draw_params* params, uint8_t* d_bev) {
    const bool panels = params && (params->layers & RTM3D_DRAW_BEV) != 0;
    if (draw_check_args(B, topk, d_rec, h_imgs, h_hw, d_K_camera, params, d_bev, DRAW_FRAME_LAYERS | RTM3D_DRAW_BEV, "five", panels)) return 1;
    const rtm3d_draw_params& P = *params;
    const bool frames = (P.layers & DRAW_FRAME_LAYERS) != 0;
    const int bev_tiles = panels ? ((P.bev_w + DRAW_TW - 1) / DRAW_TW) * ((P.bev_h + DRAW_TH - 1) / DRAW_TH) : 0;
    for (int b0 = 0; b0 < B; b0 += DRAW_MAX_BATCH) {
        const int nb = B - b0 < DRAW_MAX_BATCH ? B - b0 : DRAW_MAX_BATCH;
        DrawBatch fb;
        const int tiles = draw_fill_batch(fb, h_imgs, h_hw, b0, nb, frames);
        const int grid = tiles + nb * bev_tiles;                   // <= 64 * 65536 * 2
        hipLaunchKernelGGL(records_draw_kernel, dim3((unsigned)grid), dim3(DRAW_THREADS), 0, (hipStream_t)stream, fb, nb, topk,
                           d_rec + (size_t)b0 * topk * 32, d_K_camera ? d_K_camera + (size_t)b0 * 9 : nullptr, P,
                           panels ? d_bev + (size_t)b0 * P.bev_h * P.bev_w * 3 : nullptr, bev_tiles > 0 ? bev_tiles : 1);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rt_set_error("records_draw launch: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
