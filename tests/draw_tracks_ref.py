"""numpy yardstick of rtm3d_records_draw_tracks, written from include/rtm3d_hip.h, "drawing tracks" (and "drawing", through
tests/draw_ref.py, for segments, faces and coordinates).  Like tests/draw_ref.py it is a SCATTER: primitive by primitive, in
painter's order, each over its own bounding box - no tiles, no lists, no binning.  The font is drawn here a second time, as
'#' / '.' art; tests/test_draw_tracks_cpu.py compares it with the library's table.  Nothing of rtm3d_amd is imported."""
import numpy as np

from tests import draw_ref as ref

FACE, BOX2D, WIREFRAME, KEYPOINT, BEV, LABEL, TRACK_BEV = 1, 2, 4, 8, 16, 32, 64
HEADER, SLOT = 8, 24
CHARS = ' 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#?.%-:/'
DEFAULTS = dict(ref.DEFAULTS, palette=None, label_fields=3, font_scale=1, names=None, bev_fade=256, vel_horizon=1.0)

_ART = """
 |.....|.....|.....|.....|.....|.....|.....
0|.###.|#...#|#..##|#.#.#|##..#|#...#|.###.
1|..#..|.##..|..#..|..#..|..#..|..#..|.###.
2|.###.|#...#|....#|...#.|..#..|.#...|#####
3|#####|...#.|..#..|...#.|....#|#...#|.###.
4|...#.|..##.|.#.#.|#..#.|#####|...#.|...#.
5|#####|#....|####.|....#|....#|#...#|.###.
6|..##.|.#...|#....|####.|#...#|#...#|.###.
7|#####|....#|...#.|..#..|.#...|.#...|.#...
8|.###.|#...#|#...#|.###.|#...#|#...#|.###.
9|.###.|#...#|#...#|.####|....#|...#.|.##..
A|.###.|#...#|#...#|#####|#...#|#...#|#...#
B|####.|#...#|#...#|####.|#...#|#...#|####.
C|.###.|#...#|#....|#....|#....|#...#|.###.
D|###..|#..#.|#...#|#...#|#...#|#..#.|###..
E|#####|#....|#....|####.|#....|#....|#####
F|#####|#....|#....|####.|#....|#....|#....
G|.###.|#...#|#....|#.###|#...#|#...#|.####
H|#...#|#...#|#...#|#####|#...#|#...#|#...#
I|.###.|..#..|..#..|..#..|..#..|..#..|.###.
J|..###|...#.|...#.|...#.|...#.|#..#.|.##..
K|#...#|#..#.|#.#..|##...|#.#..|#..#.|#...#
L|#....|#....|#....|#....|#....|#....|#####
M|#...#|##.##|#.#.#|#.#.#|#...#|#...#|#...#
N|#...#|#...#|##..#|#.#.#|#..##|#...#|#...#
O|.###.|#...#|#...#|#...#|#...#|#...#|.###.
P|####.|#...#|#...#|####.|#....|#....|#....
Q|.###.|#...#|#...#|#...#|#.#.#|#..#.|.##.#
R|####.|#...#|#...#|####.|#.#..|#..#.|#...#
S|.####|#....|#....|.###.|....#|....#|####.
T|#####|..#..|..#..|..#..|..#..|..#..|..#..
U|#...#|#...#|#...#|#...#|#...#|#...#|.###.
V|#...#|#...#|#...#|#...#|#...#|.#.#.|..#..
W|#...#|#...#|#...#|#.#.#|#.#.#|#.#.#|.#.#.
X|#...#|#...#|.#.#.|..#..|.#.#.|#...#|#...#
Y|#...#|#...#|#...#|.#.#.|..#..|..#..|..#..
Z|#####|....#|...#.|..#..|.#...|#....|#####
#|.#.#.|.#.#.|#####|.#.#.|#####|.#.#.|.#.#.
?|.###.|#...#|....#|...#.|..#..|.....|..#..
.|.....|.....|.....|.....|.....|.##..|.##..
%|##..#|##..#|...#.|..#..|.#...|#..##|#..##
-|.....|.....|.....|#####|.....|.....|.....
:|.....|.##..|.##..|.....|.##..|.##..|.....
/|....#|....#|...#.|..#..|.#...|#....|#....
"""
# ART[ch] = 7 strings of 5 characters, top row first, left column first
ART = {ln[0]: ln[2:].split('|') for ln in _ART.strip('\n').split('\n')}
assert ''.join(ART) == CHARS and all(len(g) == 7 and all(len(r) == 5 for r in g) for g in ART.values())


def font_rows(ch):
    """The seven row values of the header: 5 low bits, bit 4 the left column."""
    return [sum(16 >> c for c in range(5) if row[c] == '#') for row in ART[ch]]


def fold(byte):
    """A byte of a class name as the character that is drawn."""
    c = chr(byte) if isinstance(byte, int) else byte
    if 'a' <= c <= 'z':
        c = c.upper()
    return c if c in CHARS else '?'


def label_text(fields, tid, name, score, z, kept=True):
    """The text of a label: fields in mask order, one space between, empty fields left out."""
    out = []
    tid = int(tid)
    if fields & 1 and tid != 0:
        out.append(('?' if tid < 0 else '#') + str(abs(tid) % 10 ** 7))
    if fields & 2:
        name = bytes(name)[:7].split(b'\0')[0]
        if name:
            out.append(''.join(fold(b) for b in name))
    if fields & 4:
        v = np.float64(np.float32(score)) * np.float64(100.0)
        out.append('%02d%%' % (0 if not v >= 0 else 99 if v >= 99 else int(v)))
    if fields & 8 and kept:
        v = np.float64(np.float32(z)) * np.float64(10.0)
        n = 0 if not v >= 0 else 9999 if v >= 9999 else int(v)
        out.append('%d.%dM' % (n // 10, n % 10))
    return ' '.join(out)


def id_colour(palette, tid, tentative):
    c = np.asarray(palette[(abs(int(tid)) - 1) % len(palette)], np.int64)
    return ((c + 1) >> 1 if tentative else c).astype(np.uint8)


def ink(bg):
    bg = [int(v) for v in bg]
    return (0, 0, 0) if 299 * bg[0] + 587 * bg[1] + 114 * bg[2] >= 128000 else (255, 255, 255)


def _ok(*v):
    return all(-ref.LIMIT <= i <= ref.LIMIT for i in v)


def paint_rect(img, x0, y0, x1, y1, colour):
    """Opaque rectangle of the columns x0..x1 and rows y0..y1, both inclusive; returns the pixels covered."""
    if not _ok(x0, y0, x1, y1):
        return 0
    h, w = img.shape[:2]
    xa, xb, ya, yb = max(x0, 0), min(x1, w - 1), max(y0, 0), min(y1, h - 1)
    if xa > xb or ya > yb:
        return 0
    img[ya:yb + 1, xa:xb + 1] = colour
    return (xb - xa + 1) * (yb - ya + 1)


def paint_glyph(img, ch, ax, ay, s, colour):
    """Glyph ch with its top-left pixel at (ax, ay), every glyph pixel an s x s block; returns the pixels covered."""
    if not _ok(ax, ay, ax + 5 * s - 1, ay + 7 * s - 1):
        return 0
    h, w = img.shape[:2]
    n = 0
    for gy, row in enumerate(ART[ch]):
        for gx, bit in enumerate(row):
            if bit == '#':
                for y in range(ay + gy * s, ay + gy * s + s):
                    for x in range(ax + gx * s, ax + gx * s + s):
                        if 0 <= x < w and 0 <= y < h:
                            img[y, x] = colour
                            n += 1
    return n


def paint_text(img, text, tx, ty, s, colour):
    return sum(paint_glyph(img, ch, tx + 6 * s * i, ty, s, colour) for i, ch in enumerate(text))


def label_box(x1, y1, n, s):
    """Inclusive extents (x0, y0, x1, y1) of the background of a label of n characters anchored at the box corner (x1, y1)."""
    top = y1 - 9 * s
    if top < 0:
        top = y1
    return x1, top, x1 + (6 * n + 1) * s - 1, top + 9 * s - 1


def paint_label(img, text, x1, y1, s, colour):
    """Background and glyphs of one label; returns (background pixels, glyph pixels)."""
    if not text:
        return 0, 0
    bx0, by0, bx1, by1 = label_box(x1, y1, len(text), s)
    return paint_rect(img, bx0, by0, bx1, by1, colour), paint_text(img, text, bx0 + s, by0 + s, s, ink(colour))


def track_points(slot, bev_hw, m, vel_horizon):
    """(7, 2) fp64 panel coordinates of a table slot: four footprint corners, the centre, the midpoint of the +x edge, the end of
    the velocity mark."""
    ww, ll, X, Z, ry = slot[8], slot[9], slot[10], slot[12], slot[13]
    c, s = np.cos(ry), np.sin(ry)
    hl, hw = ll / 2.0, ww / 2.0
    out = np.zeros((7, 2))
    with np.errstate(all='ignore'):
        for i, (lx, lz) in enumerate(((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw), (0.0, 0.0), (hl, 0.0))):
            wx, wz = (c * lx + s * lz) + X, (c * lz - s * lx) + Z
            out[i] = bev_hw[1] / 2.0 + wx / m, float(bev_hw[0]) - wz / m
        ex, ez = X + slot[14] * vel_horizon, Z + slot[16] * vel_horizon
        out[6] = bev_hw[1] / 2.0 + ex / m, float(bev_hw[0]) - ez / m
    return out


def live(slot):
    return bool(slot[0] >= 1 and slot[0] < 2.0 ** 31)


def draw(images, rec, ids, K=None, bev=None, state=None, **params):
    """Paint ``images`` and ``bev`` IN PLACE from rec (B, topk, 32), ids (B, topk) and, for TRACK_BEV, state (B, 8 + 24 T)
    fp64.  Returns {name: pixels covered}: the layer bits of draw_ref plus 'label_bg', 'label_glyph', 'track_box', 'track_head',
    'track_vel', 'track_text'."""
    p = dict(DEFAULTS)
    p.update(params)
    colors, palette, layers, s = p['colors'], p['palette'], p['layers'], p['font_scale']
    rec = np.asarray(rec, np.float32)
    ids = np.asarray(ids, np.int64)
    stats = {FACE: 0, BOX2D: 0, WIREFRAME: 0, KEYPOINT: 0, BEV: 0, 'label_bg': 0, 'label_glyph': 0, 'track_box': 0, 'track_head': 0,
             'track_vel': 0, 'track_text': 0}
    topk = rec.shape[1]

    def painted(r):
        return bool(r[31] >= p['min_flag']) and bool(r[0] >= 0 and r[0] < len(colors))

    def colour_of(b, slot):
        t = ids[b, slot]
        return np.asarray(colors[int(rec[b, slot, 0])], np.uint8) if t == 0 else id_colour(palette, t, t < 0)

    if layers & (BEV | TRACK_BEV) and p['bev_fade'] < 256:
        bev[...] = ((bev.astype(np.int64) * p['bev_fade'] + 128) >> 8).astype(np.uint8)
    for b, img in enumerate(images):
        for slot in range(topk - 1, -1, -1):
            r = rec[b, slot]
            if not painted(r):
                continue
            colour = colour_of(b, slot)
            verts = None
            if p['source'] == 0:
                verts = [ref.point(r[4 + 2 * i], r[5 + 2 * i]) for i in range(8)]
            elif r[31] == 2 and layers & (FACE | WIREFRAME):
                uv, depth = ref.project_corners(r, K[b])
                if np.all(depth >= 0.1):
                    verts = [ref.point(u, v) for u, v in uv]
            if layers & FACE and verts is not None:
                stats[FACE] += ref.paint_face(img, [verts[0], verts[1], verts[3], verts[2]], colour, p['face_alpha'])
            if layers & BOX2D:
                x1, y1, x2, y2 = [ref.coord(v) for v in r[20:24]]
                for P, Q in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
                    if None not in P and None not in Q:
                        stats[BOX2D] += ref.paint_segment(img, P, Q, p['thickness'], colour)
            if layers & WIREFRAME and verts is not None:
                for i, j in ref.EDGES:
                    stats[WIREFRAME] += ref.paint_segment(img, verts[i], verts[j], p['thickness'], colour)
            if layers & KEYPOINT:
                c = ref.point(r[2], r[3])
                stats[KEYPOINT] += ref.paint_segment(img, c, c, 2 * p['radius'], colour)
        if layers & LABEL:                       # the second pass: every label lies over every box
            for slot in range(topk - 1, -1, -1):
                r = rec[b, slot]
                anchor = ref.point(r[20], r[21])
                if not painted(r) or anchor is None:
                    continue
                text = label_text(p['label_fields'], ids[b, slot], p['names'][int(r[0])], r[1], r[29], kept=bool(r[31] == 2))
                n = paint_label(img, text, anchor[0], anchor[1], s, colour_of(b, slot))
                stats['label_bg'] += n[0]
                stats['label_glyph'] += n[1]
        if layers & BEV:
            for slot in range(topk - 1, -1, -1):
                r = rec[b, slot]
                if r[31] != 2 or not painted(r):
                    continue
                q = [ref.point(u, v) for u, v in ref.bev_points(r, p['bev_hw'], p['bev_m_per_px'])]
                for i, j in ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5)):
                    stats[BEV] += ref.paint_segment(bev[b], q[i], q[j], 1, colour_of(b, slot))
        if layers & TRACK_BEV:
            table = np.asarray(state[b], np.float64)[HEADER:].reshape(-1, SLOT)
            for t in range(table.shape[0] - 1, -1, -1):
                sl = table[t]
                if not live(sl):
                    continue
                tentative = bool(sl[3] < 1)
                colour = id_colour(palette, int(sl[0]), tentative)
                q = [ref.point(u, v) for u, v in track_points(sl, p['bev_hw'], p['bev_m_per_px'], p['vel_horizon'])]
                for i, j in ((0, 1), (1, 2), (2, 3), (3, 0)):
                    stats['track_box'] += ref.paint_segment(bev[b], q[i], q[j], 1, colour)
                stats['track_head'] += ref.paint_segment(bev[b], q[4], q[5], 1, colour)
                if p['vel_horizon'] > 0:
                    stats['track_vel'] += ref.paint_segment(bev[b], q[4], q[6], 1, colour)
                if p['label_fields'] & 1 and q[4] is not None:
                    text = label_text(1, -int(sl[0]) if tentative else int(sl[0]), b'', 0.0, 0.0)
                    stats['track_text'] += paint_text(bev[b], text, q[4][0], q[4][1], s, colour)
    return stats
