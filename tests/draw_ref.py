"""numpy yardstick of the drawing rule (include/rtm3d_hip.h, "drawing"), written the other way round from csrc/draw.hip: a
SCATTER that paints primitive by primitive, sequentially, in painter's order - slots from the last to the first; per slot the
face shade, the 2D box, the wireframe, the key-point disc - each primitive over its own bounding box.  It shares no structure
with the kernel's per-pixel gather (no tiles, no lists, no binning), so agreement between the two means something.
All coverage tests are exact integers (int64 arrays)."""
import math

import numpy as np

FACE, BOX2D, WIREFRAME, KEYPOINT, BEV = 1, 2, 4, 8, 16
LIMIT = 8192
EDGES = ((0, 1), (1, 3), (3, 2), (2, 0), (0, 4), (4, 5), (5, 7), (7, 6), (6, 4), (5, 1), (3, 7), (6, 2))
DEFAULTS = dict(layers=FACE | BOX2D | WIREFRAME | KEYPOINT, source=0, min_flag=1, thickness=1, radius=5, face_alpha=77, colors=None,
                bev_hw=(400, 400), bev_m_per_px=0.2)


def coord(v):
    """Truncation toward zero, or None for a coordinate that is not finite or whose integer lies outside [-8192, 8192]."""
    v = float(v)
    if not math.isfinite(v):
        return None
    i = int(v)
    return i if -LIMIT <= i <= LIMIT else None


def point(x, y):
    x, y = coord(x), coord(y)
    return None if x is None or y is None else (x, y)


def paint_segment(img, P, Q, t, colour):
    """Opaque thick segment; returns the number of pixels covered."""
    if P is None or Q is None:
        return 0
    h, w = img.shape[:2]
    inf = (t + 1) // 2
    x0, x1 = max(min(P[0], Q[0]) - inf, 0), min(max(P[0], Q[0]) + inf, w - 1)
    y0, y1 = max(min(P[1], Q[1]) - inf, 0), min(max(P[1], Q[1]) + inf, h - 1)
    if x0 > x1 or y0 > y1:
        return 0
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    dx, dy = Q[0] - P[0], Q[1] - P[1]
    vx, vy = xs - P[0], ys - P[1]
    k, dd = vx * dx + vy * dy, dx * dx + dy * dy
    head = 4 * (vx * vx + vy * vy) <= t * t
    tail = 4 * ((xs - Q[0]) ** 2 + (ys - Q[1]) ** 2) <= t * t
    body = (2 * (vx * dy - vy * dx)) ** 2 <= t * t * dd
    m = np.where(k <= 0, head, np.where(k >= dd, tail, body))
    img[y0:y1 + 1, x0:x1 + 1][m] = colour
    return int(m.sum())


def _tri(xs, ys, a, b, c):
    if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) == 0:
        return np.zeros(xs.shape, bool)
    e = [(q[0] - p[0]) * (ys - p[1]) - (q[1] - p[1]) * (xs - p[0]) for p, q in ((a, b), (b, c), (c, a))]
    return ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))


def paint_face(img, quad, colour, alpha):
    """Shade of the quadrilateral quad = vertices (0, 1, 3, 2); returns the number of pixels covered."""
    if any(q is None for q in quad):
        return 0
    h, w = img.shape[:2]
    x0, x1 = max(min(q[0] for q in quad), 0), min(max(q[0] for q in quad), w - 1)
    y0, y1 = max(min(q[1] for q in quad), 0), min(max(q[1] for q in quad), h - 1)
    if x0 > x1 or y0 > y1:
        return 0
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    m = _tri(xs, ys, quad[0], quad[1], quad[2]) | _tri(xs, ys, quad[0], quad[2], quad[3])
    sub = img[y0:y1 + 1, x0:x1 + 1]
    new = (sub.astype(np.int64) * (256 - alpha) + np.asarray(colour, np.int64) * alpha + 128) >> 8
    sub[m] = new[m].astype(np.uint8)
    return int(m.sum())


def project_corners(r, K):
    """The solved box of record r through K (9,) fp64: ((8, 2) fp64 pixels, (8,) fp64 camera depths) in the corner order and
    operation sequence of csrc/box_project.h, fed with plain sin(ry), cos(ry)."""
    r = np.asarray(r, np.float32).astype(np.float64)
    K = np.asarray(K, np.float64)
    hh, ww, ll, X0, Y0, Z0, ry = r[24:31]
    sn, cs = np.sin(ry), np.cos(ry)
    dx, dy, dz = ll / 2, hh / 2, ww / 2
    uv, depth = np.zeros((8, 2)), np.zeros(8)
    with np.errstate(all='ignore'):
        for c in range(8):
            sx, sy, sz = (-1.0 if c & 4 else 1.0), (-1.0 if c & 2 else 1.0), (-1.0 if c & 1 else 1.0)
            X = (cs * dx) * sx + (sn * dz) * sz + X0
            Y = dy * sy + Y0
            Z = (-sn * dx) * sx + (cs * dz) * sz + Z0
            pu, pv, pw = K[0] * X + K[1] * Y + K[2] * Z, K[3] * X + K[4] * Y + K[5] * Z, K[6] * X + K[7] * Y + K[8] * Z
            uv[c] = pu / (pw + 1e-6), pv / (pw + 1e-6)
            depth[c] = Z
    return uv, depth


def bev_points(r, bev_hw, m):
    """(6, 2) fp64 panel coordinates of record r: the four footprint corners, the centre, the midpoint of the +x edge."""
    r = np.asarray(r, np.float32).astype(np.float64)
    ww, ll, X, Z, ry = r[25], r[26], r[27], r[29], r[30]
    c, s = np.cos(ry), np.sin(ry)
    hl, hw = ll / 2.0, ww / 2.0
    out = np.zeros((6, 2))
    with np.errstate(all='ignore'):
        for i, (lx, lz) in enumerate(((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw), (0.0, 0.0), (hl, 0.0))):
            wx, wz = (c * lx + s * lz) + X, (c * lz - s * lx) + Z
            out[i] = bev_hw[1] / 2.0 + wx / m, float(bev_hw[0]) - wz / m
    return out


def draw(images, rec, K=None, bev=None, **params):
    """Paint ``images`` (list of uint8 (h, w, 3) arrays) and ``bev`` ((B, bh, bw, 3) or None) IN PLACE from rec (B, topk, 32).
    Returns {layer bit: pixels covered inside the images} (compounded coverage counted once per primitive)."""
    p = dict(DEFAULTS)
    p.update(params)
    colors = p['colors']
    rec = np.asarray(rec, np.float32)
    stats = {FACE: 0, BOX2D: 0, WIREFRAME: 0, KEYPOINT: 0, BEV: 0}
    for b, img in enumerate(images):
        for slot in range(rec.shape[1] - 1, -1, -1):
            r = rec[b, slot]
            if not r[31] >= p['min_flag'] or not (r[0] >= 0 and r[0] < len(colors)):
                continue
            colour = np.asarray(colors[int(r[0])], np.uint8)
            verts = None
            if p['source'] == 0:
                verts = [point(r[4 + 2 * i], r[5 + 2 * i]) for i in range(8)]
            elif r[31] == 2 and p['layers'] & (FACE | WIREFRAME):
                uv, depth = project_corners(r, K[b])
                if np.all(depth >= 0.1):
                    verts = [point(u, v) for u, v in uv]
            if p['layers'] & FACE and verts is not None:
                stats[FACE] += paint_face(img, [verts[0], verts[1], verts[3], verts[2]], colour, p['face_alpha'])
            if p['layers'] & BOX2D:
                x1, y1, x2, y2 = [coord(v) for v in r[20:24]]
                for P, Q in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
                    if None not in P and None not in Q:
                        stats[BOX2D] += paint_segment(img, P, Q, p['thickness'], colour)
            if p['layers'] & WIREFRAME and verts is not None:
                for i, j in EDGES:
                    stats[WIREFRAME] += paint_segment(img, verts[i], verts[j], p['thickness'], colour)
            if p['layers'] & KEYPOINT:
                c = point(r[2], r[3])
                stats[KEYPOINT] += paint_segment(img, c, c, 2 * p['radius'], colour)
        if p['layers'] & BEV:
            for slot in range(rec.shape[1] - 1, -1, -1):
                r = rec[b, slot]
                if r[31] != 2 or not r[31] >= p['min_flag'] or not (r[0] >= 0 and r[0] < len(colors)):
                    continue
                colour = np.asarray(colors[int(r[0])], np.uint8)
                q = [point(u, v) for u, v in bev_points(r, p['bev_hw'], p['bev_m_per_px'])]
                for i, j in ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5)):
                    stats[BEV] += paint_segment(bev[b], q[i], q[j], 1, colour)
    return stats
