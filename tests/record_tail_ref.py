"""The yardstick of the record tail: what include/rtm3d_hip.h says rtm3d_pack_records, rtm3d_project_boxes,
rtm3d_frames_adjust_k and rtm3d_records_to_camera compute, restated as plain loops over Python floats (IEEE binary64) with
``math`` and numpy's scalar roundings only.  Written from the header's text, not from the kernels: one slot, one field, one
corner at a time; no vectorised expression whose operation order numpy chooses.

Conventions (the header's):
  record   32 fp32: [0] class [1] score [2:4] key point [4:20] vertices [20:24] 2D box [24:27] (h, w, l) = x[3], x[4], x[2]
           [27:30] location x[5:8] [30] Ry = atan2(x0, x1) [31] flag 0 empty / 1 2D only / 2 kept (status >= 0 and fun <
           fun_accept); a slot with rank >= n[image] is 32 zeros; without solver outputs [24:31] are zero and the flag 0 / 1
  yaw      ry = atan2(x0, x1), sin / cos of it with |.| < 1e-3 snapped to 0
  corner   c = 0..7 with signs i, j, k in {1, -1} nested (i slowest), c = 8 the centre; (R diag(l, h, w) / 2) signs +
           location, through K, divided by z + 1e-6
  K_net    row 0 / w then * rw, row 1 / h then * rh, then cx + pad_w, cy + pad_h
  camera   (float)(((double)x - pad_w) * ((double)w / (double)rw)) on the even fields of [2:24], y likewise on the odd ones
  row      16 fp64, all zero unless the RECORD's flag is 2 and status >= 0 and fun < fun_accept
Non-finite projections: the device reduces and clips with IEEE fmin / fmax, where a NaN operand loses: the rectangle of eight
corners is NaN only where all eight are, and a NaN rectangle coordinate clips to 0 (fmax(NaN, 0) = 0).  ``fmin`` / ``fmax``
below state that; numpy's minimum / maximum / clip would propagate the NaN instead.

geom is a tuple (h, w, rh, rw, pad_w, pad_h) - the fields of rtm3d_frame_geom in order."""
import math

import numpy as np

PI = 3.141592653589793
SNAP = 1e-3


def f32(v):
    """(float)v: round to nearest even, beyond FLT_MAX to infinity."""
    with np.errstate(over='ignore'):
        return float(np.float32(v))


def div(a, b):
    """IEEE a / b (x / 0 = +-inf, 0 / 0 = NaN) - Python's own raises."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.float64(a) / np.float64(b))


def fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


# ------------------------------------------------------------------------------------------------ the record
def pack_records(n, cls, score, mproj, verts, bbox, topk, x=None, fun=None, status=None, fun_accept=0.1):
    """(B, topk, 32) float32.  n (B,), cls (B*topk,) int64, score (B*topk,), mproj (B*topk, 2), verts (B*topk, 16),
    bbox (B*topk, 4) float32; x (B*topk, 8), fun (B*topk,) float64 and status (B*topk,) int32, or all three None."""
    B = len(n)
    rec = np.zeros((B, topk, 32), np.float32)
    for b in range(B):
        for r in range(topk):
            if r >= int(n[b]):
                continue
            s = b * topk + r
            out = [0.0] * 32
            out[0] = f32(int(cls[s]))
            out[1] = float(score[s])
            out[2:4] = [float(v) for v in mproj[s]]
            out[4:20] = [float(v) for v in verts[s]]
            out[20:24] = [float(v) for v in bbox[s]]
            flag = 1.0
            if x is not None:
                xs = [float(v) for v in x[s]]
                out[24:27] = [f32(xs[3]), f32(xs[4]), f32(xs[2])]
                out[27:30] = [f32(xs[5]), f32(xs[6]), f32(xs[7])]
                out[30] = f32(math.atan2(xs[0], xs[1]))
                if int(status[s]) >= 0 and float(fun[s]) < fun_accept:
                    flag = 2.0
            out[31] = flag
            with np.errstate(over='ignore'):
                rec[b, r] = np.array(out, np.float64).astype(np.float32)       # every entry already is an fp32 value
    return rec


# ------------------------------------------------------------------------------------------------ the projection
def box_yaw(x0, x1, snap=True):
    ry = math.atan2(x0, x1)
    sn, cs = math.sin(ry), math.cos(ry)
    if snap:
        if abs(sn) < SNAP:
            sn = 0.0
        if abs(cs) < SNAP:
            cs = 0.0
    return ry, sn, cs


CORNER_SIGNS = [(i, j, k) for i in (1.0, -1.0) for j in (1.0, -1.0) for k in (1.0, -1.0)] + [(0.0, 0.0, 0.0)]


def project_corner(xs, K, sn, cs, c):
    """(u, v) of corner c of x = [., ., l, h, w, X, Y, Z]: R = [[c, 0, s], [0, 1, 0], [-s, 0, c]], half extents (l, h, w) / 2."""
    sx, sy, sz = CORNER_SIGNS[c]
    dx, dy, dz = xs[2] / 2, xs[3] / 2, xs[4] / 2
    X = (cs * dx) * sx + (sn * dz) * sz + xs[5]
    Y = dy * sy + xs[6]
    Z = (-sn * dx) * sx + (cs * dz) * sz + xs[7]
    pu = K[0] * X + K[1] * Y + K[2] * Z
    pv = K[3] * X + K[4] * Y + K[5] * Z
    pw = K[6] * X + K[7] * Y + K[8] * Z
    return div(pu, pw + 1e-6), div(pv, pw + 1e-6)


def project_box(xs, K, snap=True):
    """(proj [9][2], rect [x1, y1, x2, y2]): the nine projections and the bounding rectangle of the first eight."""
    xs, K = [float(v) for v in xs], [float(v) for v in K]
    _, sn, cs = box_yaw(xs[0], xs[1], snap)
    proj = [project_corner(xs, K, sn, cs, c) for c in range(9)]
    x1, y1 = proj[0]
    x2, y2 = proj[0]
    for u, v in proj[1:8]:
        x1, y1, x2, y2 = fmin(x1, u), fmin(y1, v), fmax(x2, u), fmax(y2, v)
    return proj, [x1, y1, x2, y2]


def project_boxes(x, status, K, topk, snap=True):
    """rtm3d_project_boxes: (N, 9, 2), (N, 4); K one row per slot (topk == 0) or per image of topk slots; status < 0: zeros."""
    N = len(x)
    proj, rect = np.zeros((N, 9, 2)), np.zeros((N, 4))
    for s in range(N):
        if int(status[s]) < 0:
            continue
        p, r = project_box(x[s], K[s // topk if topk > 0 else s], snap)
        proj[s], rect[s] = p, r
    return proj, rect


# ------------------------------------------------------------------------------------------------ the camera frame
def k_net(K, geom):
    h, w, rh, rw, pad_w, pad_h = [float(v) for v in geom]
    out = [float(v) for v in K]
    for e in range(3):
        out[e] = out[e] / w
        out[e] = out[e] * rw
    for e in range(3, 6):
        out[e] = out[e] / h
        out[e] = out[e] * rh
    out[2] = out[2] + pad_w
    out[5] = out[5] + pad_h
    return out


def to_camera(rec, geoms):
    """(B, topk, 32) canvas records -> the records in the pixels of each frame; slots with flag < 1 are not touched."""
    out = np.array(rec, np.float32)
    for b, g in enumerate(geoms):
        h, w, rh, rw, pad_w, pad_h = [float(v) for v in g]
        for r in range(rec.shape[1]):
            if not float(rec[b, r, 31]) >= 1.0:
                continue
            for f in range(2, 24):
                v = float(rec[b, r, f])
                out[b, r, f] = np.float32((v - pad_w) * (w / rw) if f % 2 == 0 else (v - pad_h) * (h / rh))
    return out


def kept(flag, status, fun, fun_accept):
    return float(flag) == 2.0 and int(status) >= 0 and float(fun) < fun_accept


def kitti_row(slot, xs, K, geom, clip=True, snap=True):
    """The 16 numbers of a kept slot; slot = its 32-float record (class and score are read from it)."""
    xs = [float(v) for v in xs]
    ry = math.atan2(xs[0], xs[1])
    _, (x1, y1, x2, y2) = project_box(xs, K, snap)
    if clip:
        xmax, ymax = float(geom[1] - 1), float(geom[0] - 1)
        x1, x2 = fmin(fmax(x1, 0.0), xmax), fmin(fmax(x2, 0.0), xmax)
        y1, y2 = fmin(fmax(y1, 0.0), ymax), fmin(fmax(y2, 0.0), ymax)
    a = math.fmod(ry - math.atan2(xs[5], xs[7]) + PI, 2 * PI)
    if a < 0.0:
        a += 2 * PI
    return [float(slot[0]), a - PI, x1, y1, x2, y2, xs[3], xs[4], xs[2], xs[5], xs[6] + xs[3] / 2.0, xs[7], ry, float(slot[1]), 2.0, 0.0]


def kitti_rows(rec, x, fun, status, K_cam, geoms, fun_accept=0.1, clip=True, snap=True):
    """(B, topk, 16) rows for CANVAS or camera records (only [0], [1] and the flag [31] of a record are read)."""
    B, topk = rec.shape[:2]
    rows = np.zeros((B, topk, 16))
    for b in range(B):
        for r in range(topk):
            s = b * topk + r
            if kept(rec[b, r, 31], status[s], fun[s], fun_accept):
                rows[b, r] = kitti_row(rec[b, r], x[s], K_cam[b], geoms[b], clip, snap)
    return rows


def unwrapped_alpha(xs):
    return math.atan2(xs[0], xs[1]) - math.atan2(xs[5], xs[7])
