"""The yardstick of the box-overlap tests: an independent fp64 numpy statement of rotated-box overlaps and greedy NMS,
written for these tests (not a port of the device code: it clips in WORLD coordinates against B's directed edges, the device
code clips in B's own frame against axis-aligned bounds).

Box = (h, w, l, X, Y, Z, ry): centre (X, Y, Z), footprint l x w in the x-z plane, corners
(X, Z) + R (+-l/2, +-w/2) with R = [[c, s], [-s, c]], plain c = cos(ry), s = sin(ry); vertical extent [Y - h/2, Y + h/2].
tests/test_box_overlap_cpu.py checks this file against closed forms before any device result is compared with it.
"""
import numpy as np

CRITERIA = ('iou', 'a', 'b')


def valid(box):
    box = np.asarray(box, np.float64)
    return bool(np.all(np.isfinite(box)) and np.all(box[:3] > 0))


def footprint(box):
    """(4, 2) corners (x, z), in a fixed rotational order."""
    h, w, l, X, Y, Z, ry = [float(v) for v in box]
    c, s = np.cos(ry), np.sin(ry)
    loc = np.array([[l / 2, w / 2], [-l / 2, w / 2], [-l / 2, -w / 2], [l / 2, -w / 2]])
    R = np.array([[c, s], [-s, c]])
    return loc @ R.T + np.array([X, Z])


def _area(poly):
    if len(poly) < 3:
        return 0.0
    x, z = poly[:, 0], poly[:, 1]
    return 0.5 * abs(float(np.sum(x * np.roll(z, -1) - z * np.roll(x, -1))))


def clip_polygon(subject, clipper):
    """Sutherland-Hodgman: the convex polygon ``subject`` inside the convex polygon ``clipper`` (closed inside test)."""
    if _signed(clipper) < 0:
        clipper = clipper[::-1]
    out = [p for p in subject]
    for k in range(len(clipper)):
        e0, e1 = clipper[k], clipper[(k + 1) % len(clipper)]
        d = e1 - e0
        side = lambda p: d[0] * (p[1] - e0[1]) - d[1] * (p[0] - e0[0])       # >= 0: left of e0 -> e1, inside (CCW clipper)
        inp, out = out, []
        for i in range(len(inp)):
            cur, prev = inp[i], inp[i - 1]
            sc, sp = side(cur), side(prev)
            if sc >= 0:
                if sp < 0:
                    out.append(prev + (cur - prev) * (sp / (sp - sc)))
                out.append(cur)
            elif sp >= 0:
                out.append(prev + (cur - prev) * (sp / (sp - sc)))
        if not out:
            break
    return np.array(out, np.float64).reshape(-1, 2)


def _signed(poly):
    x, z = poly[:, 0], poly[:, 1]
    return float(np.sum(x * np.roll(z, -1) - z * np.roll(x, -1)))


def pair(a, b):
    """(BEV intersection area, vertical overlap, footprint area a, footprint area b); zeros for an invalid box."""
    if not (valid(a) and valid(b)):
        return 0.0, 0.0, 0.0, 0.0
    inter = _area(clip_polygon(footprint(a), footprint(b)))
    ov = max(0.0, min(a[4] + a[0] / 2, b[4] + b[0] / 2) - max(a[4] - a[0] / 2, b[4] - b[0] / 2))
    return inter, ov, float(a[2] * a[1]), float(b[2] * b[1])


def _ratio(inter, sa, sb, criterion):
    den = {'iou': sa + sb - inter, 'a': sa, 'b': sb}[criterion]
    return inter / den if den > 0 else 0.0


def overlap(a, b, criterion='iou'):
    """(bev, vol) overlap of two boxes."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    inter, ov, sa, sb = pair(a, b)
    if not (valid(a) and valid(b)):
        return 0.0, 0.0
    return _ratio(inter, sa, sb, criterion), _ratio(inter * ov, sa * a[0], sb * b[0], criterion)


def overlaps(A, Bx, na=None, nb=None, criterion='iou'):
    """(B, cap_a, cap_b) BEV and 3D matrices; entries beyond the counts are 0."""
    A, Bx = np.asarray(A, np.float64), np.asarray(Bx, np.float64)
    B, ca, cb = A.shape[0], A.shape[1], Bx.shape[1]
    na = [ca] * B if na is None else na
    nb = [cb] * B if nb is None else nb
    bev, vol = np.zeros((B, ca, cb)), np.zeros((B, ca, cb))
    for m in range(B):
        for i in range(int(na[m])):
            for j in range(int(nb[m])):
                bev[m, i, j], vol[m, i, j] = overlap(A[m, i], Bx[m, j], criterion)
    return bev, vol


def record_ious(rec):
    """(bev, vol): two (topk, topk) IoU matrices between the flag-2 slots of one image's records (0 elsewhere), on
    double(rec[:, 24:31]).  Pairs whose footprints cannot meet (centres further apart than the two half diagonals) are 0
    without clipping."""
    rec = np.asarray(rec)
    n = rec.shape[0]
    box = rec[:, 24:31].astype(np.float64)
    cand = rec[:, 31] == 2
    with np.errstate(invalid='ignore'):
        reach = 0.5 * np.hypot(box[:, 1], box[:, 2])
    bev, vol = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            if cand[i] and cand[j] and not np.hypot(box[i, 3] - box[j, 3], box[i, 5] - box[j, 5]) > reach[i] + reach[j]:
                bev[i, j], vol[i, j] = overlap(box[i], box[j])
                bev[j, i], vol[j, i] = bev[i, j], vol[i, j]
    return bev, vol


def nms_flags(rec, iou_thresh, ious, class_aware=False):
    """The flags [31] of one image's (topk, 32) records after greedy NMS in slot order: a flag-2 slot becomes 1 when an
    earlier SURVIVING flag-2 slot (of the same class, if class_aware) has IoU (``ious``: one matrix of record_ious) strictly
    greater than iou_thresh with it."""
    rec = np.asarray(rec)
    flags = rec[:, 31].copy()
    kept = []
    for i in range(rec.shape[0]):
        if flags[i] != 2:
            continue
        if any(ious[j, i] > iou_thresh and (not class_aware or rec[j, 0] == rec[i, 0]) for j in kept):
            flags[i] = 1
        else:
            kept.append(i)
    return flags


def min_edge_angle(a, b):
    """Smallest angle (rad) between an edge direction of a and one of b: their yaws modulo pi/2, folded to [0, pi/4]."""
    d = (float(a[6]) - float(b[6])) % (np.pi / 2)
    return min(d, np.pi / 2 - d)
