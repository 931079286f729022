"""The yardstick of the rig-fusion tests: a numpy fp64 statement of the rule in include/rtm3d_hip.h, "rig fusion", written from
that comment - sequential and obvious: a sorted candidate list, one walk over it, scalar sums in the order the comment gives.
The IoUs come from tests/box_overlap_ref.py, which clips in world coordinates - not the device's arithmetic, agreeing with it to
~1e-14.  tests/test_rig_cpu.py checks this file against closed forms before any device result is compared with it.

``fuse`` runs one call and also returns its smallest decision margin: the minimum over the evaluated pairs of |affinity - thresh|
and over the merged members of the distance of |d_m| from pi / 2.  A comparison with another implementation is only meaningful
on inputs whose margin is well above the arithmetic difference of the two."""
import numpy as np

from tests import box_overlap_ref as bo
from tests.track_ref import wrap, PI, HALF_PI

METRICS = {'bev': 0, 'iou3d': 1, 'dist': 2}
MERGES = {'best': 0, 'mean': 1}
DEFAULTS = dict(metric='bev', thresh=0.1, class_aware=True, cross_only=True, merge='mean', min_score=0.0)


def params(**kw):
    assert not set(kw) - set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def transform(box, e):
    """Step 1: a record's (7,) float64 box through the (12,) extrinsic."""
    e = np.asarray(e, np.float64).reshape(12)
    h, w, l, x, y, z, ry = [np.float64(v) for v in box]
    with np.errstate(invalid='ignore', over='ignore'):
        X = ((e[0] * x + e[1] * y) + e[2] * z) + e[3]
        Y = ((e[4] * x + e[5] * y) + e[6] * z) + e[7]
        Z = ((e[8] * x + e[9] * y) + e[10] * z) + e[11]
        c, s = np.cos(ry), np.sin(ry)
        r = wrap(np.arctan2(-(e[8] * c - e[10] * s), e[0] * c - e[2] * s))
    return np.array([h, w, l, X, Y, Z, r], np.float64)


def affinity(a, b, metric):
    """Step 2 of "tracking" for box a (the earlier one) and box b."""
    with np.errstate(invalid='ignore', over='ignore'):
        ex, ey, ez = a[3] - b[3], a[4] - b[4], a[5] - b[5]
        if metric == 2:
            return -np.sqrt((ex * ex + ey * ey) + ez * ez)
        reach = 0.5 * np.sqrt(a[1] * a[1] + a[2] * a[2]) + 0.5 * np.sqrt(b[1] * b[1] + b[2] * b[2])
        if ex * ex + ez * ez > reach * reach:
            return 0.0
    bev, vol = bo.overlap(a, b)
    return bev if metric == 0 else vol


def candidates(rec, min_score):
    """Steps 1 (selection) and 2: [(camera, slot)] of one rig's (C, topk, 32) records in the order of the rule."""
    rec = np.asarray(rec, np.float32)
    C, topk = rec.shape[:2]
    cand = [(c, k) for c in range(C) for k in range(topk) if rec[c, k, 31] == 2 and np.float64(rec[c, k, 1]) >= min_score]
    cand.sort(key=lambda ck: (-float(rec[ck[0], ck[1], 1]), ck[0], ck[1]))      # -0.0 == 0.0 here as in the fp32 compare
    return cand


def fuse_one(rec, ext, P, cap):
    """One rig: rec (C, topk, 32), ext (C, 12).  Returns (out (cap, 32) f32, box (cap, 7) f64, info (cap, 4) i32, map (C, topk) i32,
    n (2,) i32, margin, clusters) with clusters = [[(camera, slot), ...]] of ALL clusters, representative first."""
    rec = np.asarray(rec, np.float32)
    ext = np.asarray(ext, np.float64).reshape(-1, 12)
    C, topk = rec.shape[:2]
    metric, thresh = METRICS[P['metric']], np.float64(P['thresh'])
    cand = candidates(rec, P['min_score'])
    boxes = [transform(rec[c, k, 24:31].astype(np.float64), ext[c]) for c, k in cand]
    margin = np.inf
    reps, rep_of = [], []
    for i, (ci, ki) in enumerate(cand):
        mine = None
        for j in reps:                                          # ascending: the earliest representative first
            cj, kj = cand[j]
            if P['cross_only'] and ci == cj:
                continue
            if P['class_aware'] and not rec[ci, ki, 0] == rec[cj, kj, 0]:
                continue
            a = affinity(boxes[j], boxes[i], metric)
            if a == a and np.isfinite(a):
                margin = min(margin, abs(float(a - thresh)))
            if a > thresh:
                mine = j
                break
        if mine is None:
            reps.append(i)
            mine = i
        rep_of.append(mine)
    out = np.zeros((cap, 32), np.float32)
    obox = np.zeros((cap, 7), np.float64)
    info = np.zeros((cap, 4), np.int32)
    omap = np.full((C, topk), -1, np.int32)
    clusters = []
    for s, j in enumerate(reps):
        members = [j] + [p for p in range(len(cand)) if rep_of[p] == j and p != j]
        clusters.append([cand[p] for p in members])
        for p in members:
            omap[cand[p]] = s if s < cap else -2
        box = boxes[j].copy()
        if MERGES[P['merge']] == 1:
            with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
                W, sums, sd = None, None, None
                for p in members:
                    w = np.float64(rec[cand[p][0], cand[p][1], 1])
                    d = wrap(boxes[p][6] - boxes[j][6])
                    if p != j and d == d:
                        margin = min(margin, abs(abs(float(d)) - HALF_PI))
                    if d > HALF_PI:
                        d = d - np.float64(PI)
                    elif d < -HALF_PI:
                        d = d + np.float64(PI)
                    terms = [w * boxes[p][a] for a in range(6)]
                    if W is None:
                        W, sums, sd = w, terms, w * d
                    else:
                        W = W + w
                        sums = [sums[a] + terms[a] for a in range(6)]
                        sd = sd + w * d
                box[:6] = [sums[a] / W for a in range(6)]
                box[6] = wrap(boxes[j][6] + sd / W)
        if s < cap:
            cj, kj = cand[j]
            out[s, 0], out[s, 1] = rec[cj, kj, 0], rec[cj, kj, 1]
            with np.errstate(invalid='ignore', over='ignore'):
                out[s, 24:31] = box.astype(np.float32)
            out[s, 31] = 2
            obox[s] = box
            mask = 0
            for c, _ in clusters[-1]:
                mask |= 1 << c
            info[s] = cj, kj, len(members), mask
    n = np.array([min(len(reps), cap), max(len(reps) - cap, 0)], np.int32)
    return out, obox, info, omap, n, margin, clusters


def fuse(rec, ext, R, C, P=None, cap=None):
    """A whole call: rec (R * C, topk, 32), ext (R * C, 12) or (R, C, 3, 4).  Returns a dict of the stacked outputs of the rule
    (out, box, info, map, n), 'margin' (the smallest over the rigs) and 'clusters' per rig."""
    P = params() if P is None else P
    rec = np.asarray(rec, np.float32)
    topk = rec.shape[1]
    ext = np.asarray(ext, np.float64).reshape(R, C, 12)
    cap = min(256, C * topk) if cap is None else cap
    res = [fuse_one(rec[r * C:(r + 1) * C], ext[r], P, cap) for r in range(R)]
    return dict(out=np.stack([x[0] for x in res]), box=np.stack([x[1] for x in res]), info=np.stack([x[2] for x in res]),
                map=np.concatenate([x[3] for x in res]), n=np.stack([x[4] for x in res]), margin=min(x[5] for x in res),
                clusters=[x[6] for x in res])


def scatter_ids(omap, ids_rig, R, C):
    """rtm3d_rig_scatter_ids: omap (R * C, topk), ids_rig (R, cap)."""
    omap = np.asarray(omap)
    out = np.zeros(omap.shape, np.int32)
    for i in range(omap.shape[0]):
        for k in range(omap.shape[1]):
            if omap[i, k] >= 0:
                out[i, k] = ids_rig[i // C, omap[i, k]]
    return out
