"""The yardstick of the KITTI evaluation tests: the protocol as plain loops over Python lists, written for reading (not a
port of rtm3d_amd/kitti_eval.py or of the kernel: the matching here is the devkit's SEQUENTIAL walk over the detections with
its running ``max_overlap`` / ``assigned_ignored_det`` state, the kernel uses the closed form of its outcome).

A frame is a list of objects; an object is a dict with 'type', 'truncation', 'occlusion', 'alpha', 'rect' (x1, y1, x2, y2),
'hwl', 'xyz' (bottom face), 'ry', 'score'.  Overlap matrices are indexed [detection][ground truth] and are GIVEN: this file
computes no box overlap except ``rect_overlap``, the rectangle rule of include/rtm3d_hip.h.
"""
import math

import numpy as np

MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
NO_DETECTION = None


def rect_overlap(a, b, criterion):
    if not all(math.isfinite(v) for v in list(a) + list(b)):
        return 0.0
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    sa = (a[2] - a[0]) * (a[3] - a[1])
    sb = (b[2] - b[0]) * (b[3] - b[1])
    den = (sa + sb - inter, sa, sb)[criterion]
    if den == 0 or not math.isfinite(den):
        return 0.0
    return inter / den


def clean_frame(gts, dets, cls, d):
    """(gflag list, dflag list, indices of the DontCare ground truths, number of counted ground truths)."""
    cls = cls.lower()
    neighbour = {'car': 'van', 'pedestrian': 'person_sitting'}.get(cls)
    gflag, dontcare, n_gt = [], [], 0
    for i, g in enumerate(gts):
        t = g['type'].lower()
        if t == cls:
            valid = 1
        elif neighbour is not None and t == neighbour:
            valid = 0
        else:
            valid = -1
        height = abs(g['rect'][3] - g['rect'][1])
        ignore = g['occlusion'] > MAX_OCCLUSION[d] or g['truncation'] > MAX_TRUNCATION[d] or height < MIN_HEIGHT[d]
        if valid == 1 and not ignore:
            gflag.append(0)
            n_gt += 1
        elif valid == 0 or (valid == 1 and ignore):
            gflag.append(1)
        else:
            gflag.append(-1)
        if t == 'dontcare':
            dontcare.append(i)
    dflag = []
    for e in dets:
        if e['type'].lower() != cls:
            dflag.append(-1)
        elif abs(e['rect'][3] - e['rect'][1]) < MIN_HEIGHT[d]:
            dflag.append(1)
        else:
            dflag.append(0)
    return gflag, dflag, dontcare, n_gt


def match_frame(ov, gflag, dflag, scores, min_overlap, thresh=None, dc_ov=None, alpha_g=None, alpha_d=None):
    """One frame, one (class, difficulty).  thresh None: scores mode (compute_fp = false) -> the list of (g, score) of the
    true positives.  Otherwise counts mode -> (tp, fp, fn, similarity).  dc_ov[detection][region]: the share of the
    detection's rectangle inside each DontCare region (bbox metric only)."""
    compute_fp = thresh is not None
    n_g, n_d = len(gflag), len(dflag)
    assigned = [False] * n_d
    below = [compute_fp and scores[j] < thresh for j in range(n_d)]
    tp = fp = fn = 0
    similarity = 0.0
    tp_scores = []
    for i in range(n_g):
        if gflag[i] == -1:
            continue
        det_idx = -1
        valid_detection = NO_DETECTION
        max_overlap = 0.0
        assigned_ignored_det = False
        for j in range(n_d):
            if dflag[j] == -1 or assigned[j] or below[j]:
                continue
            overlap = ov[j][i]
            if not compute_fp and overlap > min_overlap and (valid_detection is NO_DETECTION or scores[j] > valid_detection):
                det_idx = j
                valid_detection = scores[j]
            elif compute_fp and overlap > min_overlap and (overlap > max_overlap or assigned_ignored_det) and dflag[j] == 0:
                max_overlap = overlap
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = False
            elif compute_fp and overlap > min_overlap and valid_detection is NO_DETECTION and dflag[j] == 1:
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = True
        if valid_detection is NO_DETECTION and gflag[i] == 0:
            fn += 1
        elif valid_detection is not NO_DETECTION and (gflag[i] == 1 or dflag[det_idx] == 1):
            assigned[det_idx] = True
        elif valid_detection is not NO_DETECTION:
            tp += 1
            tp_scores.append((i, scores[det_idx]))
            if compute_fp and alpha_g is not None:
                similarity += (1.0 + math.cos(alpha_g[i] - alpha_d[det_idx])) / 2.0
            assigned[det_idx] = True
    if not compute_fp:
        return tp_scores
    for j in range(n_d):
        if not (assigned[j] or dflag[j] == -1 or dflag[j] == 1 or below[j]):
            fp += 1
    nstuff = 0
    if dc_ov is not None:
        for r in range(len(dc_ov[0]) if n_d else 0):
            for j in range(n_d):
                if assigned[j] or dflag[j] == -1 or dflag[j] == 1 or below[j]:
                    continue
                if dc_ov[j][r] > min_overlap:
                    assigned[j] = True
                    nstuff += 1
    fp -= nstuff
    return tp, fp, fn, similarity


def thresholds(scores, n_gt, n_sample_pts=41):
    scores = sorted(scores, reverse=True)
    out = []
    if n_gt == 0:
        return out
    current_recall = 0.0
    for i, s in enumerate(scores):
        l_recall = (i + 1) / n_gt
        r_recall = (i + 2) / n_gt if i < len(scores) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(scores) - 1:
            continue
        out.append(s)
        current_recall += 1 / (n_sample_pts - 1.0)
    return out


def average_precision(values):
    """(R11, R40) of a curve given at the thresholds: zero-padded to 41, running maximum from the right."""
    p = [0.0] * 41
    for k, v in enumerate(values):
        p[k] = v
    for k in range(41):
        p[k] = max(p[k:])
    r11 = sum(p[k] for k in range(0, 41, 4)) / 11 * 100
    r40 = sum(p[k] for k in range(1, 41)) / 40 * 100
    return r11, r40


def evaluate(gt_frames, det_frames, classes, min_overlap, overlaps, dontcare_ov):
    """overlaps[metric][frame]: matrix [n_d][n_g]; dontcare_ov[frame]: [n_d][n_dc] (intersection / detection area, regions in
    ground-truth order).  -> {(metric, class, difficulty): {'n_gt', 'thresholds', 'tp', 'fp', 'fn', 'similarity', 'ap_r11',
    'ap_r40', 'aos_r11', 'aos_r40'}}."""
    out = {}
    F = len(gt_frames)
    for cls in classes:
        for d in range(3):
            flags = [clean_frame(gt_frames[f], det_frames[f], cls, d) for f in range(F)]
            n_gt = sum(fl[3] for fl in flags)
            for metric in overlaps:
                mo = min_overlap[cls]
                scores = [[e['score'] for e in det_frames[f]] for f in range(F)]
                tps = []
                for f in range(F):
                    tps += [s for _, s in match_frame(overlaps[metric][f], flags[f][0], flags[f][1], scores[f], mo)]
                thr = thresholds(tps, n_gt)
                rec = {'n_gt': n_gt, 'thresholds': thr, 'tp': [], 'fp': [], 'fn': [], 'similarity': []}
                for t in thr:
                    tp = fp = fn = 0
                    sim = 0.0
                    for f in range(F):
                        bbox = metric == 'bbox'
                        r = match_frame(overlaps[metric][f], flags[f][0], flags[f][1], scores[f], mo, thresh=t,
                                        dc_ov=dontcare_ov[f] if bbox else None,
                                        alpha_g=[g['alpha'] for g in gt_frames[f]] if bbox else None,
                                        alpha_d=[e['alpha'] for e in det_frames[f]] if bbox else None)
                        tp, fp, fn, sim = tp + r[0], fp + r[1], fn + r[2], sim + r[3]
                    rec['tp'].append(tp); rec['fp'].append(fp); rec['fn'].append(fn); rec['similarity'].append(sim)
                prec = [tp / (tp + fp) if tp + fp > 0 else 0.0 for tp, fp in zip(rec['tp'], rec['fp'])]
                aos = [s / (tp + fp) if tp + fp > 0 else 0.0 for s, tp, fp in zip(rec['similarity'], rec['tp'], rec['fp'])]
                rec['ap_r11'], rec['ap_r40'] = average_precision(prec)
                rec['aos_r11'], rec['aos_r40'] = average_precision(aos)
                out[(metric, cls, d)] = rec
    return out


def rect_overlaps_numpy(a, b, na, nb, criterion):
    """The rectangle rule of include/rtm3d_hip.h as one numpy expression in the device's operation order: a (B, cap_a, 4),
    b (B, cap_b, 4) -> (B, cap_a, cap_b); what the device result must EQUAL bit for bit."""
    a, b = a[:, :, None, :], b[:, None, :, :]
    with np.errstate(all='ignore'):
        w = np.fmin(a[..., 2], b[..., 2]) - np.fmax(a[..., 0], b[..., 0])
        h = np.fmin(a[..., 3], b[..., 3]) - np.fmax(a[..., 1], b[..., 1])
        inter = w * h
        sa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + np.zeros_like(inter)
        sb = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) + np.zeros_like(inter)
        den = ((sa + sb) - inter, sa, sb)[criterion]
        ok = np.isfinite(a).all(-1) & np.isfinite(b).all(-1) & ~((w <= 0) | (h <= 0)) & (den != 0) & np.isfinite(den)
        q = inter / np.where(ok, den, 1.0)
        out = np.where(ok & np.isfinite(q), q, 0.0)
    live = (np.arange(a.shape[1])[None, :, None] < na[:, None, None]) & (np.arange(b.shape[2])[None, None, :] < nb[:, None, None])
    return np.where(live, out, 0.0)
