"""Seeded inputs of the KITTI evaluation tests (tests/test_kitti_eval_cpu.py, tests/test_gpu_kitti_eval.py).  numpy only."""
import os

import numpy as np

MATCH_ND = (0, 1, 63, 64, 65, 200, 256)
MATCH_NG = (0, 1, 5, 33)
MATCH_FRAMES = 7
MATCH_MIN_OVERLAP = (0.7, 0.5, 0.5)                  # one per group
SCORE_SET = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)
# per group: thresholds equal to scores (the `score < t` boundary) and one between two scores
MATCH_THRESHOLDS = ((0.8, 0.6, 0.45, 0.3, 0.1), (0.7, 0.2), ())
DONTCARE_ONLY_FRAME = 3                             # every ground truth of this frame has flag -1 in every group


def match_case(n_d, n_g):
    """Random inputs of rtm3d_kitti_match: F = 7 frames, 3 groups, caps larger than the counts with garbage beyond them.
    Overlaps come from 6 values around the group-independent grid {0, 0.45, 0.5, 0.6, 0.7, 0.9} - which holds both minimum
    overlaps themselves - and scores from 8 values, so ties and both strict comparisons are hit all the time."""
    rng = np.random.Generator(np.random.PCG64(1000 * n_d + n_g))
    F, G = MATCH_FRAMES, len(MATCH_MIN_OVERLAP)
    cap_d = 256 if n_d > 250 else n_d + 5
    cap_g = n_g + 2
    nd = np.array([n_d if f % 2 == 0 else max(n_d - f, 0) for f in range(F)], np.int32)
    ng = np.array([n_g if f % 3 != 1 else max(n_g - 1, 0) for f in range(F)], np.int32)
    ov_set = np.array([0.0, 0.45, 0.5, 0.6, 0.7, 0.9])
    p = np.array([0.55, 0.1, 0.1, 0.1, 0.08, 0.07]) if n_d > 8 else np.array([0.1, 0.15, 0.2, 0.2, 0.2, 0.15])
    c = {'nd': nd, 'ng': ng, 'cap_d': cap_d, 'cap_g': cap_g,
         'overlap': ov_set[rng.choice(6, size=(F, cap_d, cap_g), p=p)],
         'score': np.array(SCORE_SET)[rng.integers(8, size=(F, cap_d))],
         'gflag': rng.choice(np.array([-1, 0, 0, 1], np.int8), size=(F, G, cap_g)),
         'dflag': rng.choice(np.array([-1, 0, 0, 0, 1, 1], np.int8), size=(F, G, cap_d)),
         'dc_hit': (rng.random((F, G, cap_d)) < 0.25).astype(np.uint8),
         'alpha_g': rng.uniform(-np.pi, np.pi, (F, cap_g)), 'alpha_d': rng.uniform(-np.pi, np.pi, (F, cap_d)),
         'min_overlap': np.array(MATCH_MIN_OVERLAP)}
    c['gflag'][DONTCARE_ONLY_FRAME] = -1
    for f in range(F):                                  # garbage beyond the counts: nothing of it may be read
        c['overlap'][f, nd[f]:] = np.nan
        c['overlap'][f, :, ng[f]:] = 0.99
        c['score'][f, nd[f]:] = 9.0
        c['gflag'][f, :, ng[f]:] = 0
        c['dflag'][f, :, nd[f]:] = 0
        c['dc_hit'][f, :, nd[f]:] = 0
        c['alpha_g'][f, ng[f]:] = np.nan
        c['alpha_d'][f, nd[f]:] = np.nan
    T = max(len(t) for t in MATCH_THRESHOLDS)
    c['thr'] = np.full((G, T), np.nan)
    for g, t in enumerate(MATCH_THRESHOLDS):
        c['thr'][g, :len(t)] = t
    c['nthr'] = np.array([len(t) for t in MATCH_THRESHOLDS], np.int32)
    return c


# ------------------------------------------------------------------------------------------------ the whole protocol
K = np.array([[720.0, 0.0, 620.0], [0.0, 720.0, 180.0], [0.0, 0.0, 1.0]])
IMAGE = (1242, 375)
DIMS = {'Car': (1.5, 1.6, 3.9), 'Van': (2.1, 1.9, 5.0), 'Pedestrian': (1.75, 0.6, 0.8), 'Person_sitting': (1.25, 0.6, 0.8),
        'Cyclist': (1.7, 0.6, 1.8)}
SPLIT_CLASSES = ('Car', 'Pedestrian', 'Cyclist')


def project_rect(hwl, xyz, ry):
    """Bounding rectangle of the projected corners of a box with bottom-face centre xyz, clipped to the image."""
    h, w, l = hwl
    c, s = np.cos(ry), np.sin(ry)
    pts = []
    for sx in (1, -1):
        for sy in (0, -1):
            for sz in (1, -1):
                lx, lz = sx * l / 2, sz * w / 2
                p = np.array([xyz[0] + c * lx + s * lz, xyz[1] + sy * h, xyz[2] - s * lx + c * lz])
                q = K @ p
                pts.append(q[:2] / q[2])
    pts = np.array(pts)
    x1, y1 = pts.min(0)
    x2, y2 = pts.max(0)
    return [float(np.clip(x1, 0, IMAGE[0] - 1)), float(np.clip(y1, 0, IMAGE[1] - 1)), float(np.clip(x2, 0, IMAGE[0] - 1)),
            float(np.clip(y2, 0, IMAGE[1] - 1))]


def _alpha(ry, xyz):
    a = ry - np.arctan2(xyz[0], xyz[2])
    return float((a + np.pi) % (2 * np.pi) - np.pi)


def _obj(t, trunc, occ, hwl, xyz, ry, score=0.0, rect=None):
    return {'type': t, 'truncation': float(trunc), 'occlusion': float(occ), 'alpha': _alpha(ry, xyz),
            'rect': [float(v) for v in (rect if rect is not None else project_rect(hwl, xyz, ry))], 'hwl': [float(v) for v in hwl],
            'xyz': [float(v) for v in xyz], 'ry': float(ry), 'score': float(score)}


def dontcare_obj(rect):
    return {'type': 'DontCare', 'truncation': -1.0, 'occlusion': -1.0, 'alpha': -10.0, 'rect': [float(v) for v in rect],
            'hwl': [-1.0] * 3, 'xyz': [-1000.0] * 3, 'ry': -10.0, 'score': 0.0}


def split(n_frames=24, seed=9):
    """(gt_frames, det_frames): ground truth with every occlusion and truncation level, Van, Person_sitting and DontCare
    regions; detections = ground truths perturbed in pose and size by an amount the score falls with, about 30 % of them
    dropped, and about two false positives per frame, some inside DontCare regions and some under 25 px high."""
    rng = np.random.Generator(np.random.PCG64(seed))
    types = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting']
    gt_frames, det_frames = [], []
    for f in range(n_frames):
        gts, dets = [], []
        for _ in range(int(rng.integers(9, 14))):
            t = types[int(rng.choice(5, p=[0.36, 0.27, 0.25, 0.07, 0.05]))]
            z = 6.0 + 44.0 * float(rng.random()) ** 1.4
            xyz = [float(rng.uniform(-0.55, 0.55)) * z, 1.65 + float(rng.normal(0, 0.05)), z]
            hwl = [v * float(rng.uniform(0.9, 1.1)) for v in DIMS[t]]
            ry = float(rng.uniform(-np.pi, np.pi))
            occ = int(rng.choice(4, p=[0.64, 0.16, 0.12, 0.08]))
            trunc = float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6], p=[0.6, 0.12, 0.12, 0.1, 0.06]))
            g = _obj(t, trunc, occ, hwl, xyz, ry)
            gts.append(g)
            if rng.random() < 0.3:
                continue
            s = float(rng.random())                                     # the size of the perturbation
            size = np.array([g['rect'][2] - g['rect'][0], g['rect'][3] - g['rect'][1]] * 2)
            rect = np.array(g['rect']) + s * rng.normal(0, 0.09, 4) * size
            dt = {'Van': 'Car', 'Person_sitting': 'Pedestrian'}[t] if t in ('Van', 'Person_sitting') and rng.random() < 0.7 else t
            rel = 0.35 if t in ('Pedestrian', 'Person_sitting') else 1.0    # small footprints tolerate smaller shifts
            dets.append(_obj(dt, -1, -1, [v * (1 + s * float(rng.normal(0, 0.05))) for v in hwl],
                             [xyz[0] + rel * s * float(rng.normal(0, 0.22)), xyz[1] + s * float(rng.normal(0, 0.08)),
                              xyz[2] + rel * s * float(rng.normal(0, 0.22))],
                             ry + s * float(rng.normal(0, 0.12)), score=float(np.clip(0.95 - 0.8 * s + rng.normal(0, 0.04), 0.01, 0.99)), rect=rect))
        regions = []
        for _ in range(int(rng.integers(1, 3))):
            x1, y1 = float(rng.uniform(0, 1000)), float(rng.uniform(100, 200))
            regions.append([x1, y1, x1 + float(rng.uniform(80, 220)), y1 + float(rng.uniform(60, 150))])
            gts.append(dontcare_obj(regions[-1]))
        for _ in range(int(rng.integers(1, 4))):                            # false positives
            t = SPLIT_CLASSES[int(rng.integers(3))]
            kind = rng.random()
            z = float(rng.uniform(62.0, 80.0)) if kind < 0.25 else float(rng.uniform(8.0, 40.0))      # far: under 25 px high
            xyz = [float(rng.uniform(-0.5, 0.5)) * z, 1.65, z]
            e = _obj(t, -1, -1, DIMS[t], xyz, float(rng.uniform(-np.pi, np.pi)), score=float(rng.uniform(0.05, 0.7)))
            if 0.25 <= kind < 0.55:                                       # inside a DontCare region
                r = regions[int(rng.integers(len(regions)))]
                hgt = float(rng.uniform(42, 58))
                e['rect'] = [r[0] + 5, r[1] + 1, r[0] + 5 + 0.6 * hgt, r[1] + 1 + hgt]
            dets.append(e)
        order = np.argsort([-e['score'] for e in dets], kind='stable')
        gt_frames.append(gts)
        det_frames.append([dets[i] for i in order])
    return gt_frames, det_frames


def perfect(gt_frames, turn=0.0):
    """Detections equal to the ground truths of the three classes, with distinct scores; ``turn`` is added to ry and alpha."""
    out, k = [], 0
    for gts in gt_frames:
        dets = []
        for g in gts:
            if g['type'] in SPLIT_CLASSES:
                k += 1
                e = dict(g, score=1.0 / (1.0 + k), truncation=-1.0, occlusion=-1.0)
                e['ry'], e['alpha'] = g['ry'] + turn, g['alpha'] + turn
                dets.append(e)
        out.append(dets)
    return out


def analytic_split(n_frames=12):
    """Ground truth for the checks that need no yardstick: per frame four objects of each class in one row 15 m ahead, 2.2 m
    apart, all unoccluded, untruncated and over 40 px high - 48 counted ground truths per class at every difficulty, which is
    what 41 thresholds need - and none overlapping another of its class."""
    rng = np.random.Generator(np.random.PCG64(5))
    frames = []
    for f in range(n_frames):
        gts = []
        for i in range(12):
            t = SPLIT_CLASSES[i % 3]
            gts.append(_obj(t, 0.0, 0, DIMS[t], [-12.0 + 2.2 * i + float(rng.uniform(-0.1, 0.1)), 1.65, 15.0 + float(rng.uniform(-0.5, 0.5))],
                            np.pi / 2 + float(rng.uniform(-0.2, 0.2))))
        gts.append(dontcare_obj([5.0, 300.0, 200.0, 370.0]))
        frames.append(gts)
    return frames


def frame_rows(frames):
    """Objects -> the row lists rtm3d_amd.kitti_eval._frames_to_labels takes."""
    return [[[o['type'], o['truncation'], o['occlusion'], o['alpha']] + list(o['rect']) + list(o['hwl']) + list(o['xyz']) + [o['ry'], o['score']]
             for o in fr] for fr in frames]


def write_dir(path, frames, results, skip_empty=False):
    """One label file per frame ('%06d.txt'), every number with 17 significant digits so that reading gives the same doubles.
    skip_empty: a frame without objects gets no file (a missing result file is an empty frame)."""
    os.makedirs(path, exist_ok=True)
    for f, fr in enumerate(frames):
        if skip_empty and not fr:
            continue
        with open(os.path.join(path, '%06d.txt' % f), 'w') as fh:
            for o in fr:
                vals = [o['truncation'], o['occlusion'], o['alpha']] + list(o['rect']) + list(o['hwl']) + list(o['xyz']) + [o['ry']]
                if results:
                    vals.append(o['score'])
                fh.write(o['type'] + ' ' + ' '.join('%.17g' % v for v in vals) + '\n')


def kitti_rows(det_frames, topk, class_names=SPLIT_CLASSES):
    """The (B, topk, 16) rows of rtm3d_records_to_camera that would carry these detections: kept rows (row[14] == 2)
    interleaved with zero rows."""
    rows = np.zeros((len(det_frames), topk, 16))
    for f, fr in enumerate(det_frames):
        assert 2 * len(fr) <= topk
        for j, o in enumerate(fr):
            rows[f, 2 * j] = [class_names.index(o['type']) if o['type'] in class_names else len(class_names), o['alpha']] + list(o['rect']) + list(o['hwl']) + list(o['xyz']) + [o['ry'], o['score'], 2.0, 0.0]
    return rows


def ref_overlaps(gt_frames, det_frames):
    """Overlap matrices for the yardstick WITHOUT the device (tests/box_overlap_ref.py and kitti_eval_ref.rect_overlap): what the
    CPU check of the split's APs uses.  -> ({'bbox' | 'bev' | '3d': [frame] matrices}, [frame] DontCare matrices)."""
    from tests import box_overlap_ref, kitti_eval_ref as ref
    ov = {'bbox': [], 'bev': [], '3d': []}
    dc = []
    for gts, dets in zip(gt_frames, det_frames):
        def box(o):
            return [o['hwl'][0], o['hwl'][1], o['hwl'][2], o['xyz'][0], o['xyz'][1] - o['hwl'][0] / 2, o['xyz'][2], o['ry']]
        ov['bbox'].append([[ref.rect_overlap(e['rect'], g['rect'], 0) for g in gts] for e in dets])
        bev = np.zeros((len(dets), len(gts)))
        vol = np.zeros((len(dets), len(gts)))
        for i, e in enumerate(dets):
            for j, g in enumerate(gts):
                if g['type'] != 'DontCare':
                    bev[i, j], vol[i, j] = box_overlap_ref.overlap(box(e), box(g), 'iou')
        ov['bev'].append(bev)
        ov['3d'].append(vol)
        dc.append([[ref.rect_overlap(e['rect'], g['rect'], 1) for g in gts if g['type'] == 'DontCare'] for e in dets])
    return ov, dc
