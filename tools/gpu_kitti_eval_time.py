"""Times of the KITTI evaluation on one MI355X: a seeded synthetic split of 3769 frames with at most 32 ground truths and at
most 100 detections per frame, 3 classes x 3 difficulties x 3 metrics.
  * hipEvent times of the overlap launches and of the two matching launches on one chunk of 512 frames: median (min) of 10
    timed groups of 5 launches after a warm-up;
  * wall time of ``kitti_eval.evaluate`` over the whole split: median of 3 after one warm-up run;
  * wall time of the plain-loop restatement (tests/kitti_eval_ref.py) on the first 32 frames on the same host, fed the
    device's overlap matrices, SCALED LINEARLY to 3769 frames and labelled so.
Prints the table; with an argument, also writes it to that file (profiles/kitti_eval.txt holds its output)."""
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import kitti_eval as ke
from tests import kitti_eval_ref as ref

F, CAP_G, CAP_D, GROUPS, PER, SUBSET = 3769, 32, 100, 10, 5, 32
TYPES = np.array(['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare'])
DIMS = np.array([[1.5, 1.6, 3.9], [1.75, 0.6, 0.8], [1.7, 0.6, 1.8], [2.1, 1.9, 5.0], [1.25, 0.6, 0.8], [1.0, 1.0, 1.0]])
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def rects(hwl, xyz):
    """A stand-in for the projected rectangle: the box's height and its longer side seen from the front, f = 720."""
    z = xyz[..., 2]
    u, v = 620.0 + 720.0 * xyz[..., 0] / z, 180.0 + 720.0 * xyz[..., 1] / z
    hh, ww = 720.0 * hwl[..., 0] / z, 0.7 * 720.0 * np.maximum(hwl[..., 1], hwl[..., 2]) / z
    return np.stack([u - ww / 2, v - hh, u + ww / 2, v], -1)


def synthetic(rng):
    ng = rng.integers(4, CAP_G + 1, F)
    nd = np.minimum(ng + rng.integers(0, CAP_D - 3, F), CAP_D)
    gt, det = ke.Labels(list(range(F)), ng, CAP_G), ke.Labels(list(range(F)), nd, CAP_D)
    t = rng.choice(6, size=(F, CAP_G), p=[0.4, 0.2, 0.15, 0.08, 0.05, 0.12])
    gt.type[:] = TYPES[t]
    gt.hwl[:] = DIMS[t] * rng.uniform(0.9, 1.1, (F, CAP_G, 3))
    z = rng.uniform(6.0, 60.0, (F, CAP_G))
    gt.xyz[:] = np.stack([rng.uniform(-0.55, 0.55, (F, CAP_G)) * z, np.full((F, CAP_G), 1.65), z], -1)
    gt.ry[:] = rng.uniform(-np.pi, np.pi, (F, CAP_G))
    gt.alpha[:] = gt.ry - np.arctan2(gt.xyz[..., 0], gt.xyz[..., 2])
    gt.occlusion[:] = rng.choice(4, size=(F, CAP_G), p=[0.55, 0.2, 0.15, 0.1])
    gt.truncation[:] = rng.choice([0.0, 0.1, 0.2, 0.4, 0.6], size=(F, CAP_G))
    gt.rect[:] = rects(gt.hwl, gt.xyz)
    # detections: slot j < 32 is ground truth j perturbed (where there is one of the three classes), the others are random boxes
    src = np.arange(CAP_D) % CAP_G
    s = rng.random((F, CAP_D))
    from_gt = (np.arange(CAP_D)[None, :] < CAP_G) & (t[:, src] < 3) & (src[None, :] < ng[:, None]) & (rng.random((F, CAP_D)) < 0.7)
    dt = np.where(from_gt, t[:, src], rng.integers(0, 3, (F, CAP_D)))
    det.type[:] = TYPES[dt]
    zf = rng.uniform(6.0, 70.0, (F, CAP_D))
    free = np.stack([rng.uniform(-0.55, 0.55, (F, CAP_D)) * zf, np.full((F, CAP_D), 1.65), zf], -1)
    det.xyz[:] = np.where(from_gt[..., None], gt.xyz[:, src] + s[..., None] * rng.normal(0, 0.2, (F, CAP_D, 3)), free)
    det.hwl[:] = np.where(from_gt[..., None], gt.hwl[:, src], DIMS[dt]) * (1 + 0.05 * s[..., None] * rng.normal(0, 1, (F, CAP_D, 3)))
    det.ry[:] = np.where(from_gt, gt.ry[:, src] + 0.1 * s * rng.normal(0, 1, (F, CAP_D)), rng.uniform(-np.pi, np.pi, (F, CAP_D)))
    det.alpha[:] = det.ry - np.arctan2(det.xyz[..., 0], det.xyz[..., 2])
    det.rect[:] = rects(det.hwl, det.xyz)
    det.truncation[:], det.occlusion[:] = -1.0, -1.0
    det.score[:] = np.where(from_gt, np.clip(0.95 - 0.8 * s, 0.01, 0.99), rng.uniform(0.02, 0.6, (F, CAP_D)))
    return gt, det


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    out = []
    for _ in range(GROUPS):
        e0.record()
        for _ in range(PER):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / PER)
    return float(np.median(out)), float(np.min(out))


def objects(lab, f):
    return [{'type': str(lab.type[f, j]), 'truncation': lab.truncation[f, j], 'occlusion': lab.occlusion[f, j], 'alpha': lab.alpha[f, j],
             'rect': lab.rect[f, j].tolist(), 'hwl': lab.hwl[f, j].tolist(), 'xyz': lab.xyz[f, j].tolist(), 'ry': lab.ry[f, j],
             'score': lab.score[f, j]} for j in range(int(lab.n[f]))]


dev = torch.device('cuda', 0)
try:
    commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=os.path.dirname(os.path.abspath(__file__)),
                                     stderr=subprocess.DEVNULL).decode().strip()
except Exception:
    commit = 'unknown'
gt, det = synthetic(np.random.Generator(np.random.PCG64(1)))
log('KITTI evaluation on %s (tree on top of commit %s)' % (torch.cuda.get_device_name(0), commit))
log('synthetic split: %d frames, %d ground truths (<= %d per frame), %d detections (<= %d per frame), 3 classes x 3 difficulties x 3 metrics'
    % (F, int(gt.n.sum()), CAP_G, int(det.n.sum()), CAP_D))

# ---- the launches, on one chunk of evaluate's size
C = ke.CHUNK_FRAMES
g, d = gt.select(range(C)), det.select(range(C))
log('one chunk of %d frames, us per call: median (min) of %d groups of %d back-to-back calls, hipEvent (Python wrappers included)' % (C, GROUPS, PER))
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                  # noqa: E731
nd, ng, drect, grect, dbox, gbox = up(d.n), up(g.n), up(d.rect), up(g.rect), up(ke.boxes7(d)), up(ke.boxes7(g))
from rtm3d_amd import box_overlap                                                   # noqa: E402
t = timed(lambda: ke.rect_overlaps(drect, grect, nd, ng))
log('rect_overlaps  %d x %d x %d pairs: %9.1f (%.1f)' % (C, CAP_D, CAP_G, t[0], t[1]))
t = timed(lambda: box_overlap.overlaps(dbox, gbox, nd, ng))
log('box_overlaps   %d x %d x %d pairs (BEV and 3D): %9.1f (%.1f)' % (C, CAP_D, CAP_G, t[0], t[1]))
flags = [ke.clean(g, d, c, k) for c in ke.CLASSES for k in range(3)]
gflag, dflag = up(np.stack([f[0] for f in flags], 1)), up(np.stack([f[1] for f in flags], 1))
mo = torch.tensor([ke.MIN_OVERLAP[c] for c in ke.CLASSES for _ in range(3)], dtype=torch.float64, device=dev)
score, ov = up(d.score), ke.rect_overlaps(drect, grect, nd, ng)
t = timed(lambda: ke.match_scores(nd, ng, gflag, dflag, score, ov, mo))
log('kitti_match scores mode, %d items (one wave each): %9.1f (%.1f)' % (C * 9, t[0], t[1]))
ms = ke.match_scores(nd, ng, gflag, dflag, score, ov, mo).cpu().numpy()
thr = [ke.thresholds(ms[:, k][ms[:, k] != -np.inf], max(flags[k][3], 1)) for k in range(9)]
thr_a = np.zeros((9, ke.N_SAMPLE_PTS))
for k in range(9):
    thr_a[k, :len(thr[k])] = thr[k]
thr_t, nthr_t = up(thr_a), torch.tensor([len(v) for v in thr], dtype=torch.int32, device=dev)
alpha_g, alpha_d = up(g.alpha), up(d.alpha)
dc_hit = torch.zeros(C, 9, CAP_D, dtype=torch.uint8, device=dev)
counts = tuple(torch.zeros(9, ke.N_SAMPLE_PTS, dtype=torch.int32, device=dev) for _ in range(3))
t = timed(lambda: ke.match_counts(nd, ng, gflag, dflag, score, ov, mo, nthr_t, thr_t, dc_hit=dc_hit, alpha_g=alpha_g, alpha_d=alpha_d, counts=counts))
log('kitti_match counts mode, %d items x %d thresholds = %d waves, %d of them with a threshold: %9.1f (%.1f)'
    % (C * 9, ke.N_SAMPLE_PTS, C * 9 * ke.N_SAMPLE_PTS, C * int(nthr_t.sum()), t[0], t[1]))

# ---- the whole evaluation
ke.evaluate(gt, det, device=dev)
walls = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ke.evaluate(gt, det, device=dev)
    torch.cuda.synchronize()
    walls.append(time.perf_counter() - t0)
log('evaluate, %d frames, wall: median %.3f s (min %.3f, max %.3f) of 3 after one warm-up run' % (F, np.median(walls), min(walls), max(walls)))
log('  AP_R40 moderate: ' + ', '.join('%s %s %.2f' % (c, m, res.ap_r40[m][c][1]) for c in ke.CLASSES for m in ke.METRICS))

# ---- the restatement on a subset, same host, the device's matrices
gs, ds = gt.select(range(SUBSET)), det.select(range(SUBSET))
ovs = {k: v.cpu().numpy() for k, v in ke.overlap_matrices(gs, ds, dev).items()}
gfr, dfr = [objects(gs, f) for f in range(SUBSET)], [objects(ds, f) for f in range(SUBSET)]
mats = {m: [ovs[m][f, :len(dfr[f]), :len(gfr[f])].tolist() for f in range(SUBSET)] for m in ke.METRICS}
ndc = [sum(o['type'] == 'DontCare' for o in fr) for fr in gfr]
dcs = [ovs['dontcare'][f, :len(dfr[f]), :ndc[f]].tolist() for f in range(SUBSET)]
t0 = time.perf_counter()
want = ref.evaluate(gfr, dfr, ke.CLASSES, ke.MIN_OVERLAP, mats, dcs)
wall = time.perf_counter() - t0
sub = ke.evaluate(gs, ds, device=dev)
same = all(sub.counts[m][c][k]['tp'].tolist() == want[(m, c, k)]['tp'] and sub.counts[m][c][k]['fp'].tolist() == want[(m, c, k)]['fp']
           for m in ke.METRICS for c in ke.CLASSES for k in range(3))
log('plain-loop restatement (matching only, overlaps given), %d frames, wall %.2f s on this host = %.0f s SCALED LINEARLY to %d frames; '
    'counts equal to the device on the subset: %s' % (SUBSET, wall, wall * F / SUBSET, F, same))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
