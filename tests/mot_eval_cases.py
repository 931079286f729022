"""Generated tracking scenes for the tracking-evaluation tests (seeded, nothing from outside): car-sized objects on a grid that move
slowly, as ground truth ``Tracks``, and a tracker output made from them - the same boxes with noise, missed detections, false
positives, identity swaps between neighbours, ids that change after a gap, late births.  ``arrays`` turns a pair of ``Tracks``
into the arrays the device takes, with the similarity computed on the CPU (tests/box_overlap_ref.py, tests/kitti_eval_ref.py), so
that seeds can be chosen without a GPU: ``case(name)`` reseeds until the yardstick's own margin is >= MARGIN."""
import numpy as np

from rtm3d_amd import kitti_eval, mot_eval
from tests import box_overlap_ref, kitti_eval_ref
from tests import mot_eval_ref as ref

MARGIN = 1e-6
_cache = {}


def label_row(cls, box, score=0.0, truncation=0.0, occlusion=0.0):
    """A label row from a centre box (h, w, l, X, Y, Z, ry): the rectangle is a pinhole view of the box's extent."""
    h, w, l, X, Y, Z, ry = [float(v) for v in box]
    half = 0.5 * max(w, l)
    x1, x2 = 600.0 + 700.0 * (X - half) / Z, 600.0 + 700.0 * (X + half) / Z
    y1, y2 = 180.0 + 700.0 * (Y - h / 2) / Z, 180.0 + 700.0 * (Y + h / 2) / Z
    return (cls, truncation, occlusion, 0.0, x1, y1, x2, y2, h, w, l, X, Y + h / 2, Z, ry, score)


def scene(seed, n_seq=3, n_frames=12, n_obj=8, window=None, p_miss=0.12, p_fp=0.08, p_swap=0.06, noise=0.12, classes=('Car',)):
    """(gt, trk): two ``mot_eval.Tracks`` with sequences '0000', '0001', ...  window: None = every object lives (almost) the whole
    sequence; an int = each object lives that many frames from a random start (many ids, long absences)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt, trk = mot_eval.Tracks(), mot_eval.Tracks()
    for s in range(n_seq):
        name = '%04d' % s
        gt.sequence(name, n_frames)
        trk.sequence(name, n_frames)
        objs = []
        for i in range(n_obj):
            start = 0 if window is None else int(rng.integers(0, max(n_frames - window, 1)))
            if window is None and rng.random() < 0.25:
                start = int(rng.integers(1, max(n_frames // 2, 2)))                        # a late birth
            stop = n_frames if window is None else start + window
            objs.append(dict(dims=rng.uniform(0.9, 1.1, 3) * np.array([1.6, 1.8, 4.0]),
                             pos=np.array([(i % 5) * 9.0 - 18.0, 1.0, (i // 5) * 9.0 + 12.0]) + rng.uniform(-0.5, 0.5, 3),
                             vel=rng.uniform(-0.3, 0.3, 3) * np.array([1.0, 0.0, 1.0]), ry=rng.uniform(-3.1, 3.1), start=start, stop=stop,
                             cls=classes[i % len(classes)], tid=100 + i, gap=0))
        next_tid = 100 + n_obj
        for f in range(n_frames):
            g_ids, g_rows, t_ids, t_rows = [], [], [], []
            live = [o for o in objs if o['start'] <= f < o['stop']]
            if len(live) >= 2 and rng.random() < p_swap * len(live):
                a, b = rng.choice(len(live), 2, replace=False)
                live[a]['tid'], live[b]['tid'] = live[b]['tid'], live[a]['tid']           # an identity swap that stays
            for i, o in enumerate(objs):
                if not (o['start'] <= f < o['stop']):
                    continue
                box = np.concatenate([o['dims'], o['pos'] + (f - o['start']) * o['vel'], [o['ry']]])
                g_ids.append(i)
                g_rows.append(label_row(o['cls'], box))
                if rng.random() < p_miss:
                    o['gap'] += 1
                    continue
                if o['gap'] >= 2 and rng.random() < 0.5:
                    o['tid'], next_tid = next_tid, next_tid + 1                            # found again under a new id
                o['gap'] = 0
                seen = box.copy()
                seen[:3] *= rng.uniform(0.96, 1.04, 3)
                seen[3:6] += rng.normal(0, noise, 3) * np.array([1.0, 0.2, 1.0])
                seen[6] += rng.normal(0, 0.03)
                t_ids.append(o['tid'])
                t_rows.append(label_row(o['cls'], seen, score=float(rng.uniform(0.5, 1.0))))
            for _ in range(int(rng.random() < p_fp * max(len(live), 1)) + int(rng.random() < 0.1)):
                box = np.concatenate([[1.6, 1.8, 4.0], [rng.uniform(-20, 20), 1.0, rng.uniform(40, 60)], [rng.uniform(-3, 3)]])
                t_ids.append(next_tid)
                next_tid += 1
                t_rows.append(label_row(classes[0], box, score=0.4))
            gt.add(name, f, g_ids, g_rows)
            trk.add(name, f, t_ids, t_rows)
    return gt, trk


def cpu_similarity(gl, tl, metric):
    """``mot_eval.similarity`` on the CPU: (F, cap_g, cap_t) float64."""
    if metric == 'bbox':
        return kitti_eval_ref.rect_overlaps_numpy(gl.rect, tl.rect, gl.n, tl.n, 0)
    bev, vol = box_overlap_ref.overlaps(kitti_eval.boxes7(gl), kitti_eval.boxes7(tl), gl.n, tl.n, 'iou')
    return vol if metric == 'iou3d' else bev


def arrays(gt, trk, cls, metric):
    """What ``mot_eval.prepare(..., preprocess=False)`` returns, with the similarity from the CPU as a numpy array."""
    names, seq_start, g_all, g_ids, t_all, t_ids = mot_eval.frames_of(gt, trk)
    gl, gids, _ = mot_eval._compact(g_all, g_ids, np.char.lower(g_all.type) == cls.lower())
    tl, tids, _ = mot_eval._compact(t_all, t_ids, np.char.lower(t_all.type) == cls.lower())
    gid, _ = mot_eval.dense_ids(gids, gl.n, seq_start)
    tid, _ = mot_eval.dense_ids(tids, tl.n, seq_start)
    return dict(sim=cpu_similarity(gl, tl, metric), ng=gl.n, nt=tl.n, gid=gid, tid=tid, seq_start=seq_start, names=names)


def yardstick(a, thr=0.5, with_margin=True):
    """(hota outputs, clear outputs, margin) of the yardstick on prepared arrays (sim: anything numpy can read)."""
    sim = np.asarray(a['sim'], np.float64)
    h = ref.hota(sim, a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], with_margin)
    c = ref.clear(sim, a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], thr, with_margin)
    margin = min(h['margin'], c['margin'], ref.sim_margin(sim, a['ng'], a['nt'], [0.5]))
    return h, c, margin


# name -> (first seed, scene arguments, metric)
CASES = {
    'three_seq_iou3d': (0, dict(n_seq=3, n_frames=12, n_obj=8), 'iou3d'),
    'three_seq_bev': (100, dict(n_seq=3, n_frames=12, n_obj=8), 'bev'),
    'three_seq_bbox': (200, dict(n_seq=3, n_frames=12, n_obj=8), 'bbox'),
    'many_ids_iou3d': (300, dict(n_seq=1, n_frames=30, n_obj=40, window=6, p_swap=0.02), 'iou3d'),
}


def case(name):
    """(gt, trk, metric, seed) of a generated case whose CPU-side margin is >= MARGIN, and which holds every event."""
    if name not in _cache:
        first, kw, metric = CASES[name]
        for seed in range(first, first + 100):
            gt, trk = scene(seed, **kw)
            h, c, margin = yardstick(arrays(gt, trk, 'Car', metric))
            eventful = c['counts'][:, 3].sum() > 0 and c['counts'][:, 1].sum() > 0 and c['counts'][:, 2].sum() > 0
            if margin >= MARGIN and eventful:
                _cache[name] = (gt, trk, metric, seed)
                break
        else:
            raise RuntimeError('no seed gives case %s a margin of %g' % (name, MARGIN))
    return _cache[name]
