"""Tracking evaluation - HOTA and CLEAR-MOT over 3D IoU, BEV IoU or the IoU of the image rectangles - with the assignments, the
global alignment and the frame walk on the device (csrc/mot_eval.hip).

    python -m rtm3d_amd.mot_eval GT_DIR RESULT_DIR [--metric iou3d|bev|bbox] [--classes Car Pedestrian] [--json FILE]

The protocol is RESTATED from the published behaviour of the HOTA / CLEAR evaluation (TrackEval) and of the KITTI tracking
benchmark's preprocessing; those programs were not available to compare against: parity with them is UNPINNED.  The contract is
the set of rules in include/rtm3d_hip.h ("tracking evaluation"); tests/mot_eval_ref.py restates them as plain loops.

Host side (runs anywhere): ``read_tracking_dir``, ``Tracks``, ``dense_ids``, ``slot_tables``, ``preprocess_keep``,
``hota_metrics``, ``clear_metrics``.  Device side (no CPU fallback - RuntimeError without the library or a GPU): ``similarity``,
``assign``, ``run_device``, ``evaluate``, ``Evaluator.result``.
"""
import json
import os

import numpy as np

from . import kitti_eval
from .kitti_eval import Labels

METRICS = ('iou3d', 'bev', 'bbox')
CLASSES = ('Car', 'Pedestrian')
DISTRACTOR = {'car': 'van', 'pedestrian': 'person_sitting'}
N_ALPHA = 19
ALPHAS = np.array([0.05 + a * 0.05 for a in range(N_ALPHA)])
EPS = 2.220446049250313e-16
MAX_BOXES = 256                # ground truths / tracker boxes per frame (rtm3d_mot_*)
HOTA_FIELDS = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')
CLEAR_FIELDS = ('MOTA', 'MOTP', 'Recall', 'Precision', 'MT', 'PT', 'ML', 'Frag', 'IDSW', 'TP', 'FN', 'FP')


# ------------------------------------------------------------------------------------------------------------------- data
class Tracks:
    """Labelled boxes with identities over named sequences.  ``names``: the sequences in order; ``frames[s][f]`` = (ids (n,)
    int64, rows): rows is a list of n label rows (type, truncation, occlusion, alpha, x1, y1, x2, y2, h, w, l, X, Y, Z, ry,
    score), (X, Y, Z) the centre of the BOTTOM face as in a KITTI file.  An id may stand at most once in a frame (DontCare
    rows, which carry no identity, excepted): ``add`` raises ValueError otherwise."""

    def __init__(self):
        self.names, self.frames = [], []

    def sequence(self, name, n_frames=0):
        """The index of sequence ``name``, created if new, with at least ``n_frames`` frames."""
        if name not in self.names:
            self.names.append(name)
            self.frames.append([])
        s = self.names.index(name)
        while len(self.frames[s]) < n_frames:
            self.frames[s].append((np.zeros(0, np.int64), []))
        return s

    def add(self, name, frame, ids, rows):
        frame = int(frame)
        if frame < 0:
            raise ValueError('Tracks.add: negative frame index %d in sequence %r' % (frame, name))
        s = self.sequence(name, frame + 1)
        ids = np.asarray(ids, np.int64).reshape(-1)
        rows = [tuple(r) for r in rows]
        if len(ids) != len(rows):
            raise ValueError('Tracks.add: %d ids for %d rows' % (len(ids), len(rows)))
        old_ids, old_rows = self.frames[s][frame]
        ids, rows = np.concatenate([old_ids, ids]), old_rows + rows
        real = [int(i) for i, r in zip(ids, rows) if str(r[0]).lower() != 'dontcare']
        if len(set(real)) != len(real):
            dup = sorted(i for i in set(real) if real.count(i) > 1)
            raise ValueError('sequence %r frame %d: track id %s stands more than once' % (name, frame, dup))
        self.frames[s][frame] = (ids, rows)


def read_tracking_dir(path, results=False):
    """Read KITTI tracking label files, ``<path>/<sequence>.txt``, one per sequence, into ``Tracks``.  A line is ``frame track_id
    type truncated occluded alpha x1 y1 x2 y2 h w l X Y Z ry [score]``: 17 fields of a ground-truth file (score 0) or 18;
    results=True requires the score.  A sequence has the frames 0 .. its largest frame index.  A malformed line raises
    ValueError naming the file and the line, and so does a track id that stands twice in one frame."""
    out = Tracks()
    for fn in sorted(f for f in os.listdir(path) if f.endswith('.txt')):
        name, full = fn[:-4], os.path.join(path, fn)
        out.sequence(name)
        per = {}
        with open(full) as fh:
            for ln, line in enumerate(fh, 1):
                p = line.split()
                if not p:
                    continue
                try:
                    if len(p) not in ((18,) if results else (17, 18)):
                        raise ValueError('%d fields' % len(p))
                    frame, tid = int(p[0]), int(p[1])
                    vals = [float(v) for v in p[3:]]
                except ValueError as e:
                    raise ValueError('mot_eval: %s line %d is not a KITTI tracking %s line (%s): %r'
                                     % (full, ln, 'result' if results else 'label', e, line.rstrip('\n'))) from None
                per.setdefault(frame, ([], []))
                per[frame][0].append(tid)
                per[frame][1].append(tuple([p[2]] + vals + ([0.0] if len(p) == 17 else [])))
        for frame in sorted(per):
            try:
                out.add(name, frame, per[frame][0], per[frame][1])
            except ValueError as e:
                raise ValueError('mot_eval: %s: %s' % (full, e)) from None
    return out


def _flatten(tracks, names, n_frames):
    """(Labels over the concatenated frames, ids (F, cap) int64, -1 beyond the counts)."""
    frames, fids = [], []
    for name, n in zip(names, n_frames):
        have = tracks.frames[tracks.names.index(name)] if name in tracks.names else []
        for f in range(n):
            frames.append(have[f] if f < len(have) else (np.zeros(0, np.int64), []))
            fids.append((name, f))
    lab = kitti_eval._frames_to_labels(fids, [fr[1] for fr in frames])
    ids = np.full((len(frames), lab.cap), -1, np.int64)
    for i, fr in enumerate(frames):
        ids[i, :len(fr[0])] = fr[0]
    return lab, ids


def frames_of(gt, trk):
    """The frames of two ``Tracks`` side by side: (sequence names, seq_start (S + 1,) int32, ground-truth Labels and ids (F, cap)
    int64, tracker Labels and ids).  The sequences are the ground truth's; a sequence the tracker lacks is empty, one only the
    tracker has raises; a sequence has as many frames as the longer of the two."""
    extra = [n for n in trk.names if n not in gt.names]
    if extra:
        raise ValueError('mot_eval: the tracker has sequences the ground truth lacks: %s' % extra)
    names = list(gt.names)
    n_frames = [max(len(gt.frames[i]), len(trk.frames[trk.names.index(n)]) if n in trk.names else 0) for i, n in enumerate(names)]
    seq_start = np.concatenate([[0], np.cumsum(n_frames)]).astype(np.int32)
    return (names, seq_start) + _flatten(gt, names, n_frames) + _flatten(trk, names, n_frames)


def _compact(lab, ids, keep):
    """The entries ``keep`` (F, cap) bool of every frame moved to the front, order kept: (Labels, ids, idx (F, cap2))."""
    keep = keep & lab.valid()
    n = keep.sum(1).astype(np.int32)
    cap = max(int(n.max(initial=0)), 1)
    idx = np.argsort(~keep, axis=1, kind='stable')[:, :cap]
    live = np.arange(cap)[None, :] < n[:, None]
    out = Labels(lab.frame_ids, n, cap)
    for f in Labels.FIELDS:
        a = getattr(lab, f)
        g = np.take_along_axis(a, idx.reshape(idx.shape + (1,) * (a.ndim - 2)), 1)
        blank = np.zeros((), a.dtype) if a.dtype.kind != 'U' else ''
        setattr(out, f, np.where(live.reshape(live.shape + (1,) * (a.ndim - 2)), g, blank))
    return out, np.where(live, np.take_along_axis(ids, idx, 1), -1), idx


def dense_ids(ids, n, seq_start):
    """Ids made dense per sequence in order of first appearance (frame order, then slot order): (dense (F, cap) int32 with -1
    beyond ``n``, the number of ids of every sequence)."""
    ids = np.asarray(ids, np.int64)
    F, cap = ids.shape
    valid = np.arange(cap)[None, :] < np.asarray(n).reshape(F, 1)
    out = np.full((F, cap), -1, np.int32)
    counts = []
    for s in range(len(seq_start) - 1):
        lo, hi = int(seq_start[s]), int(seq_start[s + 1])
        v = valid[lo:hi]
        flat = ids[lo:hi][v]
        uniq, first, inv = np.unique(flat, return_index=True, return_inverse=True)
        rank = np.empty(len(uniq), np.int64)
        rank[np.argsort(first, kind='stable')] = np.arange(len(uniq))
        block = out[lo:hi]
        block[v] = rank[inv.reshape(-1)]
        counts.append(len(uniq))
    return out, counts


def slot_tables(dense, n, n_ids):
    """(F, n_ids) int32: the slot at which every dense id stands in the frame, -1 where it is absent.  Raises ValueError if an id
    stands twice in a frame."""
    F, cap = dense.shape
    table = np.full((F, max(int(n_ids), 1)), -1, np.int32)
    valid = np.arange(cap)[None, :] < np.asarray(n).reshape(F, 1)
    f, k = np.nonzero(valid)
    table[f, dense[f, k]] = k
    if int((table >= 0).sum()) != len(f):
        raise ValueError('mot_eval: an id stands more than once in a frame')
    return table


# ------------------------------------------------------------------------------------------------------------ closing formulas
def _div(a, b):
    return np.asarray(a, np.float64) / np.maximum(1.0, np.asarray(b, np.float64))


def hota_metrics(tp, fn, fp, loc, mc, gcount, tcount):
    """The HOTA family per alpha from the device's counts: tp / fn / fp (S, 19) int, loc (S, 19), mc (S, 19, n_gid, n_tid),
    gcount (S, n_gid), tcount (S, n_tid).  Sums over sequences in sequence order.  {name: (19,) float64}."""
    tp, fn, fp = (np.asarray(v, np.float64).reshape(-1, N_ALPHA) for v in (tp, fn, fp))
    mc = np.asarray(mc, np.float64)
    S = tp.shape[0]
    TP, FN, FP = tp.sum(0), fn.sum(0), fp.sum(0)
    ass = {k: np.zeros(N_ALPHA) for k in ('AssA', 'AssRe', 'AssPr')}
    for s in range(S):
        g, t = np.asarray(gcount[s], np.float64)[None, :, None], np.asarray(tcount[s], np.float64)[None, None, :]
        ass['AssA'] += (mc[s] * (mc[s] / np.maximum(1.0, (g + t) - mc[s]))).sum((1, 2))
        ass['AssRe'] += (mc[s] * (mc[s] / np.maximum(1.0, g))).sum((1, 2))
        ass['AssPr'] += (mc[s] * (mc[s] / np.maximum(1.0, t))).sum((1, 2))
    out = {'DetA': _div(TP, TP + FN + FP), 'DetRe': _div(TP, TP + FN), 'DetPr': _div(TP, TP + FP)}
    for k in ass:
        out[k] = _div(ass[k], TP)
    out['LocA'] = np.where(TP > 0, _div(np.asarray(loc, np.float64).reshape(-1, N_ALPHA).sum(0), TP), 1.0)
    out['HOTA'] = np.sqrt(out['DetA'] * out['AssA'])
    return out


def clear_metrics(counts, simsum, idcount, matched, frag):
    """The CLEAR family from the device's outputs: counts (S, 4) = TP, FN, FP, IDSW; simsum (S,); idcount / matched / frag
    (S, n_gid)."""
    c = np.asarray(counts, np.int64).reshape(-1, 4).sum(0)
    TP, FN, FP, IDSW = (int(v) for v in c)
    idcount, matched, frag = (np.asarray(v, np.int64) for v in (idcount, matched, frag))
    seen = idcount > 0
    ratio = matched[seen] / idcount[seen]
    MT = int((ratio > 0.8).sum())
    PT = int((ratio >= 0.2).sum()) - MT
    return {'MOTA': (TP - FP - IDSW) / max(1, TP + FN), 'MOTP': float(np.asarray(simsum, np.float64).sum()) / max(1, TP),
            'Recall': TP / max(1, TP + FN), 'Precision': TP / max(1, TP + FP), 'MT': MT, 'PT': PT, 'ML': int(seen.sum()) - MT - PT,
            'Frag': int((frag[frag > 0] - 1).sum()), 'IDSW': IDSW, 'TP': TP, 'FN': FN, 'FP': FP}


def preprocess_keep(cls, gt_type, gt_occlusion, gt_truncation, ng, match, nt, cap_t, dontcare_share):
    """The KITTI preprocessing decision of class ``cls`` from the match of its tracker boxes against the frame's ground truths
    (DontCare excluded): gt_type / gt_occlusion / gt_truncation (F, cap_g), match (F, cap_g) tracker slot or -1, dontcare_share
    (F, cap_t): the largest share of the tracker box's rectangle inside a DontCare rectangle.  Returns (keep_g (F, cap_g),
    keep_t (F, cap_t)) bool."""
    name = cls.lower()
    gtype = np.char.lower(gt_type)
    F, cap_g = gtype.shape
    live_g = np.arange(cap_g)[None, :] < np.asarray(ng).reshape(F, 1)
    live_t = np.arange(cap_t)[None, :] < np.asarray(nt).reshape(F, 1)
    own = live_g & (gtype == name)
    hard = (gt_occlusion > 2) | (gt_truncation > 0)
    removes = live_g & ((gtype == DISTRACTOR.get(name, '\0')) | (own & hard)) & (match >= 0)
    is_matched = np.zeros((F, cap_t), bool)
    removed = np.zeros((F, cap_t), bool)
    f, g = np.nonzero(live_g & (match >= 0))
    is_matched[f, match[f, g]] = True
    f, g = np.nonzero(removes)
    removed[f, match[f, g]] = True
    removed |= ~is_matched & (np.asarray(dontcare_share) > 0.5)
    return own & ~hard, live_t & ~removed


# ------------------------------------------------------------------------------------------------------------------- device
def _torch():
    import torch
    return torch


def _device(device):
    try:
        return kitti_eval._device(device)
    except RuntimeError:
        raise RuntimeError('rtm3d_amd.mot_eval: the evaluation runs on the GPU (device %r); there is no CPU path' % (device,)) from None


def _up(a, dev, dt=None):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)


def similarity(gt, trk, metric='iou3d', device='cuda'):
    """The per-frame similarity matrices of two ``Labels`` over the same frames: (F, cap_g, cap_t) float64 CUDA tensor,
    ground truth x tracker box.  'iou3d' / 'bev' = rtm3d_box_overlaps (KITTI bottom-centre boxes moved to the centre convention by
    ``kitti_eval.boxes7``), 'bbox' = rtm3d_rect_overlaps, all intersection over union."""
    if metric not in METRICS:
        raise ValueError('similarity: metric must be one of %s, got %r' % (list(METRICS), metric))
    dev = _device(device)
    from . import box_overlap
    if len(gt) != len(trk):
        raise ValueError('similarity: %d / %d frames' % (len(gt), len(trk)))
    ng, nt = _up(gt.n, dev), _up(trk.n, dev)
    if metric == 'bbox':
        return kitti_eval.rect_overlaps(_up(gt.rect, dev), _up(trk.rect, dev), ng, nt, 'iou')
    bev, vol = box_overlap.overlaps(_up(kitti_eval.boxes7(gt), dev), _up(kitti_eval.boxes7(trk), dev), ng, nt, criterion='iou')
    return vol if metric == 'iou3d' else bev


def _check_sim(what, sim, ng, nt):
    torch = _torch()
    if not isinstance(sim, torch.Tensor) or not sim.is_cuda:
        raise RuntimeError('rtm3d_amd.mot_eval.%s needs CUDA (ROCm) tensors; there is no CPU path' % what)
    if sim.dtype != torch.float64 or sim.dim() != 3 or not sim.is_contiguous():
        raise ValueError('%s: a contiguous float64 tensor (F, cap_g, cap_t), got %s %s' % (what, sim.dtype, tuple(sim.shape)))
    F, cap_g, cap_t = sim.shape
    ng, nt = np.asarray(ng, np.int32).reshape(-1), np.asarray(nt, np.int32).reshape(-1)
    if len(ng) != F or len(nt) != F or ng.min(initial=0) < 0 or nt.min(initial=0) < 0 or ng.max(initial=0) > cap_g or nt.max(initial=0) > cap_t:
        raise ValueError('%s: ng / nt must hold %d counts within 0..%d / 0..%d' % (what, F, cap_g, cap_t))
    return F, cap_g, cap_t, ng, nt


def assign(w, ng, nt):
    """ASSIGN of every frame (rtm3d_mot_assign, one launch): w (F, cap_g, cap_t) float64 CUDA scores, ng / nt (F,) host counts ->
    (F, cap_g) int32 CUDA tensor, the tracker slot of every ground truth or -1."""
    torch = _torch()
    from . import _lib
    F, cap_g, cap_t, ng, nt = _check_sim('assign', w, ng, nt)
    dev = w.device
    with torch.cuda.device(dev):
        match = torch.empty(F, cap_g, dtype=torch.int32, device=dev)
        d_ng, d_nt = _up(ng, dev), _up(nt, dev)
        _lib.check(_lib.load().rtm3d_mot_assign(kitti_eval._stream(dev), F, cap_g, cap_t, d_ng.data_ptr(), d_nt.data_ptr(), w.data_ptr(),
                                                match.data_ptr()), 'mot_assign')
    return match


def run_device(sim, ng, nt, gid, tid, seq_start, clear_thresh=0.5, hota=True, clear=True):
    """The device side of HOTA and CLEAR-MOT on prepared arrays (include/rtm3d_hip.h): sim (F, cap_g, cap_t) float64 CUDA tensor;
    ng, nt (F,), gid (F, cap_g), tid (F, cap_t) dense per sequence, seq_start (S + 1,) host integer arrays.  Returns the raw device
    outputs as numpy arrays: 'potential', 'gcount', 'tcount', 'match', 'tp', 'fn', 'fp', 'loc', 'mc' (HOTA) and 'clear_match',
    'counts', 'simsum', 'idcount', 'matched', 'frag' (CLEAR).  No synchronisation until the results are fetched."""
    torch = _torch()
    from . import _lib
    lib = _lib.load()
    F, cap_g, cap_t, ng, nt = _check_sim('run_device', sim, ng, nt)
    seq_start = np.asarray(seq_start, np.int32).reshape(-1)
    S = len(seq_start) - 1
    if S < 1 or seq_start[0] != 0 or seq_start[-1] != F or (np.diff(seq_start) < 0).any():
        raise ValueError('run_device: seq_start must rise from 0 to %d, got %s' % (F, seq_start.tolist()))
    gid, tid = np.asarray(gid, np.int32).reshape(F, cap_g), np.asarray(tid, np.int32).reshape(F, cap_t)
    vg, vt = np.arange(cap_g)[None, :] < ng[:, None], np.arange(cap_t)[None, :] < nt[:, None]
    if (gid[vg] < 0).any() or (tid[vt] < 0).any():
        raise ValueError('run_device: ids must be dense and not negative')
    n_gid, n_tid = max(int(gid[vg].max(initial=-1)) + 1, 1), max(int(tid[vt].max(initial=-1)) + 1, 1)
    gslot, tslot = slot_tables(gid, ng, n_gid), slot_tables(tid, nt, n_tid)
    dev = sim.device
    out = {}
    with torch.cuda.device(dev):
        need = int(lib.rtm3d_mot_workspace_bytes(S, F, cap_g, cap_t, n_gid, n_tid))
        if need == 0:
            raise ValueError('run_device: sizes out of range (S %d, F %d, cap_g %d, cap_t %d, %d / %d ids; at most %d boxes per frame)'
                             % (S, F, cap_g, cap_t, n_gid, n_tid, MAX_BOXES))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        stream = kitti_eval._stream(dev)
        d = {k: _up(v, dev) for k, v in dict(seq=seq_start, ng=ng, nt=nt, gid=gid, tid=tid, gslot=gslot, tslot=tslot).items()}

        def zeros(*shape, dt=torch.int32):
            return torch.zeros(*shape, dtype=dt, device=dev)
        if hota:
            t = dict(potential=zeros(S, n_gid, n_tid, dt=torch.float64), gcount=zeros(S, n_gid), tcount=zeros(S, n_tid), match=zeros(F, cap_g),
                     tp=zeros(S, N_ALPHA), fn=zeros(S, N_ALPHA), fp=zeros(S, N_ALPHA), loc=zeros(S, N_ALPHA, dt=torch.float64),
                     mc=zeros(S, N_ALPHA, n_gid, n_tid))
            _lib.check(lib.rtm3d_mot_hota(stream, S, F, cap_g, cap_t, n_gid, n_tid, d['seq'].data_ptr(), d['ng'].data_ptr(), d['nt'].data_ptr(),
                                          d['gid'].data_ptr(), d['tid'].data_ptr(), d['gslot'].data_ptr(), d['tslot'].data_ptr(), sim.data_ptr(),
                                          t['potential'].data_ptr(), t['gcount'].data_ptr(), t['tcount'].data_ptr(), t['match'].data_ptr(),
                                          t['tp'].data_ptr(), t['fn'].data_ptr(), t['fp'].data_ptr(), t['loc'].data_ptr(), t['mc'].data_ptr(),
                                          ws.data_ptr()), 'mot_hota')
            out.update(t)
        if clear:
            t = dict(clear_match=zeros(F, cap_g), counts=zeros(S, 4), simsum=zeros(S, dt=torch.float64), idcount=zeros(S, n_gid),
                     matched=zeros(S, n_gid), frag=zeros(S, n_gid))
            _lib.check(lib.rtm3d_mot_clear(stream, S, F, cap_g, cap_t, n_gid, n_tid, d['seq'].data_ptr(), d['ng'].data_ptr(), d['nt'].data_ptr(),
                                           d['gid'].data_ptr(), d['tid'].data_ptr(), sim.data_ptr(), float(clear_thresh), t['clear_match'].data_ptr(),
                                           t['counts'].data_ptr(), t['simsum'].data_ptr(), t['idcount'].data_ptr(), t['matched'].data_ptr(),
                                           t['frag'].data_ptr(), ws.data_ptr()), 'mot_clear')
            out.update(t)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return out


class Result:
    """What ``evaluate`` returns, per class over all sequences: ``hota[cls][name]`` (19,) per alpha and ``hota_mean[cls][name]``
    for name in HOTA_FIELDS; ``clear[cls][name]`` for name in CLEAR_FIELDS; ``counts[cls]`` = the raw per-alpha TP / FN / FP
    summed over sequences; ``n_gt[cls]`` / ``n_trk[cls]`` the boxes evaluated (after preprocessing)."""

    def __init__(self, classes, metric, clear_thresh, preprocess, names, n_frames):
        self.classes, self.metric, self.clear_thresh, self.preprocess = tuple(classes), metric, float(clear_thresh), bool(preprocess)
        self.sequences, self.n_frames = list(names), int(n_frames)
        self.hota, self.hota_mean, self.clear, self.counts, self.n_gt, self.n_trk = {}, {}, {}, {}, {}, {}

    def table(self):
        lines = ['%-12s' % ('%s' % self.metric) + ' '.join('%8s' % k for k in HOTA_FIELDS)]
        for c in self.classes:
            lines.append('%-12s' % c + ' '.join('%8.4f' % self.hota_mean[c][k] for k in HOTA_FIELDS))
        lines.append('%-12s' % ('thr %.2f' % self.clear_thresh) + ' '.join('%9s' % k for k in CLEAR_FIELDS))
        for c in self.classes:
            lines.append('%-12s' % c + ' '.join(('%9d' if isinstance(self.clear[c][k], int) else '%9.4f') % self.clear[c][k] for k in CLEAR_FIELDS))
        return '\n'.join(lines)

    def to_json(self):
        return {'classes': list(self.classes), 'metric': self.metric, 'clear_thresh': self.clear_thresh, 'preprocess': self.preprocess,
                'sequences': self.sequences, 'n_frames': self.n_frames, 'alphas': [float(a) for a in ALPHAS],
                'n_gt': {c: int(self.n_gt[c]) for c in self.classes}, 'n_trk': {c: int(self.n_trk[c]) for c in self.classes},
                'hota': {c: {k: [float(v) for v in self.hota[c][k]] for k in HOTA_FIELDS} for c in self.classes},
                'hota_mean': {c: {k: float(self.hota_mean[c][k]) for k in HOTA_FIELDS} for c in self.classes},
                'clear': {c: {k: (int(v) if isinstance(v, int) else float(v)) for k, v in self.clear[c].items()} for c in self.classes},
                'counts': {c: {k: [int(v) for v in self.counts[c][k]] for k in ('tp', 'fn', 'fp')} for c in self.classes}}


def prepare(gt, trk, cls, metric='iou3d', preprocess=True, device='cuda'):
    """The arrays ``run_device`` takes for one class: {'sim' CUDA tensor, 'ng', 'nt', 'gid', 'tid', 'seq_start', 'names'}.  gt, trk:
    ``Tracks`` (laid side by side by ``frames_of``)."""
    torch = _torch()
    dev = _device(device)
    names, seq_start, g_all, g_ids, t_all, t_ids = frames_of(gt, trk)
    name = cls.lower()
    gtype = np.char.lower(g_all.type)
    tl, tids, _ = _compact(t_all, t_ids, np.char.lower(t_all.type) == name)
    if preprocess:
        gl, gids, _ = _compact(g_all, g_ids, gtype != 'dontcare')
    else:
        gl, gids, _ = _compact(g_all, g_ids, gtype == name)
    if max(gl.cap, tl.cap) > MAX_BOXES:
        raise ValueError('mot_eval: %d ground truths / %d tracker boxes in one frame; the evaluation holds %d' % (gl.cap, tl.cap, MAX_BOXES))
    F = len(gl)
    with torch.cuda.device(dev):
        if F == 0:
            sim = torch.zeros(0, 1, 1, dtype=torch.float64, device=dev)
        else:
            sim = similarity(gl, tl, metric, dev)
        if preprocess and F:
            match = assign(torch.where(sim >= 0.5 - EPS, sim, torch.zeros_like(sim)).contiguous(), gl.n, tl.n).cpu().numpy()
            dc, ndc = kitti_eval.dontcare_rects(g_all)
            share = kitti_eval.rect_overlaps(_up(tl.rect, dev), _up(dc, dev), _up(tl.n, dev), _up(ndc, dev), 'a').amax(2).cpu().numpy()
            keep_g, keep_t = preprocess_keep(cls, gl.type, gl.occlusion, gl.truncation, gl.n, match, tl.n, tl.cap, share)
            gl, gids, gi = _compact(gl, gids, keep_g)
            tl, tids, ti = _compact(tl, tids, keep_t)
            f = torch.arange(F, device=dev)[:, None, None]
            sim = sim[f, _up(gi, dev)[:, :, None], _up(ti, dev)[:, None, :]].contiguous()
    gid, _ = dense_ids(gids, gl.n, seq_start)
    tid, _ = dense_ids(tids, tl.n, seq_start)
    return dict(sim=sim, ng=gl.n, nt=tl.n, gid=gid, tid=tid, seq_start=seq_start, names=names)


def evaluate(gt, trk, classes=CLASSES, metric='iou3d', clear_thresh=0.5, preprocess=True, device='cuda'):
    """HOTA and CLEAR-MOT of the tracker output ``trk`` against the ground truth ``gt`` (two ``Tracks``: ``read_tracking_dir``,
    ``Evaluator``), per class, combined over the sequences.  metric: the similarity, 'iou3d' | 'bev' | 'bbox'.  clear_thresh: the
    CLEAR match threshold.  preprocess: the KITTI rule (distractor classes, occluded / truncated ground truths, DontCare regions).
    Returns a ``Result``.  Raises RuntimeError without a GPU or the library: there is no CPU path."""
    if metric not in METRICS:
        raise ValueError('evaluate: metric must be one of %s, got %r' % (list(METRICS), metric))
    if not np.isfinite(clear_thresh):
        raise ValueError('evaluate: clear_thresh must be finite, got %r' % (clear_thresh,))
    dev = _device(device)
    res = None
    for c in classes:
        p = prepare(gt, trk, c, metric, preprocess, dev)
        if res is None:
            res = Result(classes, metric, clear_thresh, preprocess, p['names'], len(p['ng']))
        res.n_gt[c], res.n_trk[c] = int(p['ng'].sum()), int(p['nt'].sum())
        if len(p['ng']) == 0:
            z = np.zeros((1, N_ALPHA))
            o = dict(tp=z, fn=z, fp=z, loc=z, mc=np.zeros((1, N_ALPHA, 1, 1)), gcount=np.zeros((1, 1)), tcount=np.zeros((1, 1)),
                     counts=np.zeros((1, 4)), simsum=np.zeros(1), idcount=np.zeros((1, 1)), matched=np.zeros((1, 1)), frag=np.zeros((1, 1)))
        else:
            o = run_device(p['sim'], p['ng'], p['nt'], p['gid'], p['tid'], p['seq_start'], clear_thresh)
        res.hota[c] = hota_metrics(o['tp'], o['fn'], o['fp'], o['loc'], o['mc'], o['gcount'], o['tcount'])
        res.hota_mean[c] = {k: float(np.mean(v)) for k, v in res.hota[c].items()}
        res.clear[c] = clear_metrics(o['counts'], o['simsum'], o['idcount'], o['matched'], o['frag'])
        res.counts[c] = {k: np.asarray(o[k]).reshape(-1, N_ALPHA).sum(0).astype(np.int64) for k in ('tp', 'fn', 'fp')}
    if res is None:
        raise ValueError('evaluate: no class given')
    return res


class Evaluator:
    """Score a tracker while it runs:

        ev = Evaluator(read_tracking_dir(gt_dir))
        for frame, frames in enumerate(loader):
            rec, rows, ids = engine.detect_frames(frames, K, kitti=True, tracker=trk)
            ev.add_frame('0000', frame, ids[0], rows[0])
        print(ev.result().table())

    ``add_frame`` takes the (topk,) ids of ``Tracker.update`` and the (topk, 16) rows of ``records_to_camera`` of one stream and
    keeps what ``kitti_results.tracking_rows`` keeps (confirmed tracks; ``include_tentative`` for all)."""

    def __init__(self, gt, classes=CLASSES, metric='iou3d', clear_thresh=0.5, preprocess=True, device='cuda',
                 class_names=('Car', 'Pedestrian', 'Cyclist'), include_tentative=False):
        self.gt, self.classes, self.metric, self.clear_thresh, self.preprocess, self.device = gt, tuple(classes), metric, clear_thresh, preprocess, device
        self.class_names, self.include_tentative = tuple(class_names), include_tentative
        self.trk = Tracks()

    def add_frame(self, seq, frame, ids, rows):
        from . import kitti_results
        tr = kitti_results.tracking_rows(ids, rows, self.class_names, self.include_tentative)
        self.trk.add(seq, frame, [r[0] for r in tr], [r[1:] for r in tr])

    def result(self):
        return evaluate(self.gt, self.trk, self.classes, self.metric, self.clear_thresh, self.preprocess, self.device)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m rtm3d_amd.mot_eval', description='HOTA and CLEAR-MOT of a directory of KITTI tracking result '
                                 'files against a directory of tracking label files, one file per sequence.')
    ap.add_argument('gt_dir')
    ap.add_argument('result_dir')
    ap.add_argument('--metric', default='iou3d', choices=METRICS)
    ap.add_argument('--classes', nargs='+', default=list(CLASSES))
    ap.add_argument('--clear-thresh', type=float, default=0.5)
    ap.add_argument('--no-preprocess', action='store_true', help='skip the KITTI preprocessing (distractors, occlusion, DontCare)')
    ap.add_argument('--json', default=None, help='also write Result.to_json() to this file')
    ap.add_argument('--device', default='cuda')
    args = ap.parse_args(argv)
    res = evaluate(read_tracking_dir(args.gt_dir), read_tracking_dir(args.result_dir, results=True), classes=args.classes, metric=args.metric,
                   clear_thresh=args.clear_thresh, preprocess=not args.no_preprocess, device=args.device)
    print(res.table())
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res.to_json(), fh)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
