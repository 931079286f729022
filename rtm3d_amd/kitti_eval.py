"""KITTI object-detection AP (bbox / BEV / 3D / AOS) with the matching on the device (csrc/kitti_eval.hip).

    python -m rtm3d_amd.kitti_eval GT_DIR DET_DIR [--classes Car Pedestrian Cyclist] [--json FILE]

The protocol is RESTATED from the published devkit's behaviour (a C++ program that is not part of this project and was not
available to compare against): parity with the external tool is UNPINNED.  The contract is the set of rules written in
include/rtm3d_hip.h ("KITTI evaluation") and in the docstrings below; tests/kitti_eval_ref.py restates them as plain loops.

Per class and difficulty (easy / moderate / hard) and per metric:
  * ``clean`` flags every ground truth and detection: 0 counted, 1 ignored, -1 other class;
  * overlaps, once per frame chunk: ``bbox`` = rtm3d_rect_overlaps (IoU of the image rectangles), ``bev`` / ``3d`` =
    ``box_overlap.overlaps`` (rotated boxes, centre Y = y_bottom - h / 2);
  * DontCare regions: in ``bbox`` a detection whose rectangle lies in a DontCare region by more than the class's minimum
    overlap (intersection / detection area) is no false positive.  In ``bev`` and ``3d`` a DontCare region has no 3D box and
    REMOVES NOTHING (the choice made here: the label files give DontCare regions no dimensions or location);
  * rtm3d_kitti_match in scores mode gives the scores of the true positives, ``thresholds`` picks at most 41 of them, the
    counts mode gives tp / fp / fn and the orientation similarity at every threshold;
  * ``ap_from_counts``: precision = tp / (tp + fp), AOS = similarity / (tp + fp) (bbox only), running maximum from the
    right, AP_R11 = 100 * mean(p[0::4]), AP_R40 = 100 * mean(p[1:41]).

Everything but the two kernels and ``box_overlap.overlaps`` is vectorised host / torch code.  There is no CPU fallback:
``evaluate`` raises RuntimeError without the library or a GPU; ``read_label_dir``, ``from_rows`` (on CPU rows), ``clean``,
``thresholds`` and ``ap_from_counts`` run anywhere.
"""
import ctypes
import json
import os

import numpy as np

METRICS = ('bbox', 'bev', '3d')
DIFFICULTIES = ('easy', 'moderate', 'hard')
CLASSES = ('Car', 'Pedestrian', 'Cyclist')
MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
NEIGHBOUR = {'car': 'van', 'pedestrian': 'person_sitting'}
MIN_OVERLAP = {'Car': 0.7, 'Pedestrian': 0.5, 'Cyclist': 0.5}      # the same in all three metrics
N_SAMPLE_PTS = 41
MAX_DET = 256                  # rtm3d_kitti_match: detections per frame
CHUNK_FRAMES = 512             # frames per launch group: bounds the overlap matrices (3 x chunk x cap_d x cap_g fp64)


class Labels:
    """Padded label arrays of F frames: ``n`` (F,) int32 entries per frame; ``type`` (F, cap) str; ``truncation``,
    ``occlusion``, ``alpha``, ``ry``, ``score`` (F, cap) float64; ``rect`` (F, cap, 4) x1 y1 x2 y2; ``hwl`` (F, cap, 3);
    ``xyz`` (F, cap, 3), the centre of the BOTTOM face.  Entries beyond ``n`` are zeros / empty strings."""
    FIELDS = ('type', 'truncation', 'occlusion', 'alpha', 'rect', 'hwl', 'xyz', 'ry', 'score')

    def __init__(self, frame_ids, n, cap):
        F = len(frame_ids)
        self.frame_ids = list(frame_ids)
        self.n = np.asarray(n, np.int32).reshape(F)
        self.type = np.full((F, cap), '', dtype='<U24')
        self.truncation, self.occlusion, self.alpha = np.zeros((F, cap)), np.zeros((F, cap)), np.zeros((F, cap))
        self.rect, self.hwl, self.xyz = np.zeros((F, cap, 4)), np.zeros((F, cap, 3)), np.zeros((F, cap, 3))
        self.ry, self.score = np.zeros((F, cap)), np.zeros((F, cap))

    @property
    def cap(self):
        return self.type.shape[1]

    def __len__(self):
        return len(self.frame_ids)

    def valid(self):
        return np.arange(self.cap)[None, :] < self.n[:, None]

    def select(self, idx):
        """The frames ``idx`` (a sequence of positions), in that order."""
        idx = np.asarray(idx, np.int64).reshape(-1)
        out = Labels([self.frame_ids[i] for i in idx], self.n[idx], self.cap)
        for f in self.FIELDS:
            setattr(out, f, getattr(self, f)[idx])
        return out

    @staticmethod
    def concat(parts):
        cap = max([p.cap for p in parts] + [1])
        out = Labels([i for p in parts for i in p.frame_ids], np.concatenate([p.n for p in parts]) if parts else [], cap)
        at = 0
        for p in parts:
            for f in Labels.FIELDS:
                getattr(out, f)[at:at + len(p), :p.cap] = getattr(p, f)
            at += len(p)
        return out


def _frames_to_labels(frame_ids, frames):
    """frames: per frame a list of (type, trunc, occ, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score)."""
    lab = Labels(frame_ids, [len(f) for f in frames], max([len(f) for f in frames] + [1]))
    for i, rows in enumerate(frames):
        for j, r in enumerate(rows):
            lab.type[i, j] = r[0]
            lab.truncation[i, j], lab.occlusion[i, j], lab.alpha[i, j] = r[1], r[2], r[3]
            lab.rect[i, j], lab.hwl[i, j], lab.xyz[i, j] = r[4:8], r[8:11], r[11:14]
            lab.ry[i, j], lab.score[i, j] = r[14], r[15]
    return lab


def read_label_dir(path, frame_ids=None, results=False):
    """Read ``<path>/<frame id>.txt`` into ``Labels``.  A line is ``type truncated occluded alpha x1 y1 x2 y2 h w l x y z
    rotation_y [score]``: 16 fields as ``kitti_results.write_kitti_label_file`` writes them, or the 15 of a ground-truth
    file (score 0).  results=True: the score is required, and a missing file is an empty frame; a missing ground-truth
    file raises.  frame_ids None: every ``*.txt`` of the directory, sorted.  A malformed line raises ValueError naming the
    file and the line."""
    if frame_ids is None:
        frame_ids = sorted(f[:-4] for f in os.listdir(path) if f.endswith('.txt'))
    frames = []
    for fid in frame_ids:
        fn = os.path.join(path, '%s.txt' % fid)
        rows = []
        if not os.path.exists(fn):
            if not results:
                raise FileNotFoundError('kitti_eval: no ground-truth file %s' % fn)
            frames.append(rows)
            continue
        with open(fn) as fh:
            for ln, line in enumerate(fh, 1):
                p = line.split()
                if not p:
                    continue
                want = (16,) if results else (15, 16)
                try:
                    if len(p) not in want:
                        raise ValueError('%d fields' % len(p))
                    vals = [float(v) for v in p[1:]]
                except ValueError as e:
                    raise ValueError('kitti_eval: %s line %d is not a KITTI %s line (%s): %r'
                                     % (fn, ln, 'result' if results else 'label', e, line.rstrip('\n'))) from None
                rows.append([p[0]] + vals + ([0.0] if len(p) == 15 else []))
        frames.append(rows)
    return _frames_to_labels(frame_ids, frames)


def from_rows(kitti_rows, frame_ids=None, class_names=CLASSES):
    """Detections from the (B, topk, 16) float64 rows of ``Engine.detect_frames`` / ``preprocess.records_to_camera`` (layout:
    include/rtm3d_hip.h, rtm3d_records_to_camera).  A row is a detection if and only if row[14] == 2; the kept rows of a
    frame keep their slot (= score) order.  Truncation and occlusion are -1, as in a result file."""
    rows = kitti_rows.detach().cpu().numpy() if hasattr(kitti_rows, 'detach') else np.asarray(kitti_rows)
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 3 or rows.shape[-1] != 16:
        raise ValueError('from_rows: rows must be (B, topk, 16), got %s' % (tuple(rows.shape),))
    B = rows.shape[0]
    frame_ids = list(range(B)) if frame_ids is None else list(frame_ids)
    if len(frame_ids) != B:
        raise ValueError('from_rows: %d frame ids for %d frames' % (len(frame_ids), B))
    keep = rows[..., 14] == 2
    n = keep.sum(1)
    lab = Labels(frame_ids, n, max(int(n.max(initial=0)), 1))
    names = np.array(list(class_names) + ['DontCare'])
    for b in range(B):
        r = rows[b][keep[b]]
        k = len(r)
        c = r[:, 0].astype(np.int64)
        lab.type[b, :k] = names[np.where((c >= 0) & (c < len(class_names)) & (c == r[:, 0]), c, len(class_names))]
        lab.truncation[b, :k], lab.occlusion[b, :k] = -1.0, -1.0
        lab.alpha[b, :k], lab.rect[b, :k], lab.hwl[b, :k], lab.xyz[b, :k] = r[:, 1], r[:, 2:6], r[:, 6:9], r[:, 9:12]
        lab.ry[b, :k], lab.score[b, :k] = r[:, 12], r[:, 13]
    return lab


def _difficulty(d):
    return DIFFICULTIES.index(d) if isinstance(d, str) else int(d)


def clean(gt, det, cls, difficulty):
    """Flags of one (class, difficulty): (gflag (F, cap_g) int8, dflag (F, cap_d) int8, dontcare (F, cap_g) bool, n_gt).
    Type comparison ignores case.  Ground truth: class validity 1 if the type is ``cls``, 0 if it is the neighbouring class
    (Van for Car, Person_sitting for Pedestrian), else -1; ignore = occlusion > MAX_OCCLUSION or truncation > MAX_TRUNCATION
    or |y2 - y1| < MIN_HEIGHT; flag 0 if valid and not ignored (these count: n_gt), 1 if neighbouring or valid but ignored,
    -1 otherwise.  dontcare marks the DontCare ground truths.  Detection: -1 if the type differs from ``cls``, else 1 if
    |y2 - y1| < MIN_HEIGHT, else 0.  Entries beyond the counts are -1 / False."""
    d = _difficulty(difficulty)
    name = cls.lower()
    gtype = np.char.lower(gt.type)
    live = gt.valid()
    valid = np.where(gtype == name, 1, np.where(gtype == NEIGHBOUR.get(name, '\0'), 0, -1))
    height = np.abs(gt.rect[..., 3] - gt.rect[..., 1])
    ignore = (gt.occlusion > MAX_OCCLUSION[d]) | (gt.truncation > MAX_TRUNCATION[d]) | (height < MIN_HEIGHT[d])
    gflag = np.where((valid == 1) & ~ignore, 0, np.where((valid == 0) | ((valid == 1) & ignore), 1, -1))
    gflag = np.where(live, gflag, -1).astype(np.int8)
    dontcare = live & (gtype == 'dontcare')
    dheight = np.abs(det.rect[..., 3] - det.rect[..., 1])
    dflag = np.where(np.char.lower(det.type) == name, np.where(dheight < MIN_HEIGHT[d], 1, 0), -1)
    dflag = np.where(det.valid(), dflag, -1).astype(np.int8)
    return gflag, dflag, dontcare, int((gflag == 0).sum())


def thresholds(scores, n_gt):
    """The score thresholds of one (class, difficulty, metric) from the scores of the true positives of all frames and the
    number of counted ground truths: sort descending, cur = 0; for each i: l = (i + 1) / n_gt, r = (i + 2) / n_gt if
    i < len - 1 else l; skip i if (r - cur) < (cur - l) and i < len - 1; otherwise keep v[i] and add 1 / 40 to cur.  At most
    41 result; none for n_gt == 0 or no scores."""
    v = np.sort(np.asarray(scores, np.float64).reshape(-1))[::-1]
    out = []
    if n_gt <= 0:
        return np.zeros(0)
    cur = 0.0
    for i in range(len(v)):
        l = (i + 1) / n_gt
        r = (i + 2) / n_gt if i < len(v) - 1 else l
        if (r - cur) < (cur - l) and i < len(v) - 1:
            continue
        out.append(v[i])
        cur += 1.0 / (N_SAMPLE_PTS - 1.0)
    return np.asarray(out, np.float64)


def ap_from_counts(tp, fp, similarity=None):
    """(AP_R11, AP_R40) - and (AOS_R11, AOS_R40) with ``similarity`` - from the counts at the thresholds of one (class,
    difficulty, metric): p[k] = tp / (tp + fp), 0 where the denominator is 0, zero-padded to 41 entries, replaced by its
    running maximum from the right; R11 = 100 * mean(p[0::4]), R40 = 100 * mean(p[1:41])."""
    tp, fp = np.asarray(tp, np.float64).reshape(-1), np.asarray(fp, np.float64).reshape(-1)
    if len(tp) > N_SAMPLE_PTS or len(tp) != len(fp):
        raise ValueError('ap_from_counts: %d / %d counts (at most %d, equally many)' % (len(tp), len(fp), N_SAMPLE_PTS))
    den = tp + fp

    def integral(num):
        p = np.zeros(N_SAMPLE_PTS)
        p[:len(tp)] = np.where(den > 0, np.asarray(num, np.float64).reshape(-1) / np.where(den > 0, den, 1.0), 0.0)
        p = np.maximum.accumulate(p[::-1])[::-1]
        return 100.0 * float(np.mean(p[0::4])), 100.0 * float(np.mean(p[1:N_SAMPLE_PTS]))
    ap = integral(tp)
    return ap if similarity is None else ap + integral(similarity)


# ---------------------------------------------------------------------------------------------------------------- device
def _torch():
    import torch
    return torch


def _device(device):
    torch = _torch()
    dev = torch.device(device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError('rtm3d_amd.kitti_eval: the evaluation runs on the GPU (device %r); there is no CPU path' % (device,))
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def _stream(dev):
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def rect_overlaps(a, b, na=None, nb=None, criterion='iou'):
    """Pairwise overlaps of image rectangles (rtm3d_rect_overlaps, one launch): a (B, cap_a, 4), b (B, cap_b, 4) float64 CUDA
    tensors of x1 y1 x2 y2, na / nb (B,) integer CUDA counts (None: all) -> (B, cap_a, cap_b) float64.  criterion 'iou', 'a'
    (intersection / area of a) or 'b'."""
    torch = _torch()
    from . import _lib, box_overlap
    if criterion not in box_overlap.CRITERIA:
        raise ValueError('rect_overlaps: criterion must be one of %s, got %r' % (sorted(box_overlap.CRITERIA), criterion))
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError('rtm3d_amd.kitti_eval.rect_overlaps needs CUDA (ROCm) tensors; there is no CPU path')
        if t.dtype != torch.float64 or t.dim() != 3 or t.shape[-1] != 4:
            raise ValueError('rect_overlaps: float64 tensors (B, cap, 4), got %s %s' % (t.dtype, tuple(t.shape)))
    if a.shape[0] != b.shape[0] or a.device != b.device:
        raise ValueError('rect_overlaps: a holds %d frames on %s, b %d on %s' % (a.shape[0], a.device, b.shape[0], b.device))
    a, b = a.contiguous(), b.contiguous()
    dev, B, cap_a, cap_b = a.device, a.shape[0], a.shape[1], b.shape[1]
    with torch.cuda.device(dev):
        na = box_overlap._counts('rect_overlaps', 'na', na, B, cap_a, dev)
        nb = box_overlap._counts('rect_overlaps', 'nb', nb, B, cap_b, dev)
        out = torch.empty(B, cap_a, cap_b, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().rtm3d_rect_overlaps(_stream(dev), B, cap_a, cap_b, na.data_ptr(), nb.data_ptr(), a.data_ptr(), b.data_ptr(),
                                                   box_overlap.CRITERIA[criterion], out.data_ptr()), 'rect_overlaps')
    return out


def _ptr(t):
    return None if t is None else t.data_ptr()


def _match_args(what, nd, ng, gflag, dflag, score, dc_hit, alpha_g, alpha_d, overlap, min_overlap):
    torch = _torch()
    F, cap_d, cap_g = overlap.shape
    G = gflag.shape[1]
    want = {'nd': (nd, torch.int32, (F,)), 'ng': (ng, torch.int32, (F,)), 'gflag': (gflag, torch.int8, (F, G, cap_g)),
            'dflag': (dflag, torch.int8, (F, G, cap_d)), 'score': (score, torch.float64, (F, cap_d)),
            'dc_hit': (dc_hit, torch.uint8, (F, G, cap_d)), 'alpha_g': (alpha_g, torch.float64, (F, cap_g)),
            'alpha_d': (alpha_d, torch.float64, (F, cap_d)), 'overlap': (overlap, torch.float64, (F, cap_d, cap_g)),
            'min_overlap': (min_overlap, torch.float64, (G,))}
    for name, (t, dt, shape) in want.items():
        if t is None and name in ('dc_hit', 'alpha_g', 'alpha_d'):
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError('rtm3d_amd.kitti_eval.%s needs CUDA (ROCm) tensors; there is no CPU path' % what)
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != overlap.device:
            raise ValueError('%s: %s must be a contiguous %s tensor %s on %s, got %s %s' % (what, name, dt, shape, overlap.device, t.dtype, tuple(t.shape)))
    if bool((min_overlap < 0).any()) or bool(torch.isnan(min_overlap).any()):
        raise ValueError('%s: min_overlap must be >= 0' % what)
    return F, G, cap_d, cap_g


def match_scores(nd, ng, gflag, dflag, score, overlap, min_overlap):
    """rtm3d_kitti_match in scores mode on CUDA tensors (shapes: include/rtm3d_hip.h) -> (F, G, cap_g) float64: the score of
    the detection matched to each counted ground truth as a true positive, -inf elsewhere."""
    torch = _torch()
    from . import _lib
    F, G, cap_d, cap_g = _match_args('match_scores', nd, ng, gflag, dflag, score, None, None, None, overlap, min_overlap)
    dev = overlap.device
    with torch.cuda.device(dev):
        out = torch.empty(F, G, cap_g, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().rtm3d_kitti_match(_stream(dev), 0, F, G, cap_d, cap_g, nd.data_ptr(), ng.data_ptr(), gflag.data_ptr(),
                                                 dflag.data_ptr(), score.data_ptr(), None, None, None, overlap.data_ptr(),
                                                 min_overlap.data_ptr(), out.data_ptr(), 0, None, None, None, None, None, None), 'kitti_match')
    return out


def match_counts(nd, ng, gflag, dflag, score, overlap, min_overlap, nthr, thr, dc_hit=None, alpha_g=None, alpha_d=None, counts=None):
    """rtm3d_kitti_match in counts mode.  nthr (G,) int32, thr (G, max_thr) float64 CUDA tensors.  counts: None or the
    (tp, fp, fn) int32 (G, max_thr) tensors of an earlier chunk, which are added to.  Returns (tp, fp, fn, sim) with sim
    (F, G, max_thr) float64, the similarity of every (frame, group, threshold)."""
    torch = _torch()
    from . import _lib
    F, G, cap_d, cap_g = _match_args('match_counts', nd, ng, gflag, dflag, score, dc_hit, alpha_g, alpha_d, overlap, min_overlap)
    dev = overlap.device
    if thr.dtype != torch.float64 or thr.dim() != 2 or thr.shape[0] != G or thr.shape[1] < 1 or not thr.is_contiguous() or thr.device != dev:
        raise ValueError('match_counts: thr must be a contiguous float64 tensor (%d, max_thr >= 1) on %s' % (G, dev))
    T = thr.shape[1]
    if nthr.dtype != torch.int32 or tuple(nthr.shape) != (G,) or nthr.device != dev:
        raise ValueError('match_counts: nthr must be an int32 tensor (%d,) on %s' % (G, dev))
    with torch.cuda.device(dev):
        if counts is None:
            counts = tuple(torch.zeros(G, T, dtype=torch.int32, device=dev) for _ in range(3))
        for c in counts:
            if c.dtype != torch.int32 or tuple(c.shape) != (G, T) or not c.is_contiguous() or c.device != dev:
                raise ValueError('match_counts: counts must be three contiguous int32 tensors (%d, %d) on %s' % (G, T, dev))
        sim = torch.empty(F, G, T, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().rtm3d_kitti_match(_stream(dev), 1, F, G, cap_d, cap_g, nd.data_ptr(), ng.data_ptr(), gflag.data_ptr(),
                                                 dflag.data_ptr(), score.data_ptr(), _ptr(dc_hit), _ptr(alpha_g), _ptr(alpha_d),
                                                 overlap.data_ptr(), min_overlap.data_ptr(), None, T, nthr.data_ptr(), thr.data_ptr(),
                                                 counts[0].data_ptr(), counts[1].data_ptr(), counts[2].data_ptr(), sim.data_ptr()), 'kitti_match')
    return counts[0], counts[1], counts[2], sim


def boxes7(lab):
    """(F, cap, 7) boxes in ``box_overlap``'s convention from labels: h, w, l, X, Y = y_bottom - h / 2, Z, ry."""
    out = np.zeros(lab.type.shape + (7,))
    out[..., 0:3] = lab.hwl
    out[..., 3], out[..., 4], out[..., 5] = lab.xyz[..., 0], lab.xyz[..., 1] - lab.hwl[..., 0] / 2.0, lab.xyz[..., 2]
    out[..., 6] = lab.ry
    return out


def dontcare_rects(gt):
    """The DontCare rectangles of every frame, packed to the front: ((F, cap_dc, 4) float64, (F,) int32 counts)."""
    dc = gt.valid() & (np.char.lower(gt.type) == 'dontcare')
    n = dc.sum(1).astype(np.int32)
    out = np.zeros((len(gt), max(int(n.max(initial=0)), 1), 4))
    for f in np.nonzero(n)[0]:
        out[f, :n[f]] = gt.rect[f][dc[f]]
    return out, n


def overlap_matrices(gt, det, device='cuda'):
    """The device's overlap matrices of a set of frames: {'bbox', 'bev', '3d'} -> (F, cap_d, cap_g) float64 CUDA tensors
    (detection x ground truth, IoU) and 'dontcare' -> (F, cap_d, cap_dc): intersection / detection area with the frame's
    DontCare rectangles (``dontcare_rects``)."""
    torch = _torch()
    from . import box_overlap
    dev = _device(device)

    def up(a, dt=None):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    nd, ng = up(det.n), up(gt.n)
    drect = up(det.rect)
    out = {'bbox': rect_overlaps(drect, up(gt.rect), nd, ng, 'iou')}
    out['bev'], out['3d'] = box_overlap.overlaps(up(boxes7(det)), up(boxes7(gt)), nd, ng, criterion='iou')
    dc, ndc = dontcare_rects(gt)
    out['dontcare'] = rect_overlaps(drect, up(dc), nd, up(ndc), 'a')
    return out


class Result:
    """What ``evaluate`` returns.  ``ap_r40[metric][cls]`` / ``ap_r11`` = (easy, moderate, hard) with metric in ('bbox',
    'bev', '3d'); ``aos_r40[cls]`` / ``aos_r11[cls]`` likewise; ``n_gt[cls]`` = the counted ground truths per difficulty;
    ``thresholds[metric][cls][d]`` the score thresholds and ``counts[metric][cls][d]`` = {'tp', 'fp', 'fn', 'similarity'}
    at them (d = 0, 1, 2)."""

    def __init__(self, classes, min_overlap, n_frames):
        self.classes, self.min_overlap, self.n_frames = tuple(classes), dict(min_overlap), n_frames
        self.ap_r40 = {m: {} for m in METRICS}
        self.ap_r11 = {m: {} for m in METRICS}
        self.aos_r40, self.aos_r11, self.n_gt = {}, {}, {}
        self.thresholds = {m: {c: [None] * 3 for c in classes} for m in METRICS}
        self.counts = {m: {c: [None] * 3 for c in classes} for m in METRICS}

    def table(self):
        """Devkit-style lines: per class the AP_R40 and AP_R11 of bbox / bev / 3d / aos at easy, moderate, hard."""
        lines = []
        for c in self.classes:
            for tag, ap, aos in (('AP_R40', self.ap_r40, self.aos_r40), ('AP_R11', self.ap_r11, self.aos_r11)):
                lines.append('%s %s@%.2f, %.2f, %.2f:' % ((c, tag) + (self.min_overlap[c],) * 3))
                for m in METRICS:
                    lines.append('%-4s AP:%.4f, %.4f, %.4f' % ((m,) + tuple(ap[m][c])))
                lines.append('%-4s AP:%.4f, %.4f, %.4f' % (('aos',) + tuple(aos[c])))
        return '\n'.join(lines)

    def to_json(self):
        def lst(v):
            return [float(x) for x in v]
        return {
            'classes': list(self.classes), 'difficulties': list(DIFFICULTIES), 'metrics': list(METRICS), 'n_frames': self.n_frames,
            'min_overlap': {c: float(self.min_overlap[c]) for c in self.classes},
            'n_gt': {c: [int(v) for v in self.n_gt[c]] for c in self.classes},
            'ap_r40': {m: {c: lst(self.ap_r40[m][c]) for c in self.classes} for m in METRICS},
            'ap_r11': {m: {c: lst(self.ap_r11[m][c]) for c in self.classes} for m in METRICS},
            'aos_r40': {c: lst(self.aos_r40[c]) for c in self.classes}, 'aos_r11': {c: lst(self.aos_r11[c]) for c in self.classes},
            'thresholds': {m: {c: [lst(t) for t in self.thresholds[m][c]] for c in self.classes} for m in METRICS},
            'counts': {m: {c: [{'tp': [int(v) for v in k['tp']], 'fp': [int(v) for v in k['fp']], 'fn': [int(v) for v in k['fn']],
                                'similarity': lst(k['similarity'])} for k in self.counts[m][c]] for c in self.classes} for m in METRICS},
        }


def _min_overlaps(classes, min_overlap):
    mo = dict(MIN_OVERLAP)
    mo.update(min_overlap or {})
    for c in classes:
        if c not in mo:
            raise ValueError('kitti_eval: no min_overlap for class %r (known: %s); pass min_overlap={%r: ...}' % (c, sorted(mo), c))
        if not mo[c] >= 0:
            raise ValueError('kitti_eval: min_overlap of %r must be >= 0, got %r' % (c, mo[c]))
    return {c: float(mo[c]) for c in classes}


def evaluate(gt, det, classes=CLASSES, min_overlap=None, device='cuda', chunk_frames=CHUNK_FRAMES):
    """KITTI AP of the detections ``det`` against the ground truth ``gt`` (two ``Labels`` over the same frames in the same
    order: ``read_label_dir`` / ``from_rows``).  min_overlap: {class: value} overriding ``MIN_OVERLAP``.  Returns a
    ``Result``.  Two passes over chunks of ``chunk_frames`` frames, each computing the chunk's overlap matrices on the device:
    the first collects the true positives' scores (thresholds), the second the counts at the thresholds.  At most 256
    detections per frame.  Raises RuntimeError without a GPU or the library: there is no CPU path."""
    dev = _device(device)
    torch = _torch()
    if len(gt) != len(det) or list(gt.frame_ids) != list(det.frame_ids):
        raise ValueError('evaluate: ground truth and detections must cover the same frames in the same order (%d / %d frames)' % (len(gt), len(det)))
    if det.cap > MAX_DET:
        if int(det.n.max(initial=0)) > MAX_DET:
            raise ValueError('evaluate: %d detections in one frame; the matching holds %d' % (int(det.n.max()), MAX_DET))
        trimmed = Labels(det.frame_ids, det.n, max(int(det.n.max(initial=0)), 1))
        for f in Labels.FIELDS:
            setattr(trimmed, f, np.ascontiguousarray(getattr(det, f)[:, :trimmed.cap]))
        det = trimmed
    classes = tuple(classes)
    mo = _min_overlaps(classes, min_overlap)
    F, G, T = len(gt), len(classes) * 3, N_SAMPLE_PTS
    res = Result(classes, mo, F)
    flags = [clean(gt, det, c, d) for c in classes for d in range(3)]             # group = class * 3 + difficulty
    for ci, c in enumerate(classes):
        res.n_gt[c] = tuple(flags[ci * 3 + d][3] for d in range(3))
    if F == 0:
        gflag = dflag = None
    else:
        gflag = np.ascontiguousarray(np.stack([f[0] for f in flags], 1))         # (F, G, cap_g)
        dflag = np.ascontiguousarray(np.stack([f[1] for f in flags], 1))
    chunks = [(lo, min(lo + chunk_frames, F)) for lo in range(0, F, max(int(chunk_frames), 1))]

    def chunk_state(lo, hi):
        g, d = gt.select(range(lo, hi)), det.select(range(lo, hi))
        with torch.cuda.device(dev):
            ov = overlap_matrices(g, d, dev)
            st = {'nd': torch.from_numpy(d.n).to(dev), 'ng': torch.from_numpy(g.n).to(dev), 'ov': ov,
                  'gflag': torch.from_numpy(gflag[lo:hi]).to(dev), 'dflag': torch.from_numpy(dflag[lo:hi]).to(dev),
                  'score': torch.from_numpy(np.ascontiguousarray(d.score)).to(dev),
                  'alpha_g': torch.from_numpy(np.ascontiguousarray(g.alpha)).to(dev),
                  'alpha_d': torch.from_numpy(np.ascontiguousarray(d.alpha)).to(dev)}
            # (F, G, cap_d): the detection lies in a DontCare region by more than the min_overlap of the group's class
            st['dc_hit'] = (ov['dontcare'].amax(2)[:, None, :] > mo_t[None, :, None]).to(torch.uint8).contiguous()
        return st

    with torch.cuda.device(dev):
        mo_t = torch.tensor([mo[c] for c in classes for _ in range(3)], dtype=torch.float64, device=dev)
        tp_scores = {m: [[] for _ in range(G)] for m in METRICS}
        for lo, hi in chunks:
            st = chunk_state(lo, hi)
            for m in METRICS:
                ms = match_scores(st['nd'], st['ng'], st['gflag'], st['dflag'], st['score'], st['ov'][m], mo_t).cpu().numpy()
                for k in range(G):
                    v = ms[:, k, :]
                    tp_scores[m][k].append(v[v != -np.inf])
        thr = {m: [thresholds(np.concatenate(tp_scores[m][k]) if tp_scores[m][k] else [], flags[k][3]) for k in range(G)] for m in METRICS}
        thr_t, nthr_t, counts, sims = {}, {}, {m: None for m in METRICS}, {m: torch.zeros(G, T, dtype=torch.float64, device=dev) for m in METRICS}
        for m in METRICS:
            a = np.zeros((G, T))
            for k in range(G):
                a[k, :len(thr[m][k])] = thr[m][k]
            thr_t[m] = torch.from_numpy(a).to(dev)
            nthr_t[m] = torch.tensor([len(t) for t in thr[m]], dtype=torch.int32, device=dev)
        for lo, hi in chunks:
            st = chunk_state(lo, hi)
            for m in METRICS:
                bbox = m == 'bbox'
                tp, fp, fn, sim = match_counts(st['nd'], st['ng'], st['gflag'], st['dflag'], st['score'], st['ov'][m], mo_t, nthr_t[m], thr_t[m],
                                               dc_hit=st['dc_hit'] if bbox else None, alpha_g=st['alpha_g'] if bbox else None,
                                               alpha_d=st['alpha_d'] if bbox else None, counts=counts[m])
                counts[m] = (tp, fp, fn)
                sims[m] += sim.sum(0)
        host = {m: ([c.cpu().numpy() for c in counts[m]] if counts[m] is not None else [np.zeros((G, T), np.int32)] * 3) + [sims[m].cpu().numpy()]
                for m in METRICS}
    for m in METRICS:
        for ci, c in enumerate(classes):
            r40, r11, a40, a11 = [], [], [], []
            for d in range(3):
                k, n = ci * 3 + d, len(thr[m][ci * 3 + d])
                cnt = {'tp': host[m][0][k, :n].copy(), 'fp': host[m][1][k, :n].copy(), 'fn': host[m][2][k, :n].copy(),
                       'similarity': host[m][3][k, :n].copy()}
                res.thresholds[m][c][d], res.counts[m][c][d] = thr[m][k], cnt
                ap = ap_from_counts(cnt['tp'], cnt['fp'], cnt['similarity'])
                r11.append(ap[0]); r40.append(ap[1]); a11.append(ap[2]); a40.append(ap[3])
            res.ap_r40[m][c], res.ap_r11[m][c] = tuple(r40), tuple(r11)
            if m == 'bbox':
                res.aos_r40[c], res.aos_r11[c] = tuple(a40), tuple(a11)
    return res


class Evaluator:
    """Accumulate detections while detecting, evaluate at the end:

        ev = Evaluator(read_label_dir(gt_dir))
        for ids, frames in loader:
            rec, rows = engine.detect_frames(frames, K)
            ev.add_rows(ids, rows)
        print(ev.result().table())

    ``result`` evaluates the frames that were added (each once), in the ground truth's order."""

    def __init__(self, gt, classes=CLASSES, min_overlap=None, device='cuda', class_names=CLASSES):
        self.gt, self.classes, self.min_overlap, self.device, self.class_names = gt, tuple(classes), min_overlap, device, tuple(class_names)
        self._index = {fid: i for i, fid in enumerate(gt.frame_ids)}
        self._parts = {}

    def add_rows(self, frame_ids, kitti_rows):
        """The (B, topk, 16) rows of ``Engine.detect_frames`` / ``records_to_camera`` for the frames ``frame_ids`` of the ground truth."""
        lab = from_rows(kitti_rows, frame_ids, self.class_names)
        for i, fid in enumerate(lab.frame_ids):
            if fid not in self._index:
                raise KeyError('Evaluator.add_rows: frame %r is not in the ground truth' % (fid,))
            if fid in self._parts:
                raise ValueError('Evaluator.add_rows: frame %r was added before' % (fid,))
            self._parts[fid] = lab.select([i])

    def result(self):
        order = sorted(self._parts, key=self._index.get)
        det = Labels.concat([self._parts[f] for f in order]) if order else Labels([], [], 1)
        return evaluate(self.gt.select([self._index[f] for f in order]), det, self.classes, self.min_overlap, self.device)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m rtm3d_amd.kitti_eval', description='KITTI AP (bbox / BEV / 3D / AOS) of a directory of result '
                                 'files against a directory of label files; every label file is one frame, a missing result file an empty frame.')
    ap.add_argument('gt_dir')
    ap.add_argument('det_dir')
    ap.add_argument('--classes', nargs='+', default=list(CLASSES))
    ap.add_argument('--json', default=None, help='also write Result.to_json() to this file')
    ap.add_argument('--device', default='cuda')
    args = ap.parse_args(argv)
    gt = read_label_dir(args.gt_dir)
    det = read_label_dir(args.det_dir, gt.frame_ids, results=True)
    res = evaluate(gt, det, classes=args.classes, device=args.device)
    print(res.table())
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res.to_json(), fh)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
