"""Rotated-box overlaps and 3D non-maximum suppression of detection records on the device (csrc/box_overlap.hip).

A box is 7 values in the order of record fields [24:31]: h, w, l, X, Y, Z, ry - (X, Y, Z) the box CENTRE in camera
coordinates (y down), the footprint l x w in the x-z plane rotated by plain cos(ry) / sin(ry) (no snapping of small values,
unlike ``kitti_results.rotation_matrix``), the vertical extent [Y - h/2, Y + h/2].  Everything is fp64 on the device; the
conventions are stated in include/rtm3d_hip.h, "box overlaps".

``overlaps`` gives the pairwise BEV / 3D overlap matrices the KITTI evaluation is built on (``rtm3d_amd.kitti_eval``: difficulty
filtering, device-side matching and the AP integral).  ``nms3d_records`` removes duplicate 3D boxes from
the (B, topk, 32) records of ``distributed.pack_records`` in place: a suppressed slot's flag goes 2 -> 1.
Device tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _lib

CRITERIA = {'iou': 0, 'a': 1, 'b': 2}
METRICS = {'bev': 0, '3d': 1}
MAX_TOPK = 256


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_cuda(what, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError('rtm3d_amd.box_overlap.%s needs CUDA (ROCm) tensors; there is no CPU path' % what)


def _boxes(what, name, t):
    if t.dtype != torch.float64 or t.dim() not in (2, 3) or t.shape[-1] != 7:
        raise ValueError('%s: %s must be a float64 tensor (B, cap, 7) or (N, 7), got %s %s' % (what, name, t.dtype, tuple(t.shape)))
    return (t.unsqueeze(0) if t.dim() == 2 else t).contiguous()


def _counts(what, name, n, B, cap, dev):
    if n is None:
        return torch.full((B,), cap, dtype=torch.int32, device=dev)
    _need_cuda(what, n)
    n = n.to(torch.int32).reshape(-1).contiguous()
    if n.numel() != B:
        raise ValueError('%s: %s holds %d counts for %d images' % (what, name, n.numel(), B))
    return n


def overlaps(a, b, na=None, nb=None, criterion='iou'):
    """Pairwise overlaps of two box lists per image (rtm3d_box_overlaps, one launch, no synchronisation).
    a: (B, cap_a, 7) float64 CUDA boxes, b: (B, cap_b, 7); (N, 7) is B = 1.  na / nb: (B,) integer CUDA tensors, the valid
    entries per image (None: all of them); entries beyond them are 0.  criterion: 'iou' = intersection / union, 'a' /
    'b' = intersection / size of a / of b.  Returns (bev, vol): (B, cap_a, cap_b) float64 - footprint-area and volume
    overlaps; (cap_a, cap_b) when both inputs were (N, 7)."""
    if criterion not in CRITERIA:
        raise ValueError("overlaps: criterion must be one of %s, got %r" % (sorted(CRITERIA), criterion))
    _need_cuda('overlaps', a, b)
    squeeze = a.dim() == 2 and b.dim() == 2
    a, b = _boxes('overlaps', 'a', a), _boxes('overlaps', 'b', b)
    if a.shape[0] != b.shape[0] or a.device != b.device:
        raise ValueError('overlaps: a holds %d images on %s, b %d on %s' % (a.shape[0], a.device, b.shape[0], b.device))
    dev, B, cap_a, cap_b = a.device, a.shape[0], a.shape[1], b.shape[1]
    with torch.cuda.device(dev):
        na, nb = _counts('overlaps', 'na', na, B, cap_a, dev), _counts('overlaps', 'nb', nb, B, cap_b, dev)
        bev = torch.empty(B, cap_a, cap_b, dtype=torch.float64, device=dev)
        vol = torch.empty(B, cap_a, cap_b, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().rtm3d_box_overlaps(_stream(dev), B, cap_a, cap_b, na.data_ptr(), nb.data_ptr(), a.data_ptr(), b.data_ptr(),
                                                  CRITERIA[criterion], bev.data_ptr(), vol.data_ptr()), 'box_overlaps')
    return (bev[0], vol[0]) if squeeze else (bev, vol)


def nms3d_records(rec, iou_thresh, metric='bev', class_aware=False, kitti_rows=None):
    """Greedy 3D NMS IN PLACE on (..., topk, 32) fp32 CUDA records (rtm3d_records_nms3d) on the current stream: among the slots
    with flag 2, in slot (= score) order, a slot whose IoU with an earlier surviving slot is strictly greater than
    ``iou_thresh`` gets flag 1; nothing else of the record changes.  metric: 'bev' | '3d'.  class_aware: only boxes of the
    same class suppress each other.  kitti_rows: the (..., topk, 16) float64 rows of ``preprocess.records_to_camera`` /
    ``Engine.detect_frames``; the rows of suppressed slots are zeroed.  Returns rec."""
    if metric not in METRICS:
        raise ValueError("nms3d_records: metric must be one of %s, got %r" % (sorted(METRICS), metric))
    _need_cuda('nms3d_records', rec)
    if rec.dtype != torch.float32 or rec.dim() < 2 or rec.shape[-1] != 32 or not rec.is_contiguous():
        raise ValueError('nms3d_records: rec must be a contiguous fp32 tensor (..., topk, 32), got %s %s' % (rec.dtype, tuple(rec.shape)))
    topk = int(rec.shape[-2])
    B = rec.numel() // (topk * 32) if topk else 0
    rows = 0
    if kitti_rows is not None:
        _need_cuda('nms3d_records', kitti_rows)
        if kitti_rows.dtype != torch.float64 or tuple(kitti_rows.shape) != tuple(rec.shape[:-1]) + (16,) or not kitti_rows.is_contiguous() \
                or kitti_rows.device != rec.device:
            raise ValueError('nms3d_records: kitti_rows must be a contiguous float64 tensor %s on %s' % (tuple(rec.shape[:-1]) + (16,), rec.device))
        rows = kitti_rows.data_ptr()
    with torch.cuda.device(rec.device):
        _lib.check(_lib.load().rtm3d_records_nms3d(_stream(rec.device), B, topk, rec.data_ptr(), float(iou_thresh), METRICS[metric],
                                                   1 if class_aware else 0, rows), 'records_nms3d')
    return rec


def nms3d_options(nms3d):
    """The ``nms3d`` keyword of Detect3DPipeline / Engine.detect: None, a float threshold, or a dict of nms3d_records'
    keyword arguments (iou_thresh, metric, class_aware) -> None or the checked keyword dict."""
    if nms3d is None:
        return None
    opts = dict(nms3d) if isinstance(nms3d, dict) else {'iou_thresh': float(nms3d)}
    unknown = set(opts) - {'iou_thresh', 'metric', 'class_aware'}
    if unknown or 'iou_thresh' not in opts:
        raise ValueError("nms3d: a float threshold or a dict with 'iou_thresh' and optionally 'metric', 'class_aware'; got %r" % (nms3d,))
    if opts.get('metric', 'bev') not in METRICS:
        raise ValueError("nms3d: metric must be one of %s, got %r" % (sorted(METRICS), opts['metric']))
    opts['iou_thresh'] = float(opts['iou_thresh'])
    return opts
