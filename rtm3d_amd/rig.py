"""Fusion of the kept 3D boxes of the C cameras of a rig into one set of boxes on the device (csrc/rig.hip; the rule:
include/rtm3d_hip.h, "rig fusion").

A ``Rig`` holds the cameras' extrinsics - the 3 x 4 [R | t] that takes a point of camera c's coordinates to the rig frame - for
R rigs (or R time steps of one rig) of C cameras.  ``fuse`` takes the (R * C, topk, 32) records of all cameras, image index
r * C + c, and returns per rig at most ``cap`` fused records in the rig frame, score-descending, the boxes two cameras report for
one object merged into one, with the map from every camera's record slot to its fused slot.  The rig frame is camera-like (x
right, y down, z forward), so the fused records go through box_overlap, track.Tracker and the bird's-eye panels like any
camera's.  ``camera_ids`` takes the ids a Tracker gives to the fused records back to each camera's slots.  Three launches per
``fuse``, one per ``camera_ids``, on the current stream and never a synchronisation; the records are not modified.  Device tensors
only: there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib

METRICS = {'bev': 0, 'iou3d': 1, 'dist': 2}
MERGES = {'best': 0, 'mean': 1}               # RTM3D_RIG_MERGE_BEST, RTM3D_RIG_MERGE_MEAN
MAX_CAMERAS, MAX_TOPK, MAX_SLOTS, MAX_CAP = 16, 256, 2048, 256
ORTHONORMAL_TOL = 1e-6

# rtm3d_rig_default_params'.  No multi-camera recording stands behind them: a choice, not a tuning.
_DEFAULTS = dict(metric='bev', thresh=0.1, class_aware=True, cross_only=True, merge='mean', min_score=0.0)


class RigParams(object):
    """The parameters of rtm3d_rig_fuse (struct rtm3d_rig_params).  metric: 'bev' | 'iou3d' (IoU of two boxes in the rig frame) |
    'dist' (minus the centre distance in metres); two boxes link only if the affinity is strictly greater than ``thresh``.
    class_aware: only boxes of one class link.  cross_only: two boxes of one camera never link to each other (they can still
    meet in one cluster through a representative of another camera).  merge: 'mean' (score-weighted mean of the cluster's boxes,
    headings folded onto the representative's end) | 'best' (the representative's box).  min_score: slots below it are ignored."""

    def __init__(self, **kw):
        unknown = set(kw) - set(_DEFAULTS)
        if unknown:
            raise ValueError('RigParams: unknown parameters %s (known: %s)' % (sorted(unknown), sorted(_DEFAULTS)))
        for k, v in _DEFAULTS.items():
            setattr(self, k, kw.get(k, v))
        if self.metric not in METRICS:
            raise ValueError('RigParams: metric must be one of %s, got %r' % (sorted(METRICS), self.metric))
        if self.merge not in MERGES:
            raise ValueError('RigParams: merge must be one of %s, got %r' % (sorted(MERGES), self.merge))

    def to_c(self):
        p = _lib.RigParamsC()
        p.metric, p.merge = METRICS[self.metric], MERGES[self.merge]
        p.class_aware, p.cross_only = 1 if self.class_aware else 0, 1 if self.cross_only else 0
        p.thresh, p.min_score = float(self.thresh), float(self.min_score)
        return p


def mount(yaw, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """One camera's (3, 4) float64 [R | t] from the way it is mounted.  The rig frame is x right, y down, z forward; angles in
    radians; R = R_yaw * R_pitch * R_roll (the roll is applied first, about the camera's own optical axis):
      yaw   about y (down): positive turns the camera to the RIGHT - its optical axis (0, 0, 1) becomes (sin yaw, 0, cos yaw) -
            and adds yaw to the ry of every box it sees;
      pitch about x (right): positive tilts the camera UP - the optical axis becomes (0, -sin pitch, cos pitch);
      roll  about z (forward): positive turns the camera clockwise seen from behind - its right (1, 0, 0) becomes (cos roll, sin
            roll, 0), towards down.
    t: the position of the camera's centre in the rig frame, metres."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rp = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    Rr = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    return np.concatenate([Ry @ Rp @ Rr, np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def check_extrinsics(extrinsics, R=1):
    """(R, C, 3, 4) float64 from (C, 3, 4), (C, 4, 4) or (R, C, ...); ValueError naming the camera for one that is not finite,
    whose rotation is not orthonormal within 1e-6 or is a reflection, or whose fourth row is not (0, 0, 0, 1)."""
    e = np.asarray(extrinsics, np.float64)
    if e.ndim == 3:
        e = np.broadcast_to(e, (int(R),) + e.shape)
    if e.ndim != 4 or e.shape[0] != int(R) or e.shape[2:] not in ((3, 4), (4, 4)):
        raise ValueError('Rig: extrinsics must have shape (C, 3, 4), (C, 4, 4) or (%d, C, ...), got %s' % (R, np.shape(extrinsics)))
    C = e.shape[1]
    if not 1 <= C <= MAX_CAMERAS:
        raise ValueError('Rig: %d cameras per rig (1..%d)' % (C, MAX_CAMERAS))
    for r in range(e.shape[0]):
        for c in range(C):
            m = e[r, c]
            where = 'camera %d' % c + (' of rig %d' % r if e.shape[0] > 1 else '')
            if not np.isfinite(m).all():
                raise ValueError('Rig: the extrinsics of %s are not finite' % where)
            if m.shape[0] == 4 and np.abs(m[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > ORTHONORMAL_TOL:
                raise ValueError('Rig: the fourth row of the extrinsics of %s is not (0, 0, 0, 1)' % where)
            rot = m[:3, :3]
            err = float(np.abs(rot.T @ rot - np.eye(3)).max())
            if err > ORTHONORMAL_TOL:
                raise ValueError('Rig: the rotation of %s is not orthonormal (R^T R differs from 1 by %.3g, bar %g)' % (where, err, ORTHONORMAL_TOL))
            if np.linalg.det(rot) < 0.0:
                raise ValueError('Rig: the rotation of %s is a reflection (determinant -1)' % where)
    return np.array(e[:, :, :3, :], dtype=np.float64, order='C')               # a copy: e may be a broadcast view


class Fused(object):
    """What Rig.fuse returns, all CUDA tensors: ``records`` (R, cap, 32) fp32 fused records in the rig frame, score-descending;
    ``box`` (R, cap, 7) float64 h w l X Y Z ry before the rounding to fp32; ``info`` (R, cap, 4) int32 representative's camera,
    its record slot, member count, bit mask of the cluster's cameras; ``map`` (R * C, topk) int32 per record slot: -1 no
    candidate, s >= 0 its fused slot, -2 its cluster did not fit; ``n`` (R, 2) int32 clusters written, clusters dropped."""

    def __init__(self, records, box, info, map, n):
        self.records, self.box, self.info, self.map, self.n = records, box, info, map, n


class Rig(object):
    """R rigs of C cameras.  extrinsics: (C, 3, 4) or (C, 4, 4) - the same for every rig - or (R, C, 3, 4) / (R, C, 4, 4), camera
    coordinates -> rig frame, checked on the host before the upload.  cap: fused slots per rig (1..256); None = min(256, C * topk)
    of the first ``fuse``.  A Rig belongs to one torch stream, like a track.Tracker (the workspace is its own)."""

    def __init__(self, extrinsics, R=1, cap=None, params=None, device='cuda'):
        ext = check_extrinsics(extrinsics, R)
        if cap is not None and not 1 <= int(cap) <= MAX_CAP:
            raise ValueError('Rig: cap must be in 1..%d, got %r' % (MAX_CAP, cap))
        lib = _lib.load()
        d = torch.device(device)
        if d.type != 'cuda':
            raise RuntimeError('rtm3d_amd.rig.Rig needs a CUDA (ROCm) device; there is no CPU path')
        self.device = torch.device('cuda', d.index if d.index is not None else torch.cuda.current_device())
        self.R, self.C = int(ext.shape[0]), int(ext.shape[1])
        self.cap = None if cap is None else int(cap)
        self.params = RigParams() if params is None else params
        self.lib = lib
        self.extrinsics = torch.from_numpy(ext.reshape(self.R * self.C, 12)).to(self.device)
        self._ws = None

    def check_sizes(self, topk):
        """The cap this rig runs records of ``topk`` slots with; ValueError for sizes rtm3d_rig_fuse would refuse."""
        topk = int(topk)
        if not 1 <= topk <= MAX_TOPK or self.C * topk > MAX_SLOTS:
            raise ValueError('Rig: topk %d with %d cameras (topk 1..%d, C * topk at most %d)' % (topk, self.C, MAX_TOPK, MAX_SLOTS))
        return min(MAX_CAP, self.C * topk) if self.cap is None else self.cap

    def fuse(self, rec):
        """One frame of every rig (rtm3d_rig_fuse) on the current stream.  rec: the contiguous (R * C, topk, 32) fp32 CUDA records
        (read only), image index r * C + c.  Returns a ``Fused``."""
        if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
            raise RuntimeError('rtm3d_amd.rig.Rig.fuse needs CUDA (ROCm) tensors; there is no CPU path')
        if rec.dtype != torch.float32 or rec.dim() != 3 or rec.shape[0] != self.R * self.C or rec.shape[2] != 32 or not rec.is_contiguous() \
                or rec.device != self.device:
            raise ValueError('Rig.fuse: rec must be a contiguous fp32 tensor (%d, topk, 32) on %s, got %s %s'
                             % (self.R * self.C, self.device, rec.dtype, tuple(rec.shape)))
        topk = int(rec.shape[1])
        cap = self.check_sizes(topk)
        if self.cap is None:
            self.cap = cap
        R, C = self.R, self.C
        with torch.cuda.device(self.device):
            need = int(self.lib.rtm3d_rig_workspace_bytes(R, C, topk))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
            out = Fused(torch.empty(R, cap, 32, dtype=torch.float32, device=self.device),
                        torch.empty(R, cap, 7, dtype=torch.float64, device=self.device),
                        torch.empty(R, cap, 4, dtype=torch.int32, device=self.device),
                        torch.empty(R * C, topk, dtype=torch.int32, device=self.device),
                        torch.empty(R, 2, dtype=torch.int32, device=self.device))
            p = self.params.to_c()
            P = lambda t: ctypes.c_void_p(t.data_ptr())
            _lib.check(self.lib.rtm3d_rig_fuse(ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), R, C, topk, cap, P(rec),
                                               P(self.extrinsics), ctypes.byref(p), P(out.records), P(out.box), P(out.info), P(out.map),
                                               P(out.n), P(self._ws)), 'rig_fuse')
        return out

    def camera_ids(self, ids_rig, fused):
        """rtm3d_rig_scatter_ids: the (R, cap) int32 ids of the fused records - what Tracker.update returns for ``fused.records`` -
        taken to the cameras' record slots: (R * C, topk) int32, 0 where the slot is no candidate or its cluster was dropped."""
        if not isinstance(ids_rig, torch.Tensor) or not ids_rig.is_cuda:
            raise RuntimeError('rtm3d_amd.rig.Rig.camera_ids needs CUDA (ROCm) tensors; there is no CPU path')
        cap, topk = int(fused.records.shape[1]), int(fused.map.shape[1])
        if ids_rig.dtype != torch.int32 or tuple(ids_rig.shape) != (self.R, cap) or not ids_rig.is_contiguous() or ids_rig.device != self.device:
            raise ValueError('Rig.camera_ids: ids_rig must be a contiguous int32 tensor (%d, %d) on %s, got %s %s'
                             % (self.R, cap, self.device, ids_rig.dtype, tuple(ids_rig.shape)))
        if tuple(fused.map.shape) != (self.R * self.C, topk):
            raise ValueError('Rig.camera_ids: fused.map has shape %s, this rig runs (%d, topk)' % (tuple(fused.map.shape), self.R * self.C))
        with torch.cuda.device(self.device):
            ids = torch.empty(self.R * self.C, topk, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.rtm3d_rig_scatter_ids(ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), self.R, self.C, topk,
                                                      cap, ctypes.c_void_p(fused.map.data_ptr()), ctypes.c_void_p(ids_rig.data_ptr()),
                                                      ctypes.c_void_p(ids.data_ptr())), 'rig_scatter_ids')
        return ids
