"""Tracking of the kept 3D boxes across frames on the device (csrc/track.hip; the rule: include/rtm3d_hip.h, "tracking").

One ``Tracker`` holds B independent streams, one per batch index of the (B, topk, 32) records: a table of ``capacity`` track
slots per stream in device memory, a constant-velocity Kalman filter per slot, and a greedy association of each frame's
detections (flag 2, score >= min_score) to the live tracks on BEV IoU, 3D IoU or centre distance.  ``update`` is two launches on
the current stream and never synchronises; the records are not modified.  Device tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _lib

METRICS = {'bev': 0, '3d': 1, 'dist': 2}
MAX_TRACKS = 256
MAX_TOPK = 256
ASSIGNMENTS = {'greedy': 0, 'optimal': 1}     # RTM3D_TRACK_ASSIGN_GREEDY, RTM3D_TRACK_ASSIGN_OPTIMAL
HEADER, SLOT = 8, 24          # RTM3D_TRACK_HEADER_DOUBLES, RTM3D_TRACK_SLOT_DOUBLES

_DEFAULTS = dict(metric='3d', class_aware=False, max_misses=2, min_hits=3, thresh=0.01, min_score=0.0, p0_pos=10.0, p0_vel=1e4,
                 p0_ry=10.0, p0_dim=10.0, q_pos=0.0, q_vel=0.01, q_ry=0.0, q_dim=0.0, r_pos=1.0, r_ry=1.0, r_dim=1.0)


class TrackParams(object):
    """The parameters of rtm3d_tracks_update (struct rtm3d_track_params); the defaults are rtm3d_track_default_params'.
    metric: 'bev' | '3d' (IoU of the predicted box and the detection) | 'dist' (minus the centre distance in metres); a pair can
    match only if its affinity is strictly greater than ``thresh``.  class_aware: only boxes of the track's class match it.
    max_misses: a track is freed once it has missed more than this many frames in a row.  min_hits: a track is confirmed (+id)
    after this many matched frames in a row, or while the stream has seen no more than this many frames.  p0_* initial
    variances, q_* process noise per unit of dt, r_* measurement noise - of position / velocity, ry, and the dimensions."""

    def __init__(self, **kw):
        unknown = set(kw) - set(_DEFAULTS)
        if unknown:
            raise ValueError('TrackParams: unknown parameters %s (known: %s)' % (sorted(unknown), sorted(_DEFAULTS)))
        for k, v in _DEFAULTS.items():
            setattr(self, k, kw.get(k, v))
        if self.metric not in METRICS:
            raise ValueError("TrackParams: metric must be one of %s, got %r" % (sorted(METRICS), self.metric))

    def to_c(self):
        p = _lib.TrackParamsC()
        p.metric, p.class_aware = METRICS[self.metric], 1 if self.class_aware else 0
        p.max_misses, p.min_hits = int(self.max_misses), int(self.min_hits)
        for k in ('thresh', 'min_score', 'p0_pos', 'p0_vel', 'p0_ry', 'p0_dim', 'q_pos', 'q_vel', 'q_ry', 'q_dim', 'r_pos', 'r_ry', 'r_dim'):
            setattr(p, k, float(getattr(self, k)))
        return p


class Tracker(object):
    """B streams of at most ``capacity`` (1..256) tracks each.  ``dt`` and ``ego`` are what Engine.detect / detect_frames pass to
    ``update`` when they are given this tracker.
    A Tracker belongs to ONE torch stream: the table and the affinity workspace are its own and every ``update`` / ``reset`` is
    ordered only by the stream it is issued on.  Calling it from a second stream needs the caller's event between the two (as for
    any tensor shared between streams); use one Tracker per stream otherwise.
    assignment: 'greedy' (step 3 of the rule: the best remaining pair first) or 'optimal' (step 3b: the matching of candidate pairs
    with the largest sum of affinity - thresh; keeps the identities of neighbours that greedy swaps); kept as ``tracker.assignment``."""

    def __init__(self, B, capacity=128, params=None, device='cuda', assignment='greedy'):
        if assignment not in ASSIGNMENTS:
            raise ValueError("Tracker: assignment must be one of %s, got %r" % (sorted(ASSIGNMENTS), assignment))
        self.assignment = assignment
        lib = _lib.load()
        d = torch.device(device)
        if d.type != 'cuda':
            raise RuntimeError('rtm3d_amd.track.Tracker needs a CUDA (ROCm) device; there is no CPU path')
        self.device = torch.device('cuda', d.index if d.index is not None else torch.cuda.current_device())
        self.B, self.capacity = int(B), int(capacity)
        nbytes = int(lib.rtm3d_tracks_state_bytes(self.B, self.capacity))
        if nbytes == 0:
            raise ValueError('Tracker: B must be positive and capacity in 1..%d, got B %d, capacity %d' % (MAX_TRACKS, self.B, self.capacity))
        self.params = TrackParams() if params is None else params
        self.dt, self.ego = 1.0, None
        self.state = torch.zeros(self.B, HEADER + SLOT * self.capacity, dtype=torch.float64, device=self.device)
        assert self.state.numel() * 8 == nbytes
        self._ws = None

    def update(self, rec, dt=1.0, ego=None):
        """One frame of every stream (rtm3d_tracks_update_assign) on the current stream.  rec: the contiguous (B, topk, 32) fp32 CUDA
        records of this frame (read only).  dt: time since the previous call.  ego: None or (B, 12) / (B, 3, 4) float64 CUDA
        [R | t] per stream, previous camera coordinates -> current.  Returns the (B, topk) int32 ids: +id confirmed track, -id
        tentative track, 0 not tracked."""
        if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
            raise RuntimeError('rtm3d_amd.track.Tracker.update needs CUDA (ROCm) tensors; there is no CPU path')
        if rec.dtype != torch.float32 or rec.dim() != 3 or rec.shape[0] != self.B or rec.shape[2] != 32 or not rec.is_contiguous() \
                or rec.device != self.device:
            raise ValueError('Tracker.update: rec must be a contiguous fp32 tensor (%d, topk, 32) on %s, got %s %s'
                             % (self.B, self.device, rec.dtype, tuple(rec.shape)))
        topk = int(rec.shape[1])
        e_ptr = None
        if ego is not None:
            if not isinstance(ego, torch.Tensor) or not ego.is_cuda:
                raise RuntimeError('rtm3d_amd.track.Tracker.update needs CUDA (ROCm) tensors; there is no CPU path')
            if ego.dtype != torch.float64 or ego.numel() != self.B * 12 or ego.device != self.device:
                raise ValueError('Tracker.update: ego must be a float64 tensor (%d, 12) on %s' % (self.B, self.device))
            ego = ego.reshape(self.B, 12).contiguous()
            e_ptr = ctypes.c_void_p(ego.data_ptr())
        lib = _lib.load()
        with torch.cuda.device(self.device):
            need = int(lib.rtm3d_tracks_workspace_bytes(self.B, topk, self.capacity))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
            ids = torch.empty(self.B, topk, dtype=torch.int32, device=self.device)
            p = self.params.to_c()
            _lib.check(lib.rtm3d_tracks_update_assign(ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), self.B, topk,
                                                      self.capacity, ctypes.c_void_p(rec.data_ptr()), float(dt), e_ptr, ctypes.byref(p),
                                                      ASSIGNMENTS[self.assignment], ctypes.c_void_p(self.state.data_ptr()),
                                                      ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(self._ws.data_ptr())), 'tracks_update')
        return ids

    def tracks(self):
        """The table as named views of the state tensor (no copy, float64): per stream 'issued' (ids given so far), 'frame',
        'dropped'; per slot (B, capacity) 'id', 'cls', 'age', 'hits', 'misses', 'score', 'slot' (record slot matched in the last
        frame, -1 none), 'var_ry', 'var_dim'; (B, capacity, 7) 'box' = h w l X Y Z ry; (B, capacity, 3) 'vel' and 'cov' = Ppp Ppv
        Pvv; and 'live' = id != 0 (a new bool tensor)."""
        s = self.state[:, HEADER:].view(self.B, self.capacity, SLOT)
        out = {'issued': self.state[:, 0], 'frame': self.state[:, 1], 'dropped': self.state[:, 2]}
        for i, name in enumerate(('id', 'cls', 'age', 'hits', 'misses', 'score', 'slot')):
            out[name] = s[..., i]
        out.update(box=s[..., 7:14], vel=s[..., 14:17], cov=s[..., 17:20], var_ry=s[..., 20], var_dim=s[..., 21], live=s[..., 0] != 0)
        return out

    def reset(self, streams=None):
        """Empty all streams (None) or the listed ones: a zero fill on the current stream, the reset the table defines."""
        if streams is None:
            self.state.zero_()
        else:
            for b in streams:
                self.state[int(b)].zero_()
