"""Validation loss on the device: KITTI labels -> targets -> RTM3D loss (csrc/loss.hip; the rule: include/rtm3d_hip.h,
"validation loss").

The reference selects checkpoints by the mean of ``RTM3DLoss`` over the validation set (train.py:61-81, ``test_epoch``).  Here
the label rows are packed on the host into one fp64 row per object (``LabelBatch``), the device derives the reference's target
fields from them (``build_targets``: m_proj, m_off, v_proj, v_off, v_coor_off, v_mask, mask_3d and, for inspection, m_hm) and
``RTM3DLoss(cfg)(pred_logits, batch)`` evaluates the loss of models/rtm3d_loss.py:268-340 on the four logit maps of
``Model.forward`` without ever writing the heat-map target.  ``ValidationLoss`` keeps test_epoch's running sum on the device:
``add`` does no host synchronisation, ``result()`` synchronises once.  The loss is differentiable with respect to the four
logit maps (the header's "loss gradient", rtm3d_loss_grad): with logits that require grad, ``loss`` carries a ``grad_fn`` and
``loss.backward()`` is the line that follows it in the reference's train_epoch; ``RTM3DLoss.grad`` is the same gradient
without autograd.  There is no second derivative, no optimiser and no training loop.  Device tensors only: there is no CPU path.

``mask_3d`` is "all eight corners in front of the camera" unless the caller supplies it: PARITY UNPINNED, the reference takes
it from a KITTI devkit module that its tree does not contain.
"""
import ctypes

import numpy as np

from . import _lib

ROW, TABLE = 18, 88                      # RTM3D_LOSS_ROW, RTM3D_LOSS_TABLE
MAX_OBJECTS = 1 << 20                    # RTM3D_LOSS_MAX_OBJECTS
MAX_COORD = float(1 << 20)               # |bbox| in input pixels
ITEMS = ('main_kf', 'ver_coor', 'main_off', 'vertex_off', 'total')
COUNTS = ('num_pos', 'n_ver_coor', 'n_vertex_off', 'n_main_off', 'n_outside')
# the reference's defaults (models/configs/detault.py)
DEFAULT_RELATE_OBJS = (('Van', 'Truck'), ('Person_sitting',), ('Person_sitting',))
DEFAULTS = {('TRAINING', 'W_MKF'): 1.0, ('TRAINING', 'W_VFM'): 1.0, ('TRAINING', 'W_M_OFF'): 0.5, ('TRAINING', 'W_V_OFF'): 0.5,
            ('MODEL', 'FOCAL_LOSS_ALPHA'): 2.0, ('MODEL', 'FOCAL_LOSS_BEDA'): 4.0, ('MODEL', 'DOWN_SAMPLE'): 4.0,
            ('DATASET', 'GAUSSIAN_GEN_TYPE'): 'dynamic_radius', ('DATASET', 'RELATE_OBJs'): DEFAULT_RELATE_OBJS,
            ('DATASET', 'OBJs'): ('Car', 'Pedestrian', 'Cyclist')}


def cfg_get(cfg, node, key):
    """cfg.<node>.<key>, or the reference's default where the tree does not carry the key."""
    sub = cfg.get(node) if cfg is not None and hasattr(cfg, 'get') else getattr(cfg, node, None)
    if sub is not None:
        v = sub.get(key) if hasattr(sub, 'get') else getattr(sub, key, None)
        if v is not None:
            return v
    return DEFAULTS[(node, key)]


def _check_gaussian_type(cfg):
    kind = cfg_get(cfg, 'DATASET', 'GAUSSIAN_GEN_TYPE')
    if kind != 'dynamic_radius':
        raise NotImplementedError("DATASET.GAUSSIAN_GEN_TYPE = %r: only 'dynamic_radius' is built (the reference's dataset path for "
                                  "'dynamic_sigma' calls torch.sqrt on a numpy array and cannot run)" % (kind,))


def transform_obj_label(types, objs, relate_objs):
    """_transform_obj_label (datasets/dataset_reader.py:197-213) on type names: -> (cls, noise, repeats).  A type in ``objs``
    is one row of its class; a type listed in relate_objs[k] becomes one noise row of class k per list that contains it;
    everything else one row with cls = -1."""
    objs = list(objs)
    cls, noise, repeats = [], [], []
    for t in types:
        if t in objs:
            cls.append(objs.index(t)); noise.append(0); repeats.append(1)
            continue
        ks = [k for k, rel in enumerate(relate_objs) if t in rel]
        if ks:
            cls += ks; noise += [1] * len(ks); repeats.append(len(ks))
        else:
            cls.append(-1); noise.append(0); repeats.append(1)
    return np.asarray(cls, np.int64), np.asarray(noise, np.int64), repeats


class LabelBatch:
    """The objects of B images as the rows of rtm3d_loss_objects.  Everything is checked here, on the host, before anything
    is launched: a bad batch raises ValueError and touches no device.

    img_id (N,) non-decreasing in [0, B); cls (N,) in [-1, num_classes), -1 = mask 0; noise (N,) 0 / 1; bbox (N, 4) x1 y1 x2
    y2 in network-input pixels; dimension (N, 3) h w l; location (N, 3) the KITTI bottom centre; Ry (N,); K (B, 9) or (B, 3, 3)
    in input pixels; mask_3d (N,) 0 / 1 or None (derived: all eight corners in front of the camera)."""

    def __init__(self, B, img_id, cls, noise, bbox, dimension, location, Ry, K, mask_3d=None, num_classes=3, down_sample=4.0):
        B = int(B)
        if B < 1 or B > 65535:
            raise ValueError('LabelBatch: B = %d images (1..65535)' % B)
        img_id = np.asarray(img_id).reshape(-1)
        N = img_id.size
        if N > MAX_OBJECTS:
            raise ValueError('LabelBatch: %d objects are more than the %d one batch holds' % (N, MAX_OBJECTS))
        f = lambda a, shape, name: self._field(a, (N,) + shape, name)
        cls, noise = f(cls, (), 'cls'), f(noise, (), 'noise')
        bbox, dimension, location, Ry = f(bbox, (4,), 'bbox'), f(dimension, (3,), 'dimension'), f(location, (3,), 'location'), f(Ry, (), 'Ry')
        img_id = f(img_id, (), 'img_id')
        K = np.asarray(K, np.float64)
        if K.size != B * 9 or not np.isfinite(K).all():
            raise ValueError('LabelBatch: K must hold one finite 3 x 3 matrix per image (%d images), got shape %s' % (B, K.shape))
        num_classes = int(num_classes)
        if num_classes < 1 or num_classes > 65535:
            raise ValueError('LabelBatch: num_classes = %d' % num_classes)
        if (img_id != np.floor(img_id)).any() or (img_id < 0).any() or (img_id >= B).any():
            raise ValueError('LabelBatch: img_id outside 0..%d' % (B - 1))
        if (np.diff(img_id) < 0).any():
            raise ValueError('LabelBatch: img_id must be non-decreasing (the objects of an image are consecutive rows)')
        if (cls != np.floor(cls)).any() or (cls < -1).any() or (cls >= num_classes).any():
            raise ValueError('LabelBatch: cls outside -1..%d' % (num_classes - 1))
        if not np.isin(noise, (0.0, 1.0)).all():
            raise ValueError('LabelBatch: noise must be 0 or 1')
        if (bbox[:, 2] < bbox[:, 0]).any() or (bbox[:, 3] < bbox[:, 1]).any():
            raise ValueError('LabelBatch: a bbox with x2 < x1 or y2 < y1 (its Gaussian radius is not defined)')
        if (np.abs(bbox) > MAX_COORD).any():
            raise ValueError('LabelBatch: a bbox coordinate beyond %g input pixels' % MAX_COORD)
        if not (float(down_sample) > 0 and float(down_sample) <= 1e6):
            raise ValueError('LabelBatch: down_sample = %r' % (down_sample,))
        if mask_3d is None:
            m3 = np.full(N, -1.0)
        else:
            m3 = f(mask_3d, (), 'mask_3d')
            if not np.isin(m3, (0.0, 1.0)).all():
                raise ValueError('LabelBatch: mask_3d must be 0 or 1 (or None: derived)')
        rows = np.zeros((N, ROW))
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:7], rows[:, 7:10], rows[:, 10:13], rows[:, 13] = img_id, cls, noise, bbox, dimension, location, Ry
        rows[:, 14], rows[:, 15], rows[:, 16] = np.sin(Ry), np.cos(Ry), m3
        self.B, self.N, self.num_classes, self.down_sample = B, N, num_classes, float(down_sample)
        self.rows = rows
        self.K = np.ascontiguousarray(K.reshape(B, 9))
        self.img_start = np.searchsorted(img_id, np.arange(B + 1), side='left').astype(np.int32)
        self.device = None
        self._dev = None
        self._tables = {}

    @staticmethod
    def _field(a, shape, name):
        a = np.asarray(a, np.float64)
        if a.size != int(np.prod(shape)):
            raise ValueError('LabelBatch: %s must have shape %s, got %s' % (name, shape, a.shape))
        a = a.reshape(shape)
        if not np.isfinite(a).all():
            raise ValueError('LabelBatch: %s holds a value that is not finite' % name)
        return a

    @staticmethod
    def from_kitti(rows_per_image, K_per_image, cfg=None, scale=1.0, pad=(0.0, 0.0), mask_3d=None):
        """KITTI label rows -> LabelBatch.  rows_per_image: a ``kitti_eval.Labels`` (``kitti_eval.read_label_dir``) or, per
        image, a list of rows ``(type, truncated, occluded, alpha, x1, y1, x2, y2, h, w, l, x, y, z, rotation_y[, score])``.
        K_per_image: (B, 3, 3) / (B, 9) camera matrices of the ORIGINAL images.  scale / pad: the caller's resize and
        letterbox - scale s, (sx, sy) or one (sx, sy) per image as (B, 2); pad (pad_w, pad_h) or (B, 2): bbox -> bbox * scale +
        pad, K's first two rows times the scale and its principal point plus the pad.  mask_3d: None, or per image
        one 0 / 1 per label row (a row doubled by the class mapping carries its value twice).  Classes come from
        cfg.DATASET.OBJs and cfg.DATASET.RELATE_OBJs (the reference's defaults where the tree lacks them)."""
        from . import kitti_eval
        _check_gaussian_type(cfg)
        if isinstance(rows_per_image, kitti_eval.Labels):
            lab = rows_per_image
        else:
            frames = []
            for rows in rows_per_image:
                fr = []
                for r in rows:
                    r = list(r)
                    if len(r) not in (15, 16):
                        raise ValueError('LabelBatch.from_kitti: a label row has 15 fields (16 with a score), got %d: %r' % (len(r), r))
                    fr.append([str(r[0])] + [float(v) for v in r[1:]] + ([0.0] if len(r) == 15 else []))
                frames.append(fr)
            lab = kitti_eval._frames_to_labels(list(range(len(frames))), frames)
        B = len(lab)
        K = np.array(K_per_image, np.float64)
        if K.size != B * 9:
            raise ValueError('LabelBatch.from_kitti: %d label frames, K of shape %s' % (B, K.shape))
        K = K.reshape(B, 3, 3).copy()
        sc = np.broadcast_to(np.asarray(scale, np.float64), (B, 2)).astype(np.float64)
        pd = np.broadcast_to(np.asarray(pad, np.float64), (B, 2)).astype(np.float64)
        K[:, 0, :] *= sc[:, 0:1]; K[:, 1, :] *= sc[:, 1:2]
        K[:, 0, 2] += pd[:, 0]; K[:, 1, 2] += pd[:, 1]
        objs, rel = list(cfg_get(cfg, 'DATASET', 'OBJs')), [list(r) for r in cfg_get(cfg, 'DATASET', 'RELATE_OBJs')]
        img_id, cls, noise, bbox, dim, loc, ry, m3 = [], [], [], [], [], [], [], []
        for b in range(B):
            n = int(lab.n[b])
            c, nz, rep = transform_obj_label([str(t) for t in lab.type[b, :n]], objs, rel)
            idx = np.repeat(np.arange(n), rep)
            box = lab.rect[b, idx] * np.tile(sc[b], 2) + np.tile(pd[b], 2)
            img_id.append(np.full(len(idx), b)); cls.append(c); noise.append(nz); bbox.append(box)
            dim.append(lab.hwl[b, idx]); loc.append(lab.xyz[b, idx]); ry.append(lab.ry[b, idx])
            if mask_3d is not None:
                m = np.asarray(mask_3d[b], np.float64).reshape(-1)
                if m.size != n:
                    raise ValueError('LabelBatch.from_kitti: mask_3d of image %d holds %d values for %d rows' % (b, m.size, n))
                m3.append(m[idx])
        cat = lambda parts, tail: np.concatenate(parts).reshape((-1,) + tail) if parts else np.zeros((0,) + tail)
        return LabelBatch(B, cat(img_id, ()), cat(cls, ()), cat(noise, ()), cat(bbox, (4,)), cat(dim, (3,)), cat(loc, (3,)), cat(ry, ()),
                          K, mask_3d=cat(m3, ()) if mask_3d is not None else None, num_classes=len(objs),
                          down_sample=cfg_get(cfg, 'MODEL', 'DOWN_SAMPLE'))

    # ---- device side
    def to(self, device):
        """Upload the rows (once per device) on the current stream; returns self.  Three copies from pinned host memory with
        ``non_blocking``: the host does not wait for them, and everything that reads them is ordered behind them on that
        stream.  A loader that calls ``batch.to(device).table(H, W)`` when it makes the batch keeps the upload and the table
        launch out of the evaluation step altogether."""
        import torch
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('rtm3d_amd.loss needs a CUDA (ROCm) device; there is no CPU path')
        dev = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        if self.device != dev:
            self._pinned = tuple(torch.from_numpy(a).pin_memory() for a in (self.rows, self.K, self.img_start))   # kept alive
            self._dev = tuple(h.to(dev, non_blocking=True) for h in self._pinned)
            self.device, self._tables = dev, {}
        return self

    def table(self, H, W):
        """The derived per-object table (N, 88) float64 for an H x W map (rtm3d_loss_objects; cached per size)."""
        import torch
        if self.device is None:
            raise RuntimeError('LabelBatch.table: call batch.to(device) first')
        key = (int(H), int(W))
        if key not in self._tables:
            rows, K, _ = self._dev
            with torch.cuda.device(self.device):
                tab = torch.empty(max(self.N, 1), TABLE, dtype=torch.float64, device=self.device)
                _lib.check(_lib.load().rtm3d_loss_objects(_lib.stream_ptr(self.device), self.N, self.B, rows.data_ptr(), K.data_ptr(),
                                                          self.down_sample, key[0], key[1], tab.data_ptr()), 'loss_objects')
            self._tables[key] = tab
        return self._tables[key]


def build_targets(batch, H, W, device=None):
    """The reference's target fields (datasets/dataset_reader.py:215-291) of ``batch`` for an H x W map, as device tensors:
    m_hm (B, C, H, W) fp32; m_proj (N, 2) int64; m_off (N, 2); v_proj (N, 8, 2) int64; v_off, v_coor_off (N, 8, 2); v_mask
    (N, 8) bool; mask_3d, mask, noise_mask (N,) bool; img_id, class (N,) int64; plus radius, sigma (N,) and the raw table.
    ``RTM3DLoss`` needs none of this: m_hm exists here for inspection and tests."""
    import torch
    if device is not None or batch.device is None:
        batch.to(device if device is not None else 'cuda')
    dev, N = batch.device, batch.N
    tab = batch.table(H, W)
    with torch.cuda.device(dev):
        hm = torch.empty(batch.B, batch.num_classes, int(H), int(W), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().rtm3d_loss_heatmap(_lib.stream_ptr(dev), batch.B, batch.num_classes, int(H), int(W), batch._dev[2].data_ptr(),
                                                  tab.data_ptr(), N, hm.data_ptr()), 'loss_heatmap')
    t = tab[:N]
    return {'m_hm': hm, 'img_id': t[:, 0].long(), 'class': t[:, 1].long(), 'mask': t[:, 2] != 0, 'noise_mask': t[:, 3] != 0,
            'mask_3d': t[:, 4] != 0, 'm_proj': t[:, 8:10].long(), 'm_off': t[:, 10:12].clone(), 'radius': t[:, 14].clone(),
            'sigma': t[:, 13].clone(), 'v_proj': t[:, 32:48].reshape(N, 8, 2).long(), 'v_off': t[:, 48:64].reshape(N, 8, 2).clone(),
            'v_coor_off': t[:, 64:80].reshape(N, 8, 2).clone(), 'v_mask': t[:, 80:88] != 0, 'table': t}


class RTM3DLoss:
    """``RTM3DLoss(cfg)(pred_logits, batch) -> (loss, loss_items)``: the reference's signature (models/rtm3d_loss.py:268) with a
    ``LabelBatch`` where it takes its ParamList of targets.  pred_logits: the four fp32 NCHW logit maps of ``Model.forward`` -
    heat map (B, C, H, W), ver_coor (B, 16, H, W), m_off (B, 2, H, W), v_off (B, 2, H, W).  loss_items: (5,) fp32 device tensor
    W_MKF * main, W_VFM * ver_coor, W_M_OFF * main_off, W_V_OFF * vertex_off, total; loss is its last entry.  ``counts`` holds
    the (5,) int32 device tensor num_pos, the three selection sizes and n_outside of the last call.  Two launches on the current
    stream, no host synchronisation - but the first call with a batch uploads its rows (``LabelBatch.to``: asynchronous) and
    launches its table kernel; do both ahead with ``batch.to(device).table(H, W)`` where that matters.  An empty selection
    gives NaN, as F.l1_loss of nothing does in the reference.
    When grad mode is on and any of the four maps requires grad, ``loss`` carries a ``grad_fn`` (a once-differentiable autograd
    node; ``loss_items`` stays detached, as in the reference): its backward is rtm3d_loss_grad on the current stream - two more
    launches, the upstream gradient passed as a device scalar, only the maps that need a gradient computed, no host
    synchronisation.  Otherwise, and under ``torch.no_grad()``, the call is the forward alone, value for value and launch for
    launch.  ``grad(pred_logits, batch, upstream)`` returns the same four gradients without autograd.
    ONE STREAM PER OBJECT: the workspace is cached per shape and reused by every call, so calls through one RTM3DLoss must be
    issued on one stream (or be ordered by the caller); use one object per stream.  That holds for the backward too: it reads the
    ``counts`` its forward left on the device, so ``loss.backward()`` belongs on the stream of the call that made ``loss``."""

    def __init__(self, cfg=None):
        _check_gaussian_type(cfg)
        self.alpha, self.beta = float(cfg_get(cfg, 'MODEL', 'FOCAL_LOSS_ALPHA')), float(cfg_get(cfg, 'MODEL', 'FOCAL_LOSS_BEDA'))
        self.weights = tuple(float(cfg_get(cfg, 'TRAINING', k)) for k in ('W_MKF', 'W_VFM', 'W_M_OFF', 'W_V_OFF'))
        if not (0 < self.alpha <= 64 and 0 < self.beta <= 64):
            raise ValueError('MODEL.FOCAL_LOSS_ALPHA / FOCAL_LOSS_BEDA must lie in (0, 64], got %r / %r' % (self.alpha, self.beta))
        if any(w != w for w in self.weights):
            raise ValueError('TRAINING.W_*: a weight is NaN')
        self._params = _lib.LossParamsC(self.alpha, self.beta, (ctypes.c_float * 4)(*self.weights))
        self._ws = {}
        self.counts = None
        self._items = None                   # loss_items of the last call that went through autograd

    def _check(self, pred_logits, batch):
        import torch
        if not isinstance(batch, LabelBatch):
            raise TypeError('RTM3DLoss: targets must be a rtm3d_amd.loss.LabelBatch, got %s' % type(batch).__name__)
        pred = tuple(pred_logits)
        if len(pred) != 4:
            raise ValueError('RTM3DLoss: pred_logits must be the four logit maps, got %d' % len(pred))
        hm = pred[0]
        if not isinstance(hm, torch.Tensor) or hm.dim() != 4:
            raise ValueError('RTM3DLoss: the heat-map logits must be a (B, C, H, W) tensor')
        if not hm.is_cuda:
            raise RuntimeError('rtm3d_amd.loss.RTM3DLoss needs CUDA (ROCm) tensors; there is no CPU path')
        B, C, H, W = hm.shape
        for t, ch, name in zip(pred, (C, 16, 2, 2), ('heat map', 'ver_coor', 'm_off', 'v_off')):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, ch, H, W) or t.dtype != torch.float32 or t.device != hm.device \
                    or not t.is_contiguous():
                raise ValueError('RTM3DLoss: the %s logits must be a contiguous fp32 tensor %s on %s' % (name, (B, ch, H, W), hm.device))
        if B != batch.B or C != batch.num_classes:
            raise ValueError('RTM3DLoss: logits of %d images x %d classes, labels of %d x %d' % (B, C, batch.B, batch.num_classes))
        return pred, B, C, H, W

    def _eval(self, pred_logits, batch, accum):
        import torch
        pred, B, C, H, W = self._check(pred_logits, batch)
        dev = pred[0].device
        batch.to(dev)
        tab = batch.table(H, W)
        lib = _lib.load()
        with torch.cuda.device(dev):
            key = (dev.index, B, C, H, W)
            if key not in self._ws:
                self._ws[key] = torch.empty(max(int(lib.rtm3d_loss_workspace_bytes(B, C, H, W)), 8) // 8, dtype=torch.float64, device=dev)
            items = torch.empty(5, dtype=torch.float32, device=dev)
            counts = torch.empty(5, dtype=torch.int32, device=dev)
            _lib.check(lib.rtm3d_loss_eval(_lib.stream_ptr(dev), B, C, H, W, pred[0].data_ptr(), pred[1].data_ptr(), pred[2].data_ptr(),
                                           pred[3].data_ptr(), batch._dev[2].data_ptr(), tab.data_ptr(), batch.N, ctypes.byref(self._params),
                                           self._ws[key].data_ptr(), items.data_ptr(), counts.data_ptr(),
                                           accum.data_ptr() if accum is not None else None), 'loss_eval')
        self.counts = counts
        return items[4], items

    def __call__(self, pred_logits, targets):
        import torch
        pred = tuple(pred_logits)
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in pred):
            loss = _loss_function().apply(self, targets, *self._check(pred, targets)[0])
            return loss, self._items
        return self._eval(pred, targets, None)

    def grad(self, pred_logits, batch, upstream=None, counts=None, want=(True, True, True, True), out=None):
        """The gradient of ``loss`` with respect to the four logit maps, times ``upstream`` (a float, a one-element fp32 device
        tensor, or None = 1) - rtm3d_loss_grad, the explicit path without autograd: -> four tensors shaped like the maps (None
        where ``want`` is false).  ``counts``: the ``counts`` an earlier forward call on the same inputs left; without it
        the forward is evaluated first.  ``out``: four preallocated contiguous fp32 tensors (or None each) to write into.
        Two launches on the current stream, no host synchronisation, every element written."""
        import torch
        pred, B, C, H, W = self._check(pred_logits, batch)
        dev = pred[0].device
        if counts is None:
            with torch.no_grad():
                self._eval(pred, batch, None)
            counts = self.counts
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.numel() != 5 or counts.device != dev or not counts.is_contiguous():
            raise ValueError('RTM3DLoss.grad: counts must be the (5,) int32 tensor of a forward call on %s' % dev)
        want = tuple(bool(w) for w in want)
        if len(want) != 4 or not any(want):
            raise ValueError('RTM3DLoss.grad: want must hold four flags, at least one of them set')
        if upstream is not None:
            if isinstance(upstream, torch.Tensor):
                if upstream.numel() != 1:
                    raise ValueError('RTM3DLoss.grad: upstream must be one value, got shape %s' % (tuple(upstream.shape),))
                upstream = upstream.detach().reshape(1).to(device=dev, dtype=torch.float32).contiguous()
            else:
                upstream = torch.full((1,), float(upstream), dtype=torch.float32, device=dev)
        batch.to(dev)
        tab = batch.table(H, W)
        with torch.cuda.device(dev):
            outs = []
            for k, (p, w) in enumerate(zip(pred, want)):
                o = out[k] if out is not None and w else None
                if o is not None and (not isinstance(o, torch.Tensor) or o.shape != p.shape or o.dtype != torch.float32 or o.device != dev
                                      or not o.is_contiguous()):
                    raise ValueError('RTM3DLoss.grad: out[%d] must be a contiguous fp32 tensor %s on %s' % (k, tuple(p.shape), dev))
                outs.append(o if o is not None else (torch.empty_like(p.detach()) if w else None))
            ptr = lambda t: t.data_ptr() if t is not None else None
            _lib.check(_lib.load().rtm3d_loss_grad(_lib.stream_ptr(dev), B, C, H, W, pred[0].data_ptr(), pred[1].data_ptr(), pred[2].data_ptr(),
                                                   pred[3].data_ptr(), batch._dev[2].data_ptr(), tab.data_ptr(), batch.N,
                                                   ctypes.byref(self._params), counts.data_ptr(), ptr(upstream), *[ptr(o) for o in outs]),
                       'loss_grad')
        return tuple(outs)


_LossFunction = None


def _loss_function():
    """The autograd node of RTM3DLoss.__call__ (made on first use: this module imports without torch)."""
    global _LossFunction
    if _LossFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class _LossFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, fn, batch, hm, ver_coor, m_off, v_off):
                pred = (hm, ver_coor, m_off, v_off)
                loss, items = fn._eval(pred, batch, None)
                fn._items = items
                ctx.fn, ctx.batch, ctx.counts = fn, batch, fn.counts
                ctx.save_for_backward(*pred)
                return loss.clone()              # (not a view of loss_items, which stays a plain detached tensor)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_loss):
                want = ctx.needs_input_grad[2:6]
                return (None, None) + ctx.fn.grad(ctx.saved_tensors, ctx.batch, upstream=grad_loss, counts=ctx.counts, want=want)

    return _LossFunction


class ValidationLoss:
    """test_epoch's running mean (train.py:65-81) on the device: ``add(pred_logits, batch)`` evaluates the loss and adds
    total * B and B into a two-double device accumulator inside the same launch - no host synchronisation; ``result()``
    reads the accumulator (one synchronisation) and returns sum / count as a float (NaN before any add, or once a batch's
    loss was NaN: the reference checks every step on the host and stops, here the NaN arrives with the mean).  A batch that
    was not staged with ``batch.to(device).table(H, W)`` is uploaded (asynchronously) and gets its table inside ``add``.
    ONE STREAM PER OBJECT: the finish kernel updates the accumulator with a plain read-modify-write and the workspace is shared
    between calls; issue every ``add`` / ``reset`` / ``result`` of one ValidationLoss on one stream."""

    def __init__(self, cfg=None):
        self.loss = RTM3DLoss(cfg)
        self._acc = None

    def reset(self):
        if self._acc is not None:
            import torch
            with torch.cuda.device(self._acc.device):
                _lib.check(_lib.load().rtm3d_loss_accum_reset(_lib.stream_ptr(self._acc.device), self._acc.data_ptr()), 'loss_accum_reset')

    def add(self, pred_logits, batch):
        import torch
        dev = tuple(pred_logits)[0].device
        if self._acc is None or self._acc.device != dev:
            self._acc = torch.zeros(2, dtype=torch.float64, device=dev)
        return self.loss._eval(pred_logits, batch, self._acc)

    def result(self):
        if self._acc is None:
            return float('nan')
        import torch
        out = (ctypes.c_double * 2)()
        with torch.cuda.device(self._acc.device):
            _lib.check(_lib.load().rtm3d_loss_accum_read(_lib.stream_ptr(self._acc.device), self._acc.data_ptr(), out), 'loss_accum_read')
        return float(np.float32(out[0] / out[1])) if out[1] > 0 else float('nan')


def test_epoch(model, batches, cfg=None):
    """The reference's validation loop (train.py:61-81) over an iterable of ``(imgs, LabelBatch)``: model.eval(),
    ``model(imgs)[1]`` into the loss, the batch-size weighted mean.  Returns the mean, or None with a warning when
    it is not finite (the reference returns None at the first non-finite step)."""
    vl = ValidationLoss(cfg if cfg is not None else getattr(model, 'config', None))
    model.eval()
    for imgs, batch in batches:
        vl.add(model(imgs)[1], batch)
    mean = vl.result()
    if not np.isfinite(mean):
        print('validation loss is not finite: %s' % mean)
        return None
    print('validation loss: %s' % mean)
    return mean


test_epoch.__test__ = False              # (a library function, not a pytest test)
