"""Training augmentation on the device: frames and labels in one step (csrc/augment.hip; the rule: include/rtm3d_hip.h,
"training augmentation").

The reference feeds its loss from ``TrainAugmentation`` (preprocess/data_preprocess.py): RandomBrightnessContrast, GaussNoise,
RemoveBadBBox, Resize, RandomAffine(range=(1., 1.2), offset=0.), RandomMirror, then ``_apply_padding`` and ``Normalize`` - OpenCV
and albumentations on CPU workers, one image at a time.  Here the parameters of a batch are drawn on the host
(``AugmentParams.draw``), ``frames`` makes the network input of the whole batch in two launches per 32 frames and ``labels``
moves the KITTI rows in step, in fp64, operation by operation as the reference does - the same scale, offset and mirror drive
both.  ``TrainAugmentation`` is the three together.

The pixels are NOT those of OpenCV / albumentations (absent here): the photometric steps act on the source frame and ONE
bilinear resample with 5-bit weights follows where the reference resamples twice; the noise is an integer table look-up cut off
at 3.67 sigma.  The labels ARE the reference's, bit for bit (tests/golden/augment_cases.npz is made by its own code).  Out of
scope: the mosaic path, PhotometricDistort, an optimiser, a training loop.  Device tensors only: there is no CPU path for pixels.
"""
import ctypes

import numpy as np

from . import _frames, _lib
from ._frames import CHUNK  # noqa: F401  (a name the tests use)
from .loss import LabelBatch, cfg_get, transform_obj_label, _check_gaussian_type
from .preprocess import device_luts, frame_geometry, resized_size

MODES = {'fp32': 0, 'nhwc4': 1, 'uint8': 2}


class AugmentParams:
    """Per-frame arrays: alpha, beta (contrast gain, brightness as a fraction of 255), sigma (noise, in grey levels), seed
    (uint64, the Philox key), scale and offset (B, 2) of the affine ``dst = scale * src + offset`` in the pixels of the RESIZED
    frame, flip (mirror), fill (B, 3) uint8, the colour of canvas pixels the affine leaves without a source (none with the
    reference's scale >= 1 and offset = 0.)."""

    FIELDS = ('alpha', 'beta', 'sigma', 'seed', 'scale', 'offset', 'flip', 'fill')

    def __init__(self, alpha, beta, sigma, seed, scale, offset, flip, fill):
        self.alpha = np.array(alpha, np.float64).reshape(-1)
        B = self.alpha.size
        self.beta = np.array(beta, np.float64).reshape(B)
        self.sigma = np.array(sigma, np.float64).reshape(B)
        self.seed = np.array(seed, np.uint64).reshape(B)
        self.scale = np.array(scale, np.float64).reshape(B)
        self.offset = np.array(offset, np.float64).reshape(B, 2)
        self.flip = np.array(flip).astype(bool).reshape(B)
        self.fill = np.array(fill, np.uint8).reshape(B, 3)
        for name in ('alpha', 'beta', 'sigma', 'scale', 'offset'):
            if not np.isfinite(getattr(self, name)).all():
                raise ValueError('AugmentParams: %s holds a value that is not finite' % name)
        if (self.scale <= 0).any() or (self.sigma < 0).any():
            raise ValueError('AugmentParams: scale must be > 0 and sigma >= 0')

    def __len__(self):
        return self.alpha.size

    @staticmethod
    def identity(B):
        """Nothing happens: the frames of ``preprocess_batch``."""
        B = int(B)
        return AugmentParams(np.ones(B), np.zeros(B), np.zeros(B), np.zeros(B, np.uint64), np.ones(B), np.zeros((B, 2)), np.zeros(B, bool),
                             np.zeros((B, 3), np.uint8))

    @staticmethod
    def draw(B, hw, resize_to, rng, p_photometric=0.5, brightness_limit=0.2, contrast_limit=0.2, p_noise=0.5, var_limit=(10.0, 50.0),
             p_affine=0.5, scale_range=(1.0, 1.2), affine_offset=0.0, p_flip=0.5, fill=(0, 0, 0)):
        """One draw per frame from ``rng`` (a numpy.random.Generator); the defaults are the reference's TrainAugmentation:
        RandomBrightnessContrast(p=0.5) with albumentations' limits 0.2, GaussNoise(p=0.5) with variance U(10, 50),
        RandomAffine (p = 0.5, scale U(1, 1.2), offset = 0.), RandomMirror (p = 0.5).  hw: (h, w) of every frame, or one pair
        for all; resize_to: the longest side after Resize (None: the frames are fed at their own size).  The affine offset is
        the reference's: base = (float32(w') - float32(w') * float32(scale)) / 2 per axis, in float32 as its ``base_offset``
        is, then (2 u - 1) * affine_offset * |base| + base in float64."""
        B = int(B)
        hw = np.broadcast_to(np.asarray(hw, np.int64).reshape(-1, 2), (B, 2))
        p = AugmentParams.identity(B)
        p.fill[:] = np.asarray(fill, np.uint8).reshape(-1, 3)
        for b in range(B):
            if rng.random() < p_photometric:
                p.alpha[b] = 1.0 + rng.uniform(-contrast_limit, contrast_limit)
                p.beta[b] = rng.uniform(-brightness_limit, brightness_limit)
            if rng.random() < p_noise:
                p.sigma[b] = float(np.sqrt(rng.uniform(var_limit[0], var_limit[1])))
            p.seed[b] = rng.integers(0, 2 ** 64, dtype=np.uint64)
            if rng.random() < p_affine:
                h, w = (int(v) for v in hw[b])
                rh, rw = resized_size(h, w, resize_to) if resize_to else (h, w)
                scale = float(rng.uniform(scale_range[0], scale_range[1]))
                p.scale[b] = scale
                p.offset[b] = affine_offset_of(rw, rh, scale, rng.random(2), affine_offset)
            p.flip[b] = rng.random() < p_flip
        return p

    def select(self, idx):
        return AugmentParams(*[getattr(self, n)[idx] for n in self.FIELDS])


def affine_offset_of(rw, rh, scale, u=(0.5, 0.5), affine_offset=0.0):
    """RandomAffine's offset (preprocess/transforms.py:340-342) for a resized frame of rw x rh: float32 base, float64 result."""
    wh = np.array([rw, rh], dtype=np.float32)
    base = (wh - wh * np.float32(scale)) / np.float32(2.0)
    return (2 * np.asarray(u, np.float64) - 1) * affine_offset * np.abs(base) + base


def quantise(params):
    """(alpha_q, beta_q, sigma_q) int64 arrays: round(alpha * 65536), round(beta * 255 * 65536), round(sigma * 64)."""
    return (np.rint(params.alpha * 65536).astype(np.int64), np.rint(params.beta * 255 * 65536).astype(np.int64),
            np.rint(params.sigma * 64).astype(np.int64))


def descriptors(hw, params, size, resize_to=None):
    """The ctypes array of rtm3d_augment_frame for frames of sizes hw (B, 2) on the (H, W) canvas (host only): the rectangle
    and the map from rtm3d_frame_geometry and rtm3d_augment_geometry, the rest from ``params``.  Returns (array, geom)."""
    lib = _lib.load()
    hw = np.asarray(hw, np.int32).reshape(-1, 2)
    B = len(hw)
    if len(params) != B:
        raise ValueError('%d parameter sets for %d frames' % (len(params), B))
    geom = frame_geometry(hw, size, resize_to)
    aq, bq, sq = quantise(params)
    if (np.abs(aq) > 2 ** 24).any() or (np.abs(bq) > 2 ** 31 - 2 ** 24).any() or (sq > 65535).any():
        raise ValueError('AugmentParams: alpha beyond 256, beta beyond 127 or sigma beyond 1023.98')
    arr = (_lib.AugmentFrameC * B)()
    for b in range(B):
        f = arr[b]
        if lib.rtm3d_augment_geometry(ctypes.byref(geom[b]), float(params.scale[b]), float(params.offset[b, 0]), float(params.offset[b, 1]),
                                      int(params.flip[b]), ctypes.byref(f)) != 0:
            raise ValueError('frame %d: %s' % (b, lib.rtm3d_last_error().decode()))
        f.alpha_q, f.beta_q, f.sigma_q = int(aq[b]), int(bq[b]), int(sq[b])
        f.seed_lo, f.seed_hi = int(params.seed[b]) & 0xFFFFFFFF, int(params.seed[b]) >> 32
        f.fill[0], f.fill[1], f.fill[2] = (int(v) for v in params.fill[b])
    return arr, geom


def plan(desc, size, mode=0, border=0):
    """rtm3d_frames_augment_plan: the launch schedule, one AugmentPlan per chunk of 32 frames (host only)."""
    return _frames.chunk_plans('frames_augment_plan', _lib.AugmentPlan, desc, int(mode), int(size[0]), int(size[1]), int(border))


def noise_table():
    """rtm3d_augment_noise_table: the 4096 int16 of T (host)."""
    T = np.zeros(4096, np.int16)
    _lib.check(_lib.load().rtm3d_augment_noise_table(T.ctypes.data_as(ctypes.c_void_p)), 'augment_noise_table')
    return T


_TABLES = {}


def device_noise_table(dev):
    """T on the device, once per device."""
    import torch
    hit = _TABLES.get(dev.index)
    if hit is None:
        with torch.cuda.device(dev):
            hit = torch.as_tensor(noise_table(), device=dev)
        _TABLES[dev.index] = hit
    return hit


def frames(images, params, size, mean, std, resize_to=None, out=None, model=None, mode=None, heads='dense', head_precision=None):
    """rtm3d_frames_augment: images = list of uint8 (h, w, 3) CUDA tensors of any sizes, params = AugmentParams, size = (H, W)
    network canvas, resize_to as in ``preprocess_batch``.  mode 'fp32' (the default without a model): the fp32 (B, 3, H, W)
    batch; 'nhwc4' (the default with ``model``): straight into that model's fp16 NHWC4 input tensor - call
    ``model.forward_logits(None, preloaded=(B, H, W), heads=heads)`` next; 'uint8': the (B, H, W, 3) uint8 canvases.
    Returns (out or None, [(pad_w, pad_h)], [(h', w')]) - what ``preprocess_batch`` returns."""
    import torch
    lib = _lib.load()
    H, W = int(size[0]), int(size[1])
    if not images:
        raise ValueError('no images')
    dev = images[0].device
    if dev.type != 'cuda':
        raise RuntimeError('rtm3d_amd.augment needs CUDA (ROCm) tensors; there is no CPU path')
    imgs = _frames.packed_frames(images, 'expected uint8 (h, w, 3) images on one device', dev)
    B = len(imgs)
    if mode is None:
        mode = 'nhwc4' if model is not None else 'fp32'
    mode = MODES[mode] if mode in MODES else int(mode)
    if mode not in (0, 1, 2):
        raise ValueError('mode: one of %s' % sorted(MODES))
    if (mode == 1) != (model is not None):
        raise ValueError("mode 'nhwc4' writes a model's input tensor: pass model=... with it, and only with it")
    desc, geom = descriptors([[int(i.shape[0]), int(i.shape[1])] for i in imgs], params, (H, W), resize_to)
    d_lut, d_lut16 = device_luts(mean, std, dev)
    with torch.cuda.device(dev):
        table = device_noise_table(dev)
        sums = torch.empty(B, 3, dtype=torch.int64, device=dev)
        if mode == 1:
            dst, border = model.input_tensor(B, H, W, dev, heads, head_precision)
            ret = None
        else:
            shape, dt = ((B, 3, H, W), torch.float32) if mode == 0 else ((B, H, W, 3), torch.uint8)
            if out is None:
                out = torch.empty(shape, dtype=dt, device=dev)
            if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dt or out.device != dev or not out.is_contiguous():
                raise ValueError('out must be a contiguous %s tensor of shape %s on %s' % (dt, shape, dev))
            dst, border, ret = out.data_ptr(), 0, out
        _lib.check(lib.rtm3d_frames_augment(_lib.stream_ptr(dev), B, _lib.ptr_array(imgs), desc, ctypes.c_void_p(dst), mode, H, W, border,
                                            table.data_ptr(), d_lut.data_ptr(), d_lut16.data_ptr(), sums.data_ptr()), 'frames_augment')
    return ret, [(g.pad_w, g.pad_h) for g in geom], [(g.rh, g.rw) for g in geom]


# ------------------------------------------------------------------------------------------------ labels (host, fp64)
def _label_frames(rows_per_image):
    from . import kitti_eval
    if isinstance(rows_per_image, kitti_eval.Labels):
        return rows_per_image
    frames_ = []
    for rows in rows_per_image:
        fr = []
        for r in rows:
            r = list(r)
            if len(r) not in (15, 16):
                raise ValueError('augment.labels: a label row has 15 fields (16 with a score), got %d: %r' % (len(r), r))
            fr.append([str(r[0])] + [float(v) for v in r[1:]] + ([0.0] if len(r) == 15 else []))
        frames_.append(fr)
    return kitti_eval._frames_to_labels(list(range(len(frames_))), frames_)


def labels(rows_per_image, K_per_image, hw, params, size, resize_to=None, cfg=None, mask_3d=None):
    """The labels of ``frames(images, params, size, ..., resize_to)``: KITTI rows (as ``LabelBatch.from_kitti`` takes them) and
    the ORIGINAL frames' camera matrices -> LabelBatch in the pixels of the canvas.  fp64, the reference's chain operation by
    operation:
      1. the class mapping of ``from_kitti`` (dataset_reader.py:197-213);
      2. RemoveBadBBox: a box with w <= 2 or h <= 2 in original pixels goes;
      3. ToPercentCoords, Resize, ToAbsoluteCoords on bbox and K: divide by (w, h), then multiply by (w', h');
      4. RandomAffine: bbox and the first two rows of K times scale, plus the offset; then its centre-outside mask, which the
         reference applies whether or not the affine fired (scale 1 and offset 0 leave every number as it is);
      5. RandomMirror: bbox x = w' - x with x1 and x2 swapped, K[2] = w' - K[2] - 1 (the reference's own inconsistency, kept),
         Ry -> -Ry + pi (Ry >= 0) or -Ry - pi, location x -> -x;
      6. the shift of _apply_padding.
    A removed or masked object becomes cls = -1 (every loss term needs ``mask``, so a masked row and a deleted row are alike);
    nothing is compacted, the rows stay those of ``from_kitti``.  ``alpha`` is not a LabelBatch field.  mask_3d: None (derived
    on the device from the moved labels) or per image one 0 / 1 per label row."""
    _check_gaussian_type(cfg)
    lab = _label_frames(rows_per_image)
    B = len(lab)
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    K = np.array(K_per_image, np.float64)
    if K.size != B * 9 or len(hw) != B or len(params) != B:
        raise ValueError('augment.labels: %d label frames, K of shape %s, %d sizes, %d parameter sets' % (B, K.shape, len(hw), len(params)))
    K = K.reshape(B, 9).copy()
    H, W = int(size[0]), int(size[1])
    objs, rel = list(cfg_get(cfg, 'DATASET', 'OBJs')), [list(r) for r in cfg_get(cfg, 'DATASET', 'RELATE_OBJs')]
    img_id, cls_, noise_, bbox_, dim_, loc_, ry_, m3_ = [], [], [], [], [], [], [], []
    for b in range(B):
        n = int(lab.n[b])
        cls, noise, rep = transform_obj_label([str(t) for t in lab.type[b, :n]], objs, rel)
        idx = np.repeat(np.arange(n), rep)
        bbox = np.array(lab.rect[b, idx], np.float64).reshape(-1, 4)
        loc = np.array(lab.xyz[b, idx], np.float64).reshape(-1, 3)
        ry = np.array(lab.ry[b, idx], np.float64).reshape(-1)
        Kb = K[b]
        mask = cls != -1
        h, w = int(hw[b, 0]), int(hw[b, 1])
        rh, rw = resized_size(h, w, resize_to) if resize_to else (h, w)
        scale, off = float(params.scale[b]), params.offset[b]
        # 2. RemoveBadBBox
        mask &= ~(((bbox[:, 2] - bbox[:, 0]) <= 2) | ((bbox[:, 3] - bbox[:, 1]) <= 2))
        # 3. ToPercentCoords -> Resize -> ToAbsoluteCoords
        bbox[:, 0::2] /= w; bbox[:, 1::2] /= h
        Kb[:3] /= w; Kb[3:6] /= h
        bbox[:, 0::2] *= rw; bbox[:, 1::2] *= rh
        Kb[:3] *= rw; Kb[3:6] *= rh
        # 4. RandomAffine
        bbox *= scale
        bbox[:, 0::2] += off[0]; bbox[:, 1::2] += off[1]
        Kb[:3] *= scale; Kb[3:6] *= scale
        Kb[2] += off[0]; Kb[5] += off[1]
        cx, cy = (bbox[:, 0] + bbox[:, 2]) / 2, (bbox[:, 1] + bbox[:, 3]) / 2
        mask &= ~((cx < 0) | (cx >= rw) | (cy < 0) | (cy >= rh))
        # 5. RandomMirror
        if params.flip[b]:
            bbox[:, 0::2] = rw - bbox[:, [2, 0]]
            Kb[2] = rw - Kb[2] - 1
            pos = ry >= 0
            ry = np.where(pos, -1. * ry + np.pi, -1. * ry - np.pi)
            loc[:, 0] *= -1
        # 6. _apply_padding
        pad_w, pad_h = (W - rw) // 2, (H - rh) // 2
        if pad_w < 0 or pad_h < 0:
            raise ValueError('augment.labels: frame %d (%d x %d after Resize) does not fit the %d x %d canvas' % (b, rh, rw, H, W))
        bbox[:, 0::2] += pad_w; bbox[:, 1::2] += pad_h
        Kb[2] += pad_w; Kb[5] += pad_h
        img_id.append(np.full(len(idx), b)); cls_.append(np.where(mask, cls, -1)); noise_.append(noise); bbox_.append(bbox)
        dim_.append(lab.hwl[b, idx]); loc_.append(loc); ry_.append(ry)
        if mask_3d is not None:
            m = np.asarray(mask_3d[b], np.float64).reshape(-1)
            if m.size != n:
                raise ValueError('augment.labels: mask_3d of image %d holds %d values for %d rows' % (b, m.size, n))
            m3_.append(m[idx])
    cat = lambda parts, tail: np.concatenate(parts).reshape((-1,) + tail) if parts else np.zeros((0,) + tail)
    return LabelBatch(B, cat(img_id, ()), cat(cls_, ()), cat(noise_, ()), cat(bbox_, (4,)), cat(dim_, (3,)), cat(loc_, (3,)), cat(ry_, ()),
                      K, mask_3d=cat(m3_, ()) if mask_3d is not None else None, num_classes=len(objs),
                      down_sample=cfg_get(cfg, 'MODEL', 'DOWN_SAMPLE'))


class TrainAugmentation:
    """The facade: ``aug = TrainAugmentation(cfg_or_size, mean, std, rng=...)``, then per step
    ``inp, batch, params = aug(images, rows_per_image, K_per_image, model=None)``.  cfg_or_size: a config tree - the canvas is
    the reference's square of INPUT_SIZE[0] and Resize takes the longest side to it - or an (H, W) canvas, with ``resize_to``
    (default: its longer side; 0: no Resize).  With ``model`` the pixels go straight into that model's input tensor (inp is
    None; ``model.forward_logits(None, preloaded=(B, H, W))`` follows); without it inp is the fp32 (B, 3, H, W) batch, the input
    of a torch model.  ``draw`` carries keyword overrides of ``AugmentParams.draw``."""

    def __init__(self, cfg_or_size, mean, std, rng=None, resize_to=None, cfg=None, **draw):
        if isinstance(cfg_or_size, (tuple, list)):
            self.size = (int(cfg_or_size[0]), int(cfg_or_size[1]))
            self.cfg = cfg
        else:
            side = int(cfg_or_size.INPUT_SIZE[0])
            self.size, self.cfg = (side, side), cfg_or_size
        self.resize_to = max(self.size) if resize_to is None else (int(resize_to) or None)
        self.mean, self.std = mean, std
        self.rng = rng if rng is not None else np.random.default_rng()
        self.draw = draw

    def __call__(self, images, rows_per_image, K_per_image, model=None, mask_3d=None, params=None):
        hw = [[int(i.shape[0]), int(i.shape[1])] for i in images]
        if params is None:
            params = AugmentParams.draw(len(hw), hw, self.resize_to, self.rng, **self.draw)
        inp, _, _ = frames(images, params, self.size, self.mean, self.std, resize_to=self.resize_to, model=model)
        batch = labels(rows_per_image, K_per_image, hw, params, self.size, self.resize_to, cfg=self.cfg, mask_3d=mask_3d)
        return inp, batch, params
