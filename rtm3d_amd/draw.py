"""Detection records painted into the camera frames and a bird's-eye panel on the device (csrc/draw.hip).

The drawing rule - integer coordinates by truncation, exact integer coverage tests, painter's order with slot 0 on top - is
stated in include/rtm3d_hip.h, "drawing"; the result is defined bit for bit.  ``draw_records`` paints a list of uint8
(h, w, 3) CUDA frames IN PLACE from the (B, topk, 32) records of ``Engine.detect_frames`` (one launch on the current stream);
``draw_tracks`` (rtm3d_records_draw_tracks; the header's "drawing tracks") does the same with the ids of a ``track.Tracker``: a
stable colour per track id, a text label per slot, and a bird's-eye panel painted from the tracker's table.
``to_ppm`` writes a frame or panel as binary PPM, so looking at a result needs neither OpenCV nor an image library.
Device tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _frames, _lib

FACE, BOX2D, WIREFRAME, KEYPOINT, BEV = 1, 2, 4, 8, 16
LABEL, TRACK_BEV = 32, 64
FRAME_LAYERS = FACE | BOX2D | WIREFRAME | KEYPOINT
LABEL_ID, LABEL_CLASS, LABEL_SCORE, LABEL_DISTANCE = 1, 2, 4, 8        # bits of TrackDrawParams.label_fields
MAX_CLASSES = 16
# the default palette (RGB; the channel order of the frames is the caller's): eight well separated hues, repeated
PALETTE = ((255, 64, 64), (64, 224, 64), (64, 128, 255), (255, 208, 0), (255, 64, 224), (0, 224, 224), (255, 144, 32), (176, 112, 255))


class DrawParams(object):
    """The fields of struct rtm3d_draw_params.  layers: mask of FACE | BOX2D | WIREFRAME | KEYPOINT | BEV; source: 0 = the
    regressed vertices, 1 = the solved box projected through K_camera; min_flag: 1 = every detection, 2 = 3D-kept only;
    thickness 1..15; radius of the key-point disc; face_alpha 0..256; colors: up to 16 triples indexed by class; bev_hw,
    bev_m_per_px: size and scale of the bird's-eye panels."""

    def __init__(self, layers=FRAME_LAYERS, source=0, min_flag=1, thickness=1, radius=5, face_alpha=77, colors=None, bev_hw=(400, 400),
                 bev_m_per_px=0.2):
        self.layers, self.source, self.min_flag, self.thickness = int(layers), int(source), int(min_flag), int(thickness)
        self.radius, self.face_alpha = int(radius), int(face_alpha)
        self.colors = [tuple(int(v) for v in c) for c in (colors if colors is not None else [PALETTE[i % 8] for i in range(MAX_CLASSES)])]
        self.bev_hw, self.bev_m_per_px = (int(bev_hw[0]), int(bev_hw[1])), float(bev_m_per_px)

    def to_c(self):
        if not 1 <= len(self.colors) <= MAX_CLASSES or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in self.colors):
            raise ValueError('DrawParams: colors must be 1..%d triples of 0..255, got %r' % (MAX_CLASSES, self.colors))
        p = _lib.DrawParamsC()
        p.layers, p.source, p.min_flag, p.thickness, p.radius = self.layers, self.source, self.min_flag, self.thickness, self.radius
        p.face_alpha, p.ncls = self.face_alpha, len(self.colors)
        for i, c in enumerate(self.colors):
            for k in range(3):
                p.color[i][k] = c[k]
        if self.layers & BEV:
            p.bev_h, p.bev_w, p.bev_m_per_px = self.bev_hw[0], self.bev_hw[1], self.bev_m_per_px
        return p


def draw_records(images, rec, K_camera=None, params=None, bev=None, check_classes=True):
    """Paint the records into ``images`` IN PLACE (rtm3d_records_draw on the current stream).  images: list of B contiguous
    uint8 (h, w, 3) CUDA tensors; rec: contiguous fp32 (B, topk, 32) CUDA records in the pixels of each frame; K_camera:
    (B, 9) camera intrinsics, needed by params.source == 1; params: DrawParams (None: the defaults).  With the BEV layer set
    the panels are painted as well and returned: ``bev`` = a contiguous uint8 (B, bev_h, bev_w, 3) CUDA tensor painted in
    place, or None for new black panels.  check_classes: compare the classes of the live slots with the colour table on the
    host (one synchronisation) and raise ValueError for one outside it; False: no synchronisation, such a slot is not drawn.
    Returns the panels, or None without the BEV layer."""
    params = DrawParams() if params is None else params
    _check_frames('draw_records', images, rec)
    B, topk, dev = int(rec.shape[0]), int(rec.shape[1]), rec.device
    p = params.to_c()
    if check_classes:
        live = rec[..., 31] >= float(params.min_flag)
        bad = live & ~((rec[..., 0] >= 0) & (rec[..., 0] < p.ncls))
        if bool(bad.any()):
            raise ValueError('draw_records: a record has a class outside the colour table of %d classes' % p.ncls)
    K = None
    if K_camera is not None:
        K = torch.as_tensor(K_camera, dtype=torch.float64, device=dev).reshape(B, 9).contiguous()
    with torch.cuda.device(dev):
        panels = None
        if params.layers & BEV:
            shape = (B, params.bev_hw[0], params.bev_hw[1], 3)
            if bev is None:
                panels = torch.zeros(shape, dtype=torch.uint8, device=dev)
            elif not isinstance(bev, torch.Tensor) or bev.dtype != torch.uint8 or tuple(bev.shape) != shape or not bev.is_contiguous() \
                    or bev.device != dev:
                raise ValueError('draw_records: bev must be a contiguous uint8 tensor %s on %s' % (shape, dev))
            else:
                panels = bev
        _lib.check(_lib.load().rtm3d_records_draw(_lib.stream_ptr(dev), B, topk, rec.data_ptr(), _lib.ptr_array(images), _lib.hw_array(images),
                                                  K.data_ptr() if K is not None else None, ctypes.byref(p),
                                                  panels.data_ptr() if panels is not None else None), 'records_draw')
    return panels


class TrackDrawParams(DrawParams):
    """DrawParams plus the fields of struct rtm3d_draw_tracks_params.  layers may carry LABEL and TRACK_BEV (instead of BEV).
    palette: 1..32 RGB triples indexed by (|id| - 1) % len (None: the library's 32); label_fields: mask of LABEL_ID | LABEL_CLASS |
    LABEL_SCORE | LABEL_DISTANCE; font_scale 1..4; names: class names (None: the KITTI classes of the config), at most 7
    characters of each are drawn; bev_fade 0..256 (256 = off): the panels fade by this factor before they are painted;
    vel_horizon: length of the velocity mark in units of dt, 0 = none."""

    def __init__(self, palette=None, label_fields=LABEL_ID | LABEL_CLASS, font_scale=1, names=None, bev_fade=256, vel_horizon=1.0, **kw):
        DrawParams.__init__(self, **kw)
        if names is None:
            from .config import kitti_config
            names = kitti_config().DATASET.OBJs
        self.palette = None if palette is None else [tuple(int(v) for v in c) for c in palette]
        self.label_fields, self.font_scale, self.bev_fade, self.vel_horizon = int(label_fields), int(font_scale), int(bev_fade), float(vel_horizon)
        self.names = [n if isinstance(n, bytes) else str(n).encode('latin-1', 'replace') for n in names]

    def to_c(self):
        q = _lib.DrawTracksParamsC()
        _lib.check(_lib.load().rtm3d_draw_tracks_default_params(ctypes.byref(q)), 'draw_tracks_default_params')
        q.base = DrawParams.to_c(self)
        if self.layers & (BEV | TRACK_BEV):
            q.base.bev_h, q.base.bev_w, q.base.bev_m_per_px = self.bev_hw[0], self.bev_hw[1], self.bev_m_per_px
        if self.palette is not None:
            if not 1 <= len(self.palette) <= 32 or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in self.palette):
                raise ValueError('TrackDrawParams: palette must be 1..32 triples of 0..255, got %r' % (self.palette,))
            q.npal = len(self.palette)
            for i, c in enumerate(self.palette):
                for k in range(3):
                    q.palette[i][k] = c[k]
        if len(self.names) > MAX_CLASSES:
            raise ValueError('TrackDrawParams: at most %d class names, got %d' % (MAX_CLASSES, len(self.names)))
        for i in range(MAX_CLASSES):
            q.names[i].value = self.names[i][:7] if i < len(self.names) else b''
        q.label_fields, q.font_scale, q.bev_fade, q.vel_horizon = self.label_fields, self.font_scale, self.bev_fade, self.vel_horizon
        return q


def _check_frames(who, images, rec):
    if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
        raise RuntimeError('rtm3d_amd.draw.%s needs CUDA (ROCm) tensors; there is no CPU path' % who)
    if rec.dtype != torch.float32 or rec.dim() != 3 or rec.shape[-1] != 32 or not rec.is_contiguous():
        raise ValueError('%s: rec must be a contiguous fp32 tensor (B, topk, 32), got %s %s' % (who, rec.dtype, tuple(rec.shape)))
    B, dev = int(rec.shape[0]), rec.device
    if len(images) != B:
        raise ValueError('%s: %d frames for the records of %d images' % (who, len(images), B))
    for i, img in enumerate(images):
        if not _frames.is_packed_frame(img, device=dev):
            raise ValueError('%s: frame %d must be a contiguous uint8 (h, w, 3) tensor on %s (it is painted in place)' % (who, i, dev))


def draw_tracks(images, rec, ids, K_camera=None, params=None, tracker=None, bev=None, check_classes=True):
    """draw_records with track ids (rtm3d_records_draw_tracks on the current stream).  images, rec, K_camera, bev, check_classes:
    as for draw_records.  ids: the contiguous (B, topk) int32 CUDA ids ``Tracker.update`` returned for ``rec``; a slot with an id
    takes the id's colour.  params: TrackDrawParams (None: the defaults).  tracker: the track.Tracker whose table the TRACK_BEV
    layer paints (needed with that layer only).  Returns the panels, or None without a panel layer."""
    params = TrackDrawParams() if params is None else params
    _check_frames('draw_tracks', images, rec)
    B, topk, dev = int(rec.shape[0]), int(rec.shape[1]), rec.device
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or tuple(ids.shape) != (B, topk) or not ids.is_contiguous() or ids.device != dev:
        raise ValueError('draw_tracks: ids must be a contiguous int32 tensor (%d, %d) on %s' % (B, topk, dev))
    T, state = 0, None
    if params.layers & TRACK_BEV:
        if tracker is None:
            raise ValueError('draw_tracks: the TRACK_BEV layer paints a tracker\'s table and needs tracker=')
        if tracker.B != B or tracker.device != dev:
            raise ValueError('draw_tracks: the tracker holds %d streams on %s, the records %d on %s' % (tracker.B, tracker.device, B, dev))
        T, state = tracker.capacity, tracker.state
    q = params.to_c()
    if check_classes:
        live = rec[..., 31] >= float(params.min_flag)
        bad = live & ~((rec[..., 0] >= 0) & (rec[..., 0] < q.base.ncls))
        if bool(bad.any()):
            raise ValueError('draw_tracks: a record has a class outside the colour table of %d classes' % q.base.ncls)
    K = None
    if K_camera is not None:
        K = torch.as_tensor(K_camera, dtype=torch.float64, device=dev).reshape(B, 9).contiguous()
    with torch.cuda.device(dev):
        panels = None
        if params.layers & (BEV | TRACK_BEV):
            shape = (B, params.bev_hw[0], params.bev_hw[1], 3)
            if bev is None:
                panels = torch.zeros(shape, dtype=torch.uint8, device=dev)
            elif not isinstance(bev, torch.Tensor) or bev.dtype != torch.uint8 or tuple(bev.shape) != shape or not bev.is_contiguous() \
                    or bev.device != dev:
                raise ValueError('draw_tracks: bev must be a contiguous uint8 tensor %s on %s' % (shape, dev))
            else:
                panels = bev
        _lib.check(_lib.load().rtm3d_records_draw_tracks(_lib.stream_ptr(dev), B, topk, rec.data_ptr(), ids.data_ptr(), T,
                                                         state.data_ptr() if state is not None else None, _lib.ptr_array(images),
                                                         _lib.hw_array(images), K.data_ptr() if K is not None else None, ctypes.byref(q),
                                                         panels.data_ptr() if panels is not None else None), 'records_draw_tracks')
    return panels


def label_text(params, track_id, cls, score, z):
    """The text rtm3d_records_draw_tracks writes for a kept slot (rtm3d_draw_label_text; host only)."""
    q = params.to_c()
    out = (ctypes.c_char * 32)()
    _lib.check(_lib.load().rtm3d_draw_label_text(ctypes.byref(q), int(track_id), int(cls), float(score), float(z), out), 'draw_label_text')
    return out.value.decode('ascii')


def to_ppm(path, image):
    """Write a uint8 (h, w, 3) tensor or array as binary PPM (P6), channels as they are."""
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else image
    if a.dtype.name != 'uint8' or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('to_ppm: a uint8 (h, w, 3) image, got %s %s' % (a.dtype, a.shape))
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())


def to_jpeg(path, image, quality=90, mode='420', order='rgb'):
    """Write a uint8 (h, w, 3) CUDA tensor as a baseline JPEG file through rtm3d_amd.jpeg.encode (device DCT, host Huffman coding;
    no image library).  order: the byte order of a pixel of ``image``."""
    from . import jpeg
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise ValueError('to_jpeg: a uint8 (h, w, 3) CUDA tensor (to_ppm writes host arrays)')
    jpeg.write_files([path], jpeg.encode([image.contiguous()], quality=quality, mode=mode, order=order))
