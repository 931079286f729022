"""Raw sensor frames (include/rtm3d_hip.h, "raw sensor frames"): the Bayer mosaics that GMSL / CSI-2 automotive and
machine-vision sensors deliver - bytes, uint16, MIPI RAW10 / RAW12, any RGGB-family pattern - become the tightly packed uint8
(h, w, 3) frames that Engine.detect_frames, lens.remap, preprocess_batch and the drawing entry points read: black level,
white balance, demosaic (Malvar-He-Cutler or bilinear), colour matrix and tone table in one launch per 32 frames
(rtm3d_frames_demosaic), stream-ordered, no host synchronisation.  The integer rule is written out in the header;
tests/raw_ref.py restates it in numpy."""
import ctypes

import numpy as np

from . import _frames, _lib
from ._frames import CHUNK, lookup as _lookup  # noqa: F401  (names the tests and the engine use)

LAYOUTS = {'u8': 0, 'u16': 1, 'u16_msb': 2, 'mipi10': 3, 'mipi12': 4}
_ALIASES = {'raw8': 'u8', 'raw16': 'u16', 'raw10': 'mipi10', 'raw12': 'mipi12'}
# the bits a layout takes; the first is its default
LAYOUT_BITS = {'u8': (8,), 'u16': (16, 14, 12, 10), 'u16_msb': (16, 14, 12, 10), 'mipi10': (10,), 'mipi12': (12,)}
PATTERNS = {'rggb': 0, 'bggr': 1, 'grbg': 2, 'gbrg': 3}
# colour (0 R, 1 G, 2 B) of cells k = (y & 1) * 2 + (x & 1) = 0, 1, 2, 3
PATTERN_CELLS = {'rggb': (0, 1, 1, 2), 'bggr': (2, 1, 1, 0), 'grbg': (1, 0, 2, 1), 'gbrg': (1, 2, 0, 1)}
METHODS = {'mhc': 0, 'bilinear': 1}
ORDERS = {'rgb': 0, 'bgr': 1}
TONE_SIZE = 4096
MAX_GAIN, MAX_CCM = 16384, 8192


def layout_id(layout):
    """'mipi10' | 'u16' | ... | RTM3D_RAW_* number -> the number; ValueError for anything else."""
    v = _lookup(LAYOUTS, layout, 'layout', _ALIASES)
    if v not in LAYOUTS.values():
        raise ValueError('unknown layout %r' % (layout,))
    return v


def _layout_name(lid):
    return [k for k, v in LAYOUTS.items() if v == lid][0]


def layout(layout, bits, h, w):
    """rtm3d_raw_src_layout: (row bytes = least pitch, rows) of the plane of ``layout`` at ``bits`` and ``h`` x ``w`` (host
    only)."""
    pitch, rows = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().rtm3d_raw_src_layout(layout_id(layout), int(bits), int(h), int(w), ctypes.byref(pitch), ctypes.byref(rows)),
               'raw_src_layout')
    return pitch.value, rows.value


_plane_layout = layout                   # (RawSource takes ``layout`` as a parameter name)


def q10(v):
    """Float -> Q10 with round-half-up (1024 is 1.0)."""
    return int(np.floor(float(v) * 1024.0 + 0.5))


def tone_table(kind='srgb'):
    """A tone table for RawSource(tone=): uint8 tensor of 4096 on the CPU (move it to the device once per camera).
    'linear': t >> 4, what a source without a table gets; 'srgb': the sRGB transfer curve; a float g: the power law
    (t / 4095) ** (1 / g).  numpy only - the library takes tables as plain data and builds none."""
    import torch
    t = np.arange(TONE_SIZE, dtype=np.float64)
    if isinstance(kind, str):
        if kind == 'linear':
            return torch.from_numpy((np.arange(TONE_SIZE) >> 4).astype(np.uint8))
        if kind != 'srgb':
            raise ValueError("tone_table: 'linear', 'srgb' or a gamma, got %r" % (kind,))
        u = t / 4095.0
        v = np.where(u <= 0.0031308, 12.92 * u, 1.055 * np.power(u, 1.0 / 2.4) - 0.055)
    else:
        g = float(kind)
        if not g > 0:
            raise ValueError('tone_table: a gamma is positive, got %r' % (kind,))
        v = np.power(t / 4095.0, 1.0 / g)
    return torch.from_numpy(np.clip(np.floor(v * 255.0 + 0.5), 0, 255).astype(np.uint8))


def cell_params(pattern, bits, black=0, gains=1.0, ccm=None):
    """What RawSource makes of its numbers: (black[4], gain[4] in Q10, ccm[9] in Q10) as the descriptor carries them, per cell
    k = (y & 1) * 2 + (x & 1).  black: a scalar or one per cell; gains: a scalar, (r, g, b) or one per cell; ccm: None (the
    identity) or 3 x 3.  Floats become Q10 with round-half-up.  ValueError for what the library would refuse."""
    pid = _lookup(PATTERNS, pattern, 'pattern')
    if pid not in PATTERNS.values():
        raise ValueError('unknown pattern %r' % (pattern,))
    cells = PATTERN_CELLS[[k for k, v in PATTERNS.items() if v == pid][0]]
    M = (1 << int(bits)) - 1
    b = np.atleast_1d(np.asarray(black, dtype=np.int64))
    if b.shape not in ((1,), (4,)):
        raise ValueError('black: a scalar or one per cell, got shape %s' % (b.shape,))
    black = [int(v) for v in np.broadcast_to(b, (4,))]
    if any(v < 0 or v > M for v in black):
        raise ValueError('black: %s outside 0..%d' % (black, M))
    g = np.atleast_1d(np.asarray(gains, dtype=np.float64))
    if g.shape == (3,):
        g = g[list(cells)]
    elif g.shape not in ((1,), (4,)):
        raise ValueError('gains: a scalar, (r, g, b) or one per cell, got shape %s' % (g.shape,))
    gain = [q10(v) for v in np.broadcast_to(g, (4,))]
    if any(v < 0 or v > MAX_GAIN for v in gain):
        raise ValueError('gains: Q10 values %s outside 0..%d (a gain is at most 16.0)' % (gain, MAX_GAIN))
    c = np.eye(3) if ccm is None else np.asarray(ccm, dtype=np.float64)
    if c.size != 9:
        raise ValueError('ccm: 3 x 3 numbers, got shape %s' % (c.shape,))
    ccm = [q10(v) for v in c.reshape(-1)]
    if any(abs(v) > MAX_CCM for v in ccm):
        raise ValueError('ccm: Q10 values %s outside +-%d (an entry is at most 8.0 in magnitude)' % (ccm, MAX_CCM))
    return black, gain, ccm


class RawSource(object):
    """One raw frame as a sensor, a deserialiser or a CSI-2 receiver left it on the device.

    plane: the CUDA tensor of its samples, uint8 (for 'u16' / 'u16_msb' uint16, int16 or uint8).  A 2-D tensor whose last
    dimension is contiguous gives its own pitch (``stride(0)`` in bytes) and, for 'u8' and the uint16 layouts, its size; a 1-D
    tensor is a raw buffer and needs ``size`` and ``pitch``, and so does a MIPI plane of a width that does not fill its last group.
    layout: 'u8' 'u16' 'u16_msb' 'mipi10' 'mipi12' (or RTM3D_RAW_*).  pattern: 'rggb' 'bggr' 'grbg' 'gbrg' (or RTM3D_CFA_*).
    bits: None = the layout's default (8, 16, 16, 10, 12).  size: (h, w).  pitch: bytes per row.
    black: the black level in sample units, a scalar or one per cell k = (y & 1) * 2 + (x & 1).
    gains: white balance, floats (converted to Q10, round half up): a scalar, (r, g, b), or one per cell.
    ccm: None (identity) or 3 x 3 floats, row-major, rows R G B of the output.
    tone: None (t >> 4) or a uint8 CUDA tensor of 4096 (tone_table), which frames of one camera share."""

    def __init__(self, plane, layout, pattern, bits=None, size=None, pitch=None, black=0, gains=1.0, ccm=None, tone=None):
        import torch
        self.layout = layout_id(layout)
        name = _layout_name(self.layout)
        self.pattern = _lookup(PATTERNS, pattern, 'pattern')
        if self.pattern not in PATTERNS.values():
            raise ValueError('unknown pattern %r' % (pattern,))
        self.bits = LAYOUT_BITS[name][0] if bits is None else int(bits)
        if self.bits not in LAYOUT_BITS[name]:
            raise ValueError('layout %s takes %s bits, got %d' % (name, ' / '.join(str(b) for b in LAYOUT_BITS[name]), self.bits))
        self.black, self.gain, self.ccm = cell_params(self.pattern, self.bits, black, gains, ccm)
        wide = name in ('u16', 'u16_msb')
        ok = isinstance(plane, torch.Tensor) and plane.is_cuda and 1 <= plane.dim() <= 2 and \
            (plane.dtype == torch.uint8 or (wide and plane.dtype in (torch.uint16, torch.int16)))
        if not ok:
            raise ValueError('plane: expected a uint8 (u16 layouts: uint16, int16 or uint8) CUDA tensor of 1 or 2 dimensions')
        es = plane.element_size()
        own = _frames.plane_pitch(plane, 'plane')
        if size is None:
            if plane.dim() == 1 or name in ('mipi10', 'mipi12'):
                raise ValueError('a 1-D plane or a MIPI plane does not tell its size: give size=(h, w)')
            row = int(plane.shape[1]) * es
            bps = 2 if wide else 1
            if row % bps:
                raise ValueError('plane has rows of %d bytes, no multiple of %d' % (row, bps))
            size = (int(plane.shape[0]), row // bps)
        self.h, self.w = int(size[0]), int(size[1])
        if pitch is None:
            if own is None:
                raise ValueError('a 1-D plane is a raw buffer: give pitch=')
            pitch = own
        self.pitch = int(pitch)
        self.plane = plane
        if tone is not None:
            if not isinstance(tone, torch.Tensor) or tone.dtype != torch.uint8 or not tone.is_cuda or tone.dim() != 1 \
                    or tone.numel() != TONE_SIZE or not tone.is_contiguous() or tone.device != plane.device:
                raise ValueError('tone: a contiguous uint8 CUDA tensor of %d on the plane\'s device' % TONE_SIZE)
        self.tone = tone
        row, rows = _plane_layout(self.layout, self.bits, self.h, self.w)
        _frames.check_plane_covers(plane, self.pitch, row, rows, 'plane', 'layout')

    @property
    def device(self):
        return self.plane.device

    def c_struct(self):
        s = _lib.RawSrc()
        s.plane, s.d_tone = self.plane.data_ptr(), (None if self.tone is None else self.tone.data_ptr())
        s.pitch, s.h, s.w = self.pitch, self.h, self.w
        s.layout, s.bits, s.pattern, s.reserved, s.pad = self.layout, self.bits, self.pattern, 0, 0
        for k in range(4):
            s.black[k], s.gain[k] = self.black[k], self.gain[k]
        for k in range(9):
            s.ccm[k] = self.ccm[k]
        return s


def c_sources(sources):
    """list of RawSource -> ctypes array of rtm3d_raw_src."""
    return _frames.struct_array(_lib.RawSrc, sources, RawSource)


def plan(sources, method='mhc'):
    """rtm3d_frames_demosaic_plan: the launch schedule of demosaic(sources), one DemosaicPlan per chunk of 32 frames (host only;
    ``sources``: RawSource list or a ctypes array of RawSrc)."""
    arr = sources if isinstance(sources, ctypes.Array) else c_sources(sources)
    return _frames.chunk_plans('frames_demosaic_plan', _lib.DemosaicPlan, arr, _lookup(METHODS, method, 'method'))


def packed_buffers(sources, out=None):
    """The destination frames of a demosaic: ``out`` checked (uint8 contiguous CUDA (h, w, 3) per source), or new tensors."""
    from . import pixfmt
    return pixfmt.packed_buffers(sources, out)


def demosaic(sources, method='mhc', order='rgb', out=None):
    """rtm3d_frames_demosaic: list of RawSource -> list of packed uint8 (h, w, 3) CUDA tensors (``out``, or new ones).
    method: 'mhc' (Malvar-He-Cutler, 5 x 5) | 'bilinear'.  order: 'rgb' | 'bgr', the byte order of a written pixel - the
    channel order the checkpoint was trained on, which the library cannot know."""
    import torch
    sources = list(sources)
    src = c_sources(sources)
    dev = sources[0].device
    with torch.cuda.device(dev):
        out = packed_buffers(sources, out)
        _lib.check(_lib.load().rtm3d_frames_demosaic(_lib.stream_ptr(dev), len(out), src, _lib.ptr_array(out),
                                                     _lookup(METHODS, method, 'method'), _lookup(ORDERS, order, 'order')), 'frames_demosaic')
    return out
