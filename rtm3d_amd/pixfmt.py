"""Camera frames in decoder and camera pixel formats (include/rtm3d_hip.h, "pixel formats"): pitched NV12 / NV21 / I420 /
P010 surfaces, YUYV / UYVY, GRAY8 and pitched RGB / BGR / RGBA / BGRA rows become the tightly packed uint8 (h, w, 3) frames
that Engine.detect_frames, preprocess_batch and the drawing entry points read - one launch per 32 frames
(rtm3d_frames_convert), stream-ordered, no host synchronisation.  The integer rule is written out in the header;
tests/pixfmt_ref.py restates it in numpy."""
import ctypes

from . import _frames, _lib
from ._frames import CHUNK, lookup as _lookup  # noqa: F401  (names the tests and the engine use)

FORMATS = {'rgb24': 0, 'bgr24': 1, 'rgba32': 2, 'bgra32': 3, 'gray8': 4, 'nv12': 5, 'nv21': 6, 'i420': 7, 'yuyv': 8, 'uyvy': 9,
           'p010': 10}
_ALIASES = {'rgb': 'rgb24', 'bgr': 'bgr24', 'rgba': 'rgba32', 'bgra': 'bgra32', 'gray': 'gray8', 'grey': 'gray8', 'yuy2': 'yuyv'}
MATRICES = {'bt601': 0, 'bt709': 1}
RANGES = {'limited': 0, 'full': 1}
ORDERS = {'rgb': 0, 'bgr': 1}


def format_id(format):
    """'nv12' | 'bgra' | ... | RTM3D_PIX_* number -> the number; ValueError for anything else."""
    if isinstance(format, str):
        name = format.lower()
        name = _ALIASES.get(name, name)
        if name not in FORMATS:
            raise ValueError('unknown pixel format %r (one of %s)' % (format, ', '.join(sorted(FORMATS))))
        return FORMATS[name]
    if int(format) not in FORMATS.values():
        raise ValueError('unknown pixel format %r' % (format,))
    return int(format)


def layout(format, h, w):
    """rtm3d_frame_src_layout: [(row bytes = least pitch, rows)] per plane of ``format`` at ``h`` x ``w`` (host only)."""
    n = ctypes.c_int()
    pitch, rows = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    _lib.check(_lib.load().rtm3d_frame_src_layout(format_id(format), int(h), int(w), ctypes.byref(n), pitch, rows), 'frame_src_layout')
    return [(pitch[i], rows[i]) for i in range(n.value)]


def yuv_coefficients(format, matrix='bt601', range='limited'):
    """rtm3d_yuv_coefficients: ([cy, crv, cgu, cgv, cbu], yo, chroma offset, S) the kernel uses (host only)."""
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.load().rtm3d_yuv_coefficients(format_id(format), _lookup(MATRICES, matrix, 'matrix'), _lookup(RANGES, range, 'range'),
                                                  out), 'yuv_coefficients')
    return list(out[:5]), out[5], out[6], out[7]


class FrameSource(object):
    """One frame as a decoder, camera or capture API left it on the device.

    planes: the CUDA tensors of its planes, uint8 (for P010 uint16 or uint8).  A plane tensor whose last dimension is
    contiguous gives its own pitch: ``stride(0)`` in bytes, so a view into a pitched surface (``surface[:h, :w]``) or into a
    larger frame needs nothing more; a 1-D tensor is a raw buffer and needs ``size`` and ``pitches``.
    format: 'rgb24' 'bgr24' 'rgba32' 'bgra32' 'gray8' 'nv12' 'nv21' 'i420' 'yuyv' 'uyvy' 'p010' (or RTM3D_PIX_*).
    size: (h, w); None reads it from plane 0 - (h, w) of a luma or grey plane, (h, w, c) or (h, w * c) of packed RGB, and
    for YUYV / UYVY twice the pairs of a row, so an odd width must be given.
    pitches: bytes per row of each plane; None = the tensors' strides.  matrix: 'bt601' | 'bt709', range: 'limited' | 'full'
    (ignored for RGB and grey)."""

    def __init__(self, planes, format, size=None, pitches=None, matrix='bt601', range='limited'):
        import torch
        self.format = format_id(format)
        self.matrix, self.range = _lookup(MATRICES, matrix, 'matrix'), _lookup(RANGES, range, 'range')
        planes = [planes] if isinstance(planes, torch.Tensor) else list(planes)
        if not 1 <= len(planes) <= 3:
            raise ValueError('a frame has one to three planes, got %d' % len(planes))
        own = []
        for i, t in enumerate(planes):
            ok = isinstance(t, torch.Tensor) and t.is_cuda and 1 <= t.dim() <= 3 and \
                (t.dtype == torch.uint8 or (self.format == FORMATS['p010'] and t.dtype == torch.uint16))
            if not ok:
                raise ValueError('plane %d: expected a uint8 (P010: uint16 or uint8) CUDA tensor of 1 to 3 dimensions' % i)
            own.append(_frames.plane_pitch(t, 'plane %d' % i))
        if size is None:
            p0 = planes[0]
            if p0.dim() == 1:
                raise ValueError('a 1-D plane is a raw buffer: give size=(h, w) and pitches=')
            h, row = int(p0.shape[0]), _frames.plane_row_bytes(p0)
            bpp = {0: 3, 1: 3, 2: 4, 3: 4, 4: 1, 5: 1, 6: 1, 7: 1, 8: 2, 9: 2, 10: 2}[self.format]
            if row % bpp:
                raise ValueError('plane 0 has rows of %d bytes, no multiple of %d' % (row, bpp))
            size = (h, row // bpp)
        self.h, self.w = int(size[0]), int(size[1])
        if pitches is None:
            if any(p is None for p in own):
                raise ValueError('a 1-D plane is a raw buffer: give pitches=')
            pitches = own
        pitches = [int(p) for p in pitches]
        if len(pitches) != len(planes):
            raise ValueError('%d pitches for %d planes' % (len(pitches), len(planes)))
        self.planes, self.pitches = planes, pitches
        need = layout(self.format, self.h, self.w)
        if len(need) != len(planes):
            raise ValueError('format %d has %d planes, got %d' % (self.format, len(need), len(planes)))
        for i, (t, (row, rows)) in enumerate(zip(planes, need)):
            _frames.check_plane_covers(t, pitches[i], row, rows, 'plane %d' % i, 'format')

    # ---- constructors by layout
    @classmethod
    def nv12(cls, y, uv, **kw):
        return cls([y, uv], 'nv12', **kw)

    @classmethod
    def nv21(cls, y, vu, **kw):
        return cls([y, vu], 'nv21', **kw)

    @classmethod
    def p010(cls, y, uv, **kw):
        return cls([y, uv], 'p010', **kw)

    @classmethod
    def i420(cls, y, u, v, **kw):
        return cls([y, u, v], 'i420', **kw)

    @classmethod
    def yuyv(cls, t, **kw):
        return cls([t], 'yuyv', **kw)

    @classmethod
    def uyvy(cls, t, **kw):
        return cls([t], 'uyvy', **kw)

    @classmethod
    def gray(cls, t, **kw):
        return cls([t], 'gray8', **kw)

    @classmethod
    def packed(cls, t, format='rgb', **kw):
        """Interleaved rows: format 'rgb' | 'bgr' | 'rgba' | 'bgra'."""
        return cls([t], format, **kw)

    @property
    def device(self):
        return self.planes[0].device

    def c_struct(self):
        s = _lib.FrameSrc()
        for i, (t, p) in enumerate(zip(self.planes, self.pitches)):
            s.plane[i], s.pitch[i] = t.data_ptr(), p
        s.h, s.w, s.format, s.matrix, s.range, s.reserved = self.h, self.w, self.format, self.matrix, self.range, 0
        return s


def c_sources(sources):
    """list of FrameSource -> ctypes array of rtm3d_frame_src."""
    return _frames.struct_array(_lib.FrameSrc, sources, FrameSource)


def plan(sources):
    """rtm3d_frames_convert_plan: the launch schedule of convert(sources), one ConvertPlan per chunk of 32 frames (host only;
    ``sources``: FrameSource list or a ctypes array of FrameSrc)."""
    arr = sources if isinstance(sources, ctypes.Array) else c_sources(sources)
    return _frames.chunk_plans('frames_convert_plan', _lib.ConvertPlan, arr)


def packed_buffers(sources, out=None):
    """The destination frames of a conversion: ``out`` checked (uint8 contiguous CUDA (h, w, 3) per source), or new tensors."""
    return _frames.packed_buffers([(s.h, s.w) for s in sources], [s.device for s in sources], out, 'source')


def convert(sources, order='rgb', out=None):
    """rtm3d_frames_convert: list of FrameSource -> list of packed uint8 (h, w, 3) CUDA tensors (``out``, or new ones).
    order: 'rgb' | 'bgr', the byte order of a written pixel - the channel order the checkpoint was trained on, which the
    library cannot know."""
    import torch
    sources = list(sources)
    src = c_sources(sources)
    dev = sources[0].device
    with torch.cuda.device(dev):
        out = packed_buffers(sources, out)
        _lib.check(_lib.load().rtm3d_frames_convert(_lib.stream_ptr(dev), len(out), src, _lib.ptr_array(out),
                                                    _lookup(ORDERS, order, 'order')), 'frames_convert')
    return out
