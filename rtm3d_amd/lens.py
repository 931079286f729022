"""Lens undistortion (include/rtm3d_hip.h, "lens undistortion"): rectifying maps built on the device from a Brown (rational)
or a fisheye (Kannala-Brandt) model (rtm3d_lens_map_build) and the bilinear remap of packed uint8 (h, w, 3) frames through
them (rtm3d_frames_remap) - one launch per 32 frames, stream-ordered, no host synchronisation.  A map is plain data (int32
source positions in 1/32 pixel), so one made elsewhere serves a lens model the builder does not cover (LensMap.from_array).
Both rules are written out in the header; tests/lens_ref.py restates them in numpy.  Parity with OpenCV's remap and
initUndistortRectifyMap is not claimed: OpenCV was not at hand to pin the restatement against."""
import ctypes

import numpy as np

from . import _frames, _lib
from ._frames import CHUNK  # noqa: F401  (a name the tests use)

KINDS = {'brown': 0, 'fisheye': 1}
OUTSIDE = -2 ** 31


def _k9(K, what='K'):
    K = np.asarray(K, np.float64)
    if K.size != 9:
        raise ValueError('%s: expected a 3 x 3 matrix, got shape %s' % (what, K.shape))
    return K.reshape(9).copy()


class LensModel(object):
    """The physical camera: kind 'brown' | 'fisheye', K its 3 x 3 intrinsics (no skew), dist its coefficients, size = (h, w)
    of its frames."""

    def __init__(self, kind, K, dist, size):
        if kind not in KINDS:
            raise ValueError('unknown lens kind %r (one of %s)' % (kind, ', '.join(sorted(KINDS))))
        self.kind, self.K = kind, _k9(K)
        d = np.asarray(dist, np.float64).reshape(-1)
        most = 8 if kind == 'brown' else 4
        if d.size > most:
            raise ValueError('a %s lens has at most %d coefficients, got %d' % (kind, most, d.size))
        self.dist = np.zeros(8, np.float64)
        self.dist[:d.size] = d
        self.h, self.w = int(size[0]), int(size[1])

    @classmethod
    def brown(cls, K, dist, size):
        """dist = k1 k2 p1 p2 [k3 [k4 k5 k6]] (OpenCV's order; the rational model when all eight are given)."""
        return cls('brown', K, dist, size)

    @classmethod
    def fisheye(cls, K, dist, size):
        """dist = k1 k2 k3 k4 of the equidistant model (theta_d = theta (1 + k1 theta^2 + ...))."""
        return cls('fisheye', K, dist, size)

    def c_struct(self):
        return _lib.LensModelC(KINDS[self.kind], self.h, self.w, (ctypes.c_double * 9)(*self.K), (ctypes.c_double * 8)(*self.dist))


class LensMap(object):
    """A rectifying map on the device: ``tensor`` (ho, wo, 2) int32 CUDA, contiguous, [..., 0] = sx and [..., 1] = sy in 1/32
    pixel of the source frame (sx == OUTSIDE: no source); ``K_rect`` the 9 intrinsics of the frames it makes (None when the
    map's maker did not say), ``size`` = (ho, wo)."""

    def __init__(self, tensor, K_rect=None):
        import torch
        if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.int32 or not tensor.is_cuda or tensor.dim() != 3 \
                or tensor.shape[2] != 2 or not tensor.is_contiguous():
            raise ValueError('a map is a contiguous int32 CUDA tensor of shape (ho, wo, 2)')
        self.tensor = tensor
        self.K_rect = None if K_rect is None else _k9(K_rect, 'K_rect')
        self.size = (int(tensor.shape[0]), int(tensor.shape[1]))

    @classmethod
    def from_array(cls, array, K_rect=None, device='cuda'):
        """A map made elsewhere: an integer (ho, wo, 2) array (numpy or torch) of (sx, sy) in 1/32 pixel - e.g. the float maps of
        another library times 32, rounded - uploaded as int32."""
        import torch
        if isinstance(array, torch.Tensor):
            if array.is_floating_point():
                raise ValueError('a map holds integers (positions in 1/32 pixel)')
            t = array.to(device=device, dtype=torch.int32)
        else:
            a = np.asarray(array)
            if a.dtype.kind not in 'iu' or (a.size and (a.min() < OUTSIDE or a.max() > 2 ** 31 - 1)):
                raise ValueError('a map holds int32 values (positions in 1/32 pixel)')
            t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(device)
        return cls(t.contiguous(), K_rect)

    @property
    def device(self):
        return self.tensor.device

    def c_struct(self):
        return _lib.LensMapC(self.tensor.data_ptr(), self.size[0], self.size[1], 0)


def _per_model(v, n, what, one):
    """None | one value | a list of n -> a list of n (``one(v)`` tells whether v is a single value)."""
    if v is None:
        return [None] * n
    if one(v):
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError('%d %s for %d lens models' % (len(v), what, n))
    return v


def build_maps(models, K_rect=None, R=None, out_size=None, device='cuda'):
    """rtm3d_lens_map_build: one LensMap per LensModel.  K_rect: the intrinsics of the rectified frames (3 x 3, one for all or a
    list; None: the lens's own K).  R: the rectifying rotation in OpenCV's sense - it takes a ray of the physical camera to a
    ray of the rectified one, what initUndistortRectifyMap is given (one for all or a list; None: the identity); the library
    takes the transpose.  out_size: (ho, wo) (one for all or a list; None: the lens's own size)."""
    import torch
    models = list(models)
    n = len(models)
    cm = _frames.struct_array(_lib.LensModelC, models, LensModel)
    Ks = _per_model(K_rect, n, 'K_rect', lambda v: np.asarray(v, np.float64).size == 9)
    Rs = _per_model(R, n, 'R', lambda v: np.asarray(v, np.float64).size == 9)
    sizes = _per_model(out_size, n, 'sizes', lambda v: len(v) == 2 and not hasattr(v[0], '__len__'))
    cr = (_lib.LensRectC * n)()
    dev = torch.device(device)
    dev = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
    maps = []
    with torch.cuda.device(dev):
        for i, m in enumerate(models):
            K = m.K if Ks[i] is None else _k9(Ks[i], 'K_rect')
            Rt = np.eye(3).reshape(9) if Rs[i] is None else np.ascontiguousarray(_k9(Rs[i], 'R').reshape(3, 3).T).reshape(9)
            ho, wo = (m.h, m.w) if sizes[i] is None else (int(sizes[i][0]), int(sizes[i][1]))
            cr[i] = _lib.LensRectC(ho, wo, (ctypes.c_double * 9)(*K), (ctypes.c_double * 9)(*Rt))
            if not (1 <= ho <= 16384 and 1 <= wo <= 16384):
                raise ValueError('map %d: a map of %d x %d; a side must lie in 1..16384' % (i, ho, wo))
            maps.append(LensMap(torch.empty(ho, wo, 2, dtype=torch.int32, device=dev), K))
        _lib.check(_lib.load().rtm3d_lens_map_build(_lib.stream_ptr(dev), n, cm, cr, _lib.ptr_array([m.tensor for m in maps])),
                   'lens_map_build')
    return maps


def c_maps(maps):
    """list of LensMap -> ctypes array of rtm3d_lens_map."""
    return _frames.struct_array(_lib.LensMapC, maps, LensMap)


def plan(maps):
    """rtm3d_frames_remap_plan: the launch schedule of remap(frames, maps), one RemapPlan per chunk of 32 frames (host only;
    ``maps``: LensMap list or a ctypes array of LensMapC)."""
    arr = maps if isinstance(maps, ctypes.Array) else c_maps(maps)
    return _frames.chunk_plans('frames_remap_plan', _lib.RemapPlan, arr)


def c_fill(fill):
    fill = [int(v) for v in fill]
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError('fill: three bytes, got %r' % (fill,))
    return (ctypes.c_uint8 * 3)(*fill)


def packed_frames(frames):
    """The frames a remap reads: checked (uint8 (h, w, 3) CUDA), made contiguous."""
    return _frames.packed_frames(frames)


def rect_buffers(maps, out=None):
    """The destination frames of a remap: ``out`` checked (uint8 contiguous CUDA (ho, wo, 3) per map), or new tensors."""
    return _frames.packed_buffers([m.size for m in maps], [m.device for m in maps], out, 'map', '(ho, wo, 3)')


def remap(frames, maps, fill=(0, 0, 0), out=None):
    """rtm3d_frames_remap: frames = list of uint8 (h, w, 3) CUDA tensors, maps = one LensMap per frame (frames may share one)
    -> list of uint8 (ho, wo, 3) CUDA tensors (``out``, or new ones).  fill: the three bytes of a pixel without a source and
    of a sample outside the frame."""
    import torch
    maps = list(maps)
    frames = packed_frames(frames)
    if len(frames) != len(maps):
        raise ValueError('%d maps for %d frames' % (len(maps), len(frames)))
    cm = c_maps(maps)
    dev = frames[0].device
    with torch.cuda.device(dev):
        out = rect_buffers(maps, out)
        _lib.check(_lib.load().rtm3d_frames_remap(_lib.stream_ptr(dev), len(frames), _lib.ptr_array(frames), _lib.hw_array(frames), cm,
                                                  _lib.ptr_array(out), c_fill(fill)), 'frames_remap')
    return out
