"""Input pipeline step in front of the hot path on the GPU.

``letterbox_normalize(images, size, mean, std)`` takes already resized uint8 HWC images (what
``TestTransform``'s ``Resize`` hands to ``DatasetReader._apply_padding``), pads each one centred into the
network canvas with its own mean colour (datasets/dataset_reader.py:175-195) and applies
``Normalize -> ToTensor -> ToNCHW`` (preprocess/transforms.py:110-120, 312-322).  ``adjust_K`` shifts the
principal point like dataset_reader.py:189-193.

``preprocess_batch`` is the whole step for a batch of ragged ORIGINAL images in two kernel launches: ``Resize``
(transforms.py:480-495: longest side -> ``resize_to``, ``cv2.resize(INTER_LINEAR)``) + letterbox + normalise, writing
either the reference's fp32 NCHW batch or directly the network's fp16 NHWC4 input tensor (``Model.forward_logits`` is
then called with ``preloaded=True``).  ``resize_K`` follows ToPercentCoords -> Resize -> ToAbsoluteCoords
(transforms.py:146-176).  The resize restates OpenCV's published fixed-point bilinear algorithm; OpenCV is absent from
the build image and the reference holds no fixture for it, so that one step is PARITY UNPINNED (everything else here is
bit-exact against vectors produced by the reference's own code).
"""
import ctypes

import numpy as np
import torch

from . import _frames, _lib


def normalize_lut(mean, std):
    """float32((v / 255. - mean[c]) / std[c]) for v in 0..255, evaluated in float64 with float32 mean/std
    exactly like ``Normalize`` + ``ToTensor`` (transforms.py:110-120, 312-317)."""
    v = np.arange(256, dtype=np.float64)[None, :] / 255.
    m = np.asarray(mean, np.float32).reshape(3, 1)
    s = np.asarray(std, np.float32).reshape(3, 1)
    return np.ascontiguousarray(((v - m) / s).astype(np.float32))


_LUTS = {}


def device_luts(mean, std, dev):
    """(fp32 LUT, fp16 LUT) on the device, cached per (mean, std, device): building them per call would put a pageable
    host->device copy (which blocks the host and serialises streams) in front of every batch."""
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), dev.index)
    hit = _LUTS.get(key)
    if hit is None:
        lut = normalize_lut(mean, std)
        with torch.cuda.device(dev):
            hit = (torch.as_tensor(lut, device=dev), torch.as_tensor(lut.astype(np.float16), device=dev))   # round-to-nearest-even, as the device cast
        _LUTS[key] = hit
    return hit


def letterbox_normalize(images, size, mean, std, out=None):
    """images: list of uint8 CUDA tensors (h, w, 3); size = (H, W).  Returns ((B,3,H,W) fp32 CUDA tensor,
    [(pad_w, pad_h)] per image)."""
    lib = _lib.load()
    H, W = int(size[0]), int(size[1])
    if not images:
        raise ValueError('no images')
    dev = images[0].device
    if dev.type != 'cuda':
        raise RuntimeError('rtm3d_amd.preprocess needs CUDA (ROCm) tensors; there is no CPU path')
    B = len(images)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        lut = torch.as_tensor(normalize_lut(mean, std), device=dev)
        sums = torch.zeros(B, 3, dtype=torch.int64, device=dev)
        pads = []
        stream = _lib.stream_ptr(dev)
        for b, img in enumerate(_frames.packed_frames(images, 'expected uint8 (h, w, 3) images')):
            h, w = int(img.shape[0]), int(img.shape[1])
            _lib.check(lib.rtm3d_preprocess(stream, img.data_ptr(), h, w, out[b].data_ptr(), H, W, lut.data_ptr(), sums[b].data_ptr()),
                       'preprocess')
            pads.append(((W - w) // 2, (H - h) // 2))
    return out, pads


def adjust_K(K, pad_w, pad_h):
    """K: (..., 9) row-major intrinsics; cx += pad_w, cy += pad_h (datasets/dataset_reader.py:189-193)."""
    K = np.array(K, dtype=np.float64, copy=True).reshape(-1, 9)
    K[:, 2] += pad_w
    K[:, 5] += pad_h
    return K


def resized_size(h, w, resize_to):
    """transforms.Resize with an int size (preprocess/transforms.py:484-490): rate = size / max(h, w),
    dsize = (int(w * rate), int(h * rate)).  Returns (h', w')."""
    rate = resize_to / max(h, w)
    return int(h * rate), int(w * rate)


def resize_K(K, hw, new_hw):
    """ToPercentCoords -> Resize -> ToAbsoluteCoords on the intrinsics (transforms.py:146-176):
    K[:, :3] /= w; K[:, 3:6] /= h; then K[:, :3] *= w'; K[:, 3:6] *= h'."""
    K = np.array(K, dtype=np.float64, copy=True).reshape(-1, 9)
    K[:, :3] /= hw[1]
    K[:, 3:6] /= hw[0]
    K[:, :3] *= new_hw[1]
    K[:, 3:6] *= new_hw[0]
    return K


def preprocess_batch(images, size, mean, std, resize_to=None, out=None, model=None, heads='dense', head_precision=None):
    """images: list of uint8 CUDA tensors (h, w, 3), any sizes.  size = (H, W) network canvas.
    resize_to: None (images are already resized) or the reference's INPUT_SIZE (longest side after Resize).
    model given: write straight into that model's fp16 NHWC4 input tensor for batch (B, H, W) - call
    ``model.forward_logits(None, preloaded=(B, H, W), heads=heads)`` next (heads: the plan that forward will replay);
    otherwise returns the fp32 (B,3,H,W) batch.
    Returns (out or None, [(pad_w, pad_h)], [(h', w')])."""
    lib = _lib.load()
    H, W = int(size[0]), int(size[1])
    if not images:
        raise ValueError('no images')
    dev = images[0].device
    if dev.type != 'cuda':
        raise RuntimeError('rtm3d_amd.preprocess needs CUDA (ROCm) tensors; there is no CPU path')
    B = len(images)
    imgs = _frames.packed_frames(images, 'expected uint8 (h, w, 3) images')
    hw = np.array([[int(i.shape[0]), int(i.shape[1])] for i in imgs], np.int32)
    rhw = np.array([resized_size(h, w, resize_to) if resize_to else (h, w) for h, w in hw], np.int32)
    if (rhw[:, 0] > H).any() or (rhw[:, 1] > W).any() or (rhw < 1).any():
        raise ValueError('a resized image does not fit the %dx%d canvas: %s' % (H, W, rhw.tolist()))
    ptrs = _lib.ptr_array(imgs)
    d_lut, d_lut16 = device_luts(mean, std, dev)
    with torch.cuda.device(dev):
        sums = torch.zeros(B, 3, dtype=torch.int64, device=dev)
        stream = _lib.stream_ptr(dev)
        if model is not None:
            base, border = model.input_tensor(B, H, W, dev, heads, head_precision)
            mode, dst, ret = 1, base, None
        else:
            if out is None:
                out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
            mode, dst, border, ret = 0, out.data_ptr(), 0, out
        _lib.check(lib.rtm3d_preprocess_batch(stream, B, ptrs, hw.ctypes.data_as(ctypes.c_void_p), rhw.ctypes.data_as(ctypes.c_void_p),
                                              ctypes.c_void_p(dst), mode, H, W, border, d_lut.data_ptr(), d_lut16.data_ptr(),
                                              sums.data_ptr()), 'preprocess_batch')
    pads = [((W - int(w)) // 2, (H - int(h)) // 2) for h, w in rhw]
    return ret, pads, [(int(h), int(w)) for h, w in rhw]


# ------------------------------------------------------------------------------------------------ camera-frame bookkeeping
def frame_geometry(hw, size, resize_to=None):
    """rtm3d_frame_geometry (host, no device): per frame (h, w) its size after Resize and its centred place on the (H, W)
    canvas - ``resized_size`` and the pad rule of ``preprocess_batch`` - as the ctypes array of ``_lib.FrameGeom`` that the
    device entries below take.  A frame that does not fit is a ValueError naming it, like ``preprocess_batch``'s."""
    lib = _lib.load()
    hw = np.ascontiguousarray(np.asarray(hw, np.int32).reshape(-1, 2))
    geom = (_lib.FrameGeom * len(hw))()
    if lib.rtm3d_frame_geometry(len(hw), hw.ctypes.data_as(ctypes.c_void_p), int(resize_to or 0), int(size[0]), int(size[1]), geom) != 0:
        raise ValueError(lib.rtm3d_last_error().decode())
    return geom


def adjust_K_device(K_camera, geom, out=None):
    """``adjust_K(resize_K(K, (h, w), (h', w')), pad_w, pad_h)`` per image on the device (rtm3d_frames_adjust_k, fp64, the same
    operation order, bit for bit): K_camera (B, 9) float64 CUDA tensor of the cameras' own intrinsics, geom =
    ``frame_geometry(...)``.  Stream-ordered, no host-to-device copy.  Returns the (B, 9) intrinsics of the network canvas."""
    lib = _lib.load()
    B = len(geom)
    if not isinstance(K_camera, torch.Tensor) or not K_camera.is_cuda or K_camera.dtype != torch.float64 or K_camera.numel() != B * 9:
        raise ValueError('K_camera must be a float64 CUDA tensor with %d x 9 intrinsics' % B)
    dev = K_camera.device
    K_camera = K_camera.contiguous()
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(B, 9, dtype=torch.float64, device=dev)
        if out.dtype != torch.float64 or out.numel() != B * 9 or not out.is_contiguous() or out.device != dev:
            raise ValueError('out must be a contiguous float64 tensor of %d x 9 on %s' % (B, dev))
        _lib.check(lib.rtm3d_frames_adjust_k(_lib.stream_ptr(dev), B, geom, K_camera.data_ptr(),
                                             out.data_ptr()), 'frames_adjust_K')
    return out


def records_to_camera(rec, geom, K_camera=None, boxes=None, kitti=False):
    """Un-letterbox detection records IN PLACE (rtm3d_records_to_camera): rec (B, topk, 32) fp32 CUDA records of
    ``distributed.pack_records`` in canvas pixels -> the same records with key point, vertices and 2D box in the pixels of
    each camera frame.  kitti=True (needs K_camera, the cameras' own (B, 9) float64 intrinsics, and boxes, the
    ``model_utils.Boxes3D`` the records were packed from): also returns (B, topk, 16) float64 rows, the numbers of a KITTI
    label line per kept box (``kitti_results.kitti_label_values`` + flag), zeros elsewhere.  Returns rec or (rec, rows)."""
    from .model_utils import FUN_ACCEPT
    lib = _lib.load()
    B = len(geom)
    if not isinstance(rec, torch.Tensor) or not rec.is_cuda or rec.dtype != torch.float32 or rec.dim() != 3 or rec.shape[0] != B or \
            rec.shape[2] != 32 or not rec.is_contiguous():
        raise ValueError('rec must be a contiguous fp32 CUDA tensor (%d, topk, 32)' % B)
    dev, topk = rec.device, int(rec.shape[1])
    rows, args = None, [None] * 4
    if kitti:
        if K_camera is None or boxes is None:
            raise ValueError('the KITTI rows need K_camera and the solver outputs (boxes)')
        K_camera = torch.as_tensor(K_camera, dtype=torch.float64, device=dev).reshape(B, 9).contiguous()
        if boxes.x.shape[0] != B * topk:
            raise ValueError('boxes hold %d slots, the records %d' % (boxes.x.shape[0], B * topk))
        args = [K_camera.data_ptr(), boxes.x.data_ptr(), boxes.fun.data_ptr(), boxes.status.data_ptr()]
    with torch.cuda.device(dev):
        if kitti:
            rows = torch.empty(B, topk, 16, dtype=torch.float64, device=dev)
        _lib.check(lib.rtm3d_records_to_camera(_lib.stream_ptr(dev), B, topk, geom, rec.data_ptr(),
                                               *args, float(FUN_ACCEPT), rows.data_ptr() if kitti else None), 'records_to_camera')
    return (rec, rows) if kitti else rec
