"""Helpers shared by the route-level suites (tests/test_gpu_conv256.py, tests/test_gpu_conv128.py, tests/test_gpu_fused.py): raw
reads and writes of a plan tensor's whole padded device image, and the launch order that puts every ordered pair of regimes next
to each other."""
import ctypes

import numpy as np
import torch

SENTINEL = np.float16(1234.0)   # channels of an output tensor outside the conv's slices
H2D, D2H = 1, 2                 # hipMemcpyKind


def _hip_memcpy(lib, dst, src, nbytes, kind):
    # (the HIP runtime librtm3d_hip.so itself links: its handle resolves the symbols of its dependencies)
    f = lib.hipMemcpy
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert f(dst, src, nbytes, kind) == 0, 'hipMemcpy failed'


def _raw(R, s):
    """(device address, padded shape (B, Hp, Wp, C), border) of the tensor Slice s lives in."""
    base, B, H, W, C, P = R.tensor_info(s)
    return base, (B, H + 2 * P, W + 2 * P, C), P


def raw_read(R, s):
    base, shape, _ = _raw(R, s)
    out = np.empty(shape, np.float16)
    torch.cuda.synchronize()
    _hip_memcpy(R.lib, out.ctypes.data, base, out.nbytes, D2H)
    return out


def raw_write(R, s, img):
    base, shape, _ = _raw(R, s)
    img = np.ascontiguousarray(img, np.float16)
    assert img.shape == shape, (img.shape, shape)
    torch.cuda.synchronize()
    _hip_memcpy(R.lib, base, img.ctypes.data, img.nbytes, H2D)


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def every_pair_order(n):
    """A sequence over 0..n-1 in which every ordered pair (a, b), a != b, appears as neighbours: an Euler circuit of the
    complete directed graph (Hierholzer)."""
    succ = {a: [b for b in range(n) if b != a] for a in range(n)}
    stack, seq = [0], []
    while stack:
        v = stack[-1]
        if succ[v]:
            stack.append(succ[v].pop())
        else:
            seq.append(stack.pop())
    return seq[::-1]
