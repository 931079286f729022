"""MXFP8 (OCP Microscaling v1.0, e4m3 elements, E8M0 scale per 32 elements) on the host: the rule csrc/conv_mx8.hip applies
on the device, restated in numpy, and the weight packing of rtm3d_op_conv_mx8 (include/rtm3d_hip.h).

Per block of 32 values:  shared_exp = floor(log2(amax)) - 8, clamped to [-127, 127] (an all-zero block gets 0, i.e. scale
byte 127); element = round-to-nearest-even e4m3fn(x / 2^shared_exp), saturated to +-448.  torch's float8_e4m3fn cast does not
saturate (it returns NaN above 464), so nothing here goes through it.

Non-finite values (fp16 head maps are not guaranteed finite), the device's rule: the block maximum is taken with fmax, so a NaN
never reaches a scale - the scale comes from the other values of the block, an infinity among them gives byte 247, an all-NaN
block gets 127 like an all-zero one.  A NaN element becomes sign | 0x7e, +-448 in its block's scale, as an infinity does: code
0x7f / 0xff (e4m3fn's NaN) is never written.
"""
import numpy as np

BLOCK = 32
E4M3_MAX = 448.0


def scale_bytes(amax):
    """E8M0 byte (shared_exp + 127) of blocks with largest magnitude `amax` (float32 array, >= 0, not NaN; +inf gives 247)."""
    a = np.asarray(amax, np.float32)
    e = ((a.view(np.uint32) >> 23) & 0xff).astype(np.int32)
    s = np.clip(e - 127 - 8, -127, 127) + 127
    s = np.where(e == 0, 0, s)                              # subnormal amax: clamped to the smallest scale
    return np.where(a == 0, 127, s).astype(np.uint8)


def pow2(k):
    """2^k as float32 for integer k in [-254, 254] (two exact factors)."""
    k = np.asarray(k, np.int32)
    a = k // 2
    b = k - a
    return ((a + 127).astype(np.uint32) << 23).view(np.float32) * ((b + 127).astype(np.uint32) << 23).view(np.float32)


def e4m3_encode(v):
    """Round-to-nearest-even OCP e4m3fn code (uint8) of float32 values, saturated to +-448."""
    v = np.asarray(v, np.float32)
    sign = ((v.view(np.uint32) >> 31).astype(np.uint32) << 7)
    a = np.abs(v)
    e = ((a.view(np.uint32) >> 23) & 0xff).astype(np.int32) - 127
    e = np.maximum(e, -6)                                   # e4m3 subnormals share exponent -6 (quantum 2^-9)
    small = a < E4M3_MAX                                    # false for a NaN, like the device's !(a < 448)
    q = np.rint(np.where(small, a, 0) * pow2(3 - np.minimum(e, 8))).astype(np.int64)
    code = ((e + 7) << 3) + q - 8
    code = np.where(small, code, 0x7e)                      # (448, 464] rounds to 448; above, infinities and NaNs saturate
    return (code.astype(np.uint32) | sign).astype(np.uint8)


def e4m3_decode(b):
    """float32 value of e4m3fn codes (0x7f / 0xff: NaN)."""
    b = np.asarray(b, np.uint8).astype(np.int32)
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2(e - 10.0))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(s == 1, -v, v).astype(np.float32)


def quantize(x):
    """Blocks of 32 along the last axis of float32 `x` -> (codes uint8 of x's shape, scale bytes [..., n/32])."""
    x = np.asarray(x, np.float32)
    assert x.shape[-1] % BLOCK == 0, x.shape
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // BLOCK, BLOCK))
    sb = scale_bytes(np.fmax.reduce(np.abs(xb), axis=-1, initial=0.0))       # fmax: a NaN never reaches a scale
    with np.errstate(invalid='ignore', over='ignore'):
        codes = e4m3_encode(xb * pow2(127 - sb.astype(np.int32))[..., None])
    return codes.reshape(x.shape), sb


def dequantize(codes, sb):
    """Inverse of quantize (float64)."""
    c = e4m3_decode(codes).astype(np.float64)
    cb = c.reshape(c.shape[:-1] + (c.shape[-1] // BLOCK, BLOCK))
    return (cb * np.exp2(sb.astype(np.float64) - 127)[..., None]).reshape(c.shape)


def pack_conv_weights(wt):
    """wt: (taps, cout, cin) float32 of one group (BN folded) -> (e4m3 [cout/256][kt][256][64], E8M0 [cout/256][kt][256][2])
    with kt = taps * cin/64 k-steps in the order k = tap * (cin/64) + chunk (rtm3d_op_conv_mx8).  Scales per (output channel,
    tap, 32 input channels)."""
    T, cout, cin = wt.shape
    assert cout % 256 == 0 and cin % 64 == 0, (cout, cin)
    codes, sb = quantize(np.ascontiguousarray(wt, np.float32))                # (T, cout, cin), (T, cout, cin/32)
    cpt = cin // 64
    c = codes.reshape(T, cout // 256, 256, cpt, 64).transpose(1, 0, 3, 2, 4)   # nt, tap, chunk, row, 64
    s = sb.reshape(T, cout // 256, 256, cpt, 2).transpose(1, 0, 3, 2, 4)
    return (np.ascontiguousarray(c).reshape(-1), np.ascontiguousarray(s).reshape(-1))


def dequantized_weights(wt):
    """What the device multiplies with: the weights of pack_conv_weights dequantised, (taps, cout, cin) float64."""
    codes, sb = quantize(np.ascontiguousarray(wt, np.float32))
    return dequantize(codes, sb)
