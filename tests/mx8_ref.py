"""The yardstick of the MXFP8 regime suites (tests/test_gpu_mx8_regimes.py, tests/test_mx8_regimes.py): a float64 convolution of
dequantised operands for an arbitrary tap list, the exact-data builder whose sums every fp32 summation order gets right, and the
fp16 value classes of the quantise kernel.  Numpy only, on the CPU."""
import numpy as np

from rtm3d_amd import mx8


def conv(x, w, bias, taps, in_coff, relu):
    """x: (B, H, W, in_C) float64, w: (G, T, cout, cin) float64, bias: (G, cout), taps: T x (dy, dx), in_coff[g]: the first input
    channel of group g -> list over the groups of (B, H, W, cout) float64: out[g][n, y, x, o] =
    sum_t sum_c x[n, y + dy_t, x + dx_t, in_coff[g] + c] * w[g, t, o, c] + bias[g, o], zero outside the map, ReLU if asked."""
    x, w, bias = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    B, H, W, C = x.shape
    G, T, cout, cin = w.shape
    assert len(taps) == T and len(in_coff) == G
    P = max(max(abs(dy), abs(dx)) for dy, dx in taps)
    xp = np.zeros((B, H + 2 * P, W + 2 * P, C))
    xp[:, P:P + H, P:P + W] = x
    outs = []
    for g in range(G):
        acc = np.zeros((B * H * W, cout))
        for t, (dy, dx) in enumerate(taps):
            sl = xp[:, P + dy:P + dy + H, P + dx:P + dx + W, in_coff[g]:in_coff[g] + cin].reshape(B * H * W, cin)
            acc += np.einsum('mc,oc->mo', sl, w[g, t], optimize=True)
        acc += bias[g]
        if relu:
            acc = np.maximum(acc, 0.0)
        outs.append(acc.reshape(B, H, W, cout) + 0.0)              # (+ 0.0: no negative zeros, the device has none either)
    return outs


def exact_blocks(rng, shape, spread, shift=0, density=1.0):
    """float32 values int * 2^(e + shift): ints in [-8, 8], thinned to `density`, with one +-8 per block of 32 along the last axis
    (at a random place), e random per block in [-spread, spread].  They ARE e4m3 values times their block's scale, so the host
    quantiser represents them exactly; every value is a multiple of 2^(shift - spread)."""
    ints = rng.integers(-8, 9, shape).astype(np.float64)
    if density < 1.0:
        ints *= rng.random(shape) < density
    blocks = ints.reshape(-1, 32)
    n = len(blocks)
    blocks[np.arange(n), rng.integers(0, 32, n)] = np.where(rng.random(n) < 0.5, 8.0, -8.0)
    e = rng.integers(-spread, spread + 1, shape[:-1] + (shape[-1] // 32,))
    v = (blocks.reshape(shape) * np.exp2(e + float(shift)).repeat(32, -1)).astype(np.float32)
    assert np.array_equal(mx8.dequantize(*mx8.quantize(v)), v.astype(np.float64))
    return v


def quantum(v):
    """The largest power of two every value of `v` is a multiple of (float64; 0 for an all-zero array)."""
    v = np.abs(np.asarray(v, np.float64))
    v = v[v != 0]
    if v.size == 0:
        return 0.0
    m, e = np.frexp(v)                               # v = m * 2^e, m in [0.5, 1): m * 2^53 is an integer
    mi = (m * 2.0 ** 53).astype(np.int64)
    return float((np.exp2(e - 53.0) * (mi & -mi)).min())


def l1_exactness(x, w, bias, taps, in_coff):
    """(largest L1 sum over the outputs, common quantum): with sum |x_k w_k| + |bias| < 2^24 quanta every partial sum of every
    summation order is a multiple of the quantum below 2^24 of them, i.e. an fp32 number: the kernel's result is exact."""
    l1 = max(float(o.max()) for o in conv(np.abs(x), np.abs(w), np.abs(bias), taps, in_coff, False))
    qs = [q for q in (quantum(x) * quantum(w), quantum(bias)) if q > 0]
    return l1, min(qs)


def assert_exact(x, w, bias, taps, in_coff):
    l1, q = l1_exactness(x, w, bias, taps, in_coff)
    assert l1 < 2.0 ** 24 * q, 'L1 sum %g is %.3g x 2^24 quanta of %g' % (l1, l1 / q / 2.0 ** 24, q)
    return l1, q


# ------------------------------------------------------------------------------ fp16 value classes of the quantise kernel
NAN_CLASSES = ('one_nan', 'nan_and_inf', 'all_nan')
VALUE_CLASSES = ('pos_inf', 'neg_inf', 'neg_zero', 'f16_max', 'only_2m24', 'all_negative', 'amax_pow2', 'amax_below_pow2',
                 'ties', 'e4m3_subnormal', 'above_448') + NAN_CLASSES


def value_block(name, rng):
    """One block of 32 fp16-exact float32 values of the class `name`."""
    b = (rng.standard_normal(32) * 3.0).astype(np.float16).astype(np.float32)
    if name == 'pos_inf':
        b[5] = np.inf
    elif name == 'neg_inf':
        b[31] = -np.inf
    elif name == 'neg_zero':                       # zeros of both signs alone: scale 127, codes 0x00 / 0x80
        b[:] = 0.0
        b[1::3] = -0.0
    elif name == 'f16_max':
        b[0], b[7] = 65504.0, -65504.0
    elif name == 'only_2m24':                      # the smallest fp16 subnormal alone
        b[:] = 0.0
        b[17] = 2.0 ** -24
    elif name == 'all_negative':
        b = (-np.abs(b) - 1.0).astype(np.float16).astype(np.float32)
    elif name == 'amax_pow2':                      # floor(log2) sits exactly on the binade's lower edge ...
        b = np.clip(b, -100, 100)
        b[3] = -256.0
    elif name == 'amax_below_pow2':                # ... and one fp16 ulp below it
        b = np.clip(b, -100, 100)
        b[3] = 255.875
    elif name == 'ties':                           # block scale 2^0 (amax 256): halfway between e4m3 neighbours, both directions
        b[:] = 0.0
        b[0] = 256.0
        t = [1.0625, 1.1875, -2.125, -2.375, 17.0, 19.0, -136.0, -152.0, 272.0, -304.0, 0.0029296875, -0.0048828125]
        b[1:1 + len(t)] = t
    elif name == 'e4m3_subnormal':                 # block scale 2^0: multiples and halves of e4m3's subnormal quantum 2^-9
        b[:] = 0.0
        b[0] = -300.0
        t = [2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10, 2.0 ** -9, 7 * 2.0 ** -9, -2.0 ** -11, 1.5 * 2.0 ** -10, 15 * 2.0 ** -10, 2.0 ** -6,
             -(2.0 ** -6 - 2.0 ** -11)]
        b[1:1 + len(t)] = t
    elif name == 'above_448':                      # block scale 2^0 (amax in [448, 512)): (448, 464] rounds to 448, above saturates
        b[0] = 511.75
        b[1:8] = [448.0, 448.25, -456.0, 464.0, -464.25, 480.0, -500.0]
    elif name == 'one_nan':
        b[9] = np.nan
    elif name == 'nan_and_inf':
        b[2], b[3], b[30] = np.nan, -np.inf, np.copysign(np.nan, -1.0)
    elif name == 'all_nan':
        b[:] = np.nan
        b[::2] = np.copysign(np.nan, -1.0)
    else:
        raise ValueError(name)
    assert np.array_equal(b.astype(np.float16).astype(np.float32), b, equal_nan=True)
    return b


def f16_values(rng, shape, classes, first=0):
    """fp16-exact float32 test values of `shape` (last axis a multiple of 32): block i holds class (first + i) % len(classes) of
    `classes` while the classes last, then magnitudes all over the fp16 range, zero blocks and fp16-subnormal blocks.  Returns
    (values, {class: index of its block in values.reshape(-1, 32)})."""
    x = rng.standard_normal(shape) * np.exp2(rng.integers(-14, 13, shape[:-1] + (shape[-1] // 32,))).repeat(32, -1)
    blocks = np.clip(x, -60000, 60000).astype(np.float16).astype(np.float32).reshape(-1, 32)
    n = len(blocks)
    rest = np.arange(n) >= len(classes)
    blocks[rest & (rng.random(n) < 0.05)] = 0.0
    sub = rest & (rng.random(n) < 0.05)
    blocks[sub] = rng.integers(-1000, 1000, (int(sub.sum()), 32)) * 2.0 ** -24
    where = {}
    for i in range(min(n, len(classes))):
        name = classes[(first + i) % len(classes)]
        blocks[i] = value_block(name, rng)
        where[name] = i
    return blocks.reshape(shape), where


# ------------------------------------------------------------------------------ the data of a conv case
def conv_case_data(c):
    """Exact operands of a case of mx8_regimes.CONV_CASES: x (B, H, W, in_C), w (G, T, cout, cin), bias (G, cout), all float32,
    with the L1 bound asserted."""
    import zlib
    from tests.mx8_regimes import TAPS
    rng = np.random.default_rng(zlib.crc32(c['name'].encode()))
    taps = TAPS[c['taps']]
    x = exact_blocks(rng, (c['B'], c['H'], c['W'], c['in_C']), c['spread'], c['sx'], c['density'])
    w = exact_blocks(rng, (c['groups'], len(taps), c['cout'], c['cin']), c['spread'], c['sw'], c['density'])
    bias = (rng.integers(-64, 65, (c['groups'], c['cout'])) * 2.0 ** (c['sx'] + c['sw'] - 2)).astype(np.float32)
    if c['zero_block']:                            # output channels 32-63 of every group: no weights, bias <= 0
        w[:, :, 32:64] = 0.0
        bias[:, 32:64] = -np.abs(bias[:, 32:64])
    assert_exact(x, w, bias, taps, c['in_coff'])
    return x, w, bias


def epilogue_classes(y):
    """Which epilogue classes the blocks of the float32 output map `y` (last axis a multiple of 32) hold: the block maximum in the
    upper / lower 16 channels, and in the channels of lane half 1 / 0 of the MFMA's C layout (channel bit 2 set / clear: lanes l
    and l ^ 32 hold alternate runs of four channels), each time with the other half alone giving a smaller scale byte - a
    reduction that forgets a half then gets that block's scale wrong; and a block maximum in [448, 512) x 2^s, which saturates."""
    a = np.abs(np.asarray(y, np.float32)).reshape(-1, 32)
    sb = mx8.scale_bytes(a.max(-1)).astype(int)
    ch = np.arange(32)
    out = {}
    for name, sel in (('max_upper16', ch >= 16), ('max_lower16', ch < 16), ('max_lane_half_1', (ch & 4) != 0), ('max_lane_half_0', (ch & 4) == 0)):
        other = mx8.scale_bytes(a[:, ~sel].max(-1)).astype(int)
        out[name] = bool(((a[:, sel].max(-1) == a.max(-1)) & (other < sb) & (a[:, ~sel].max(-1) > 0)).any())
    m = np.frexp(a.max(-1))[0]                       # amax = m * 2^e, m in [0.5, 1)
    out['saturates'] = bool((m >= 448.0 / 512.0).any())
    return out
