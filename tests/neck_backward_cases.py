"""Cases of the neck-fusion-backward tests (layout: tests/neck_backward_ref.py).

The backward only READS saved activations, so an integer case may hold any activations; the real-valued cases hold the
fp16-rounded forward of their leaves, as a device forward leaves them.
"""
import numpy as np


def _sparse(rng, shape, density, values):
    a = np.zeros(shape, np.float32)
    m = rng.random(shape) < density
    a[m] = rng.choice(np.asarray(values, np.float32), int(m.sum()))
    return a


# ---- one transposed conv, small integers: every dX stays <= 2048 in magnitude (exact in fp16) and every fp32 sum below 2^24
# (check_layer_exact verifies it on the reference result).  S T = 4: the division is exact.
INT_LAYERS = {
    'b1_1x1': dict(seed=1, B=1, Hi=1, Wi=1, want=(None,)),                    # every tap touches the border
    'b3_3x5': dict(seed=2, B=3, Hi=3, Wi=5, want=(None,)),                    # 45 pixels: a partial 32-pixel tile, odd width
    'b2_4x8': dict(seed=3, B=2, Hi=4, Wi=8, want=(None,)),                    # 64 pixels: whole tiles
    'b1_5x7': dict(seed=4, B=1, Hi=5, Wi=7, want=(1, 2, 64)),                 # 35 pixels, 2 tiles: one slice, two slices (the
}                                                                            # last holds the remainder), more slices wanted than tiles


def int_layer(seed, B, Hi, Wi, want=None, C=256):
    rng = np.random.Generator(np.random.PCG64(seed))
    return {'B': B, 'Hi': Hi, 'Wi': Wi, 'S': 2.0, 'T': 2.0,
            'x': _sparse(rng, (B, Hi, Wi, C), 0.3, [-2, -1, 1, 2]).astype(np.float16),
            'dy': _sparse(rng, (B, 2 * Hi, 2 * Wi, C), 0.2, [-2, -1, 1, 2]).astype(np.float16),
            'w': _sparse(rng, (C, C, 4, 4), 0.02, [-1, 1]).astype(np.float16)}


def check_layer_exact(case, dx, dw):
    npix = case['B'] * case['Hi'] * case['Wi']
    assert np.abs(dx).max() <= 2048 and np.all(dx == np.round(dx))
    assert npix * 2 * 2 < 2 ** 24 and 16 * case['x'].shape[3] * 2 < 2 ** 24
    assert np.all(dw * 4 == np.round(dw * 4))


# ---- the softmax backward alone
def softmax_case(seed, B, H, W, C=256):
    """u spans +-30 in every channel (a kernel that skips the max subtraction overflows: exp(30) * H W is far beyond fp16 and the
    sum of exp(u) up to 60 apart loses every small term), except channel 0: equal values, s = 1 / (H W), and channel 1: one
    dominant pixel, s = 1 there and exp(-50) elsewhere."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.uniform(-30.0, 30.0, (B, H, W, C))
    u[:, 0, 0, 2:] = 30.0
    u[:, -1, -1, 2:] = -30.0
    u[..., 0] = 1.5
    u[..., 1] = -20.0
    for b in range(B):
        u[b, (H - 1) // 2, (W * (b + 1)) // (B + 1) % W, 1] = 30.0
    dz = rng.standard_normal((B, H, W, C))
    return {'B': B, 'H': H, 'W': W, 'u': u.astype(np.float16), 'dz': dz.astype(np.float16)}


# ---- the whole chain, real values
def real_case(seed, B, H, W, S, T, levels=3, C=256, want_slices=None):
    """Leaves kfpn_h (standard normal, fp16), weights N(0, 1 / (4 C)) as fp16 (a transposed-conv output sums 4 taps x C channels:
    unit variance at every level), the forward rounded to fp16 map by map, and dz = fp16(S * 1e-2 * normal)."""
    import torch
    from tests import neck_backward_ref as ref
    rng = np.random.Generator(np.random.PCG64(seed))
    w = [[(rng.standard_normal((C, C, 4, 4)) / np.sqrt(4.0 * C)).astype(np.float16) for _ in range(l + 1)] for l in range(levels)]
    h = [rng.standard_normal((B, H >> (l + 1), W >> (l + 1), C)).astype(np.float16) for l in range(levels)]
    xs, us = ref.forward([ref._nchw(a) for a in h], [[torch.as_tensor(a.astype(np.float64)) for a in row] for row in w], True)
    nhwc = lambda t: np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy()).astype(np.float16)
    dz = (float(S) * 1e-2 * rng.standard_normal((B, H, W, C))).astype(np.float16)
    return {'B': B, 'H': H, 'W': W, 'levels': levels, 'C': C, 'S': float(S), 'T': float(T), 'want_slices': want_slices,
            'dz': dz, 'us': [nhwc(u) for u in us], 'xs': [[nhwc(x) for x in row] for row in xs], 'w': w}


def fixture_case(g):
    """The case of tests/golden/neck_fusion_grad_cases.npz (fp64 throughout, S = T = 1): leaves h3 / h4 / h5, the six weights and
    G; the saved activations are the unrounded fp64 forward of the leaves."""
    import torch
    from tests import neck_backward_ref as ref
    levels = 3
    w = [[np.asarray(g['w%d_%d' % (l + 3, j)], np.float64) for j in range(l + 1)] for l in range(levels)]
    h = [torch.as_tensor(np.asarray(g['h%d' % (l + 3)], np.float64)) for l in range(levels)]                 # NCHW
    xs, us = ref.forward(h, [[torch.as_tensor(a) for a in row] for row in w], False)
    nhwc = lambda t: np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())
    G = np.asarray(g['G'], np.float64)
    B, C, H, W = G.shape
    return {'B': B, 'H': H, 'W': W, 'levels': levels, 'C': C, 'S': 1.0, 'T': 1.0, 'want_slices': None,
            'dz': np.ascontiguousarray(G.transpose(0, 2, 3, 1)), 'us': [nhwc(u) for u in us], 'xs': [[nhwc(x) for x in row] for row in xs], 'w': w}
