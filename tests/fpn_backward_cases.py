"""Cases of the neck-FPN-backward tests (layout: tests/fpn_backward_ref.py).

The backward only READS saved activations, so an integer case may hold any activations; the real-valued cases hold the
fp16-rounded forward of their leaves, as a device forward leaves them.
"""
import numpy as np

from tests.neck_backward_cases import _sparse

FEAT_CHANNELS = (64, 128, 256, 512)          # DLA-34's feat0 .. feat3: Cin of the four 1x1 convs = 320, 384, 512, 512

# ---- one 1x1 conv, small integers: every dX stays <= 2048 in magnitude (exact in fp16) and every fp32 sum below 2^24
# (check_layer_exact verifies it on the reference result).  inv = 1 / 4, mul = 2: both exact.
INT_LAYERS = {
    'b1_1x1': dict(seed=1, B=1, H=1, W=1, want=(None,)),                      # one pixel: 31 of the tile's 32 rows are zero staging
    'b3_3x5': dict(seed=2, B=3, H=3, W=5, want=(None,)),                      # 45 pixels: a partial 32-pixel tile, odd width
    'b2_4x8': dict(seed=3, B=2, H=4, W=8, want=(None,)),                      # 64 pixels: whole tiles
    'b1_5x7': dict(seed=4, B=1, H=5, W=7, want=(1, 2, 64)),                   # 35 pixels, 2 tiles: one slice, two slices (the
}                                                                            # last holds the remainder), more slices wanted than tiles
INT_CIN = (64, 320, 384, 512)                # half a ci tile; 2.5 tiles (a dgrad wave with 4 live tiles); 3 tiles; 4 tiles (two dgrad blocks)
INT_INV, INT_MUL = 0.25, 2.0


def int_layer(seed, B, H, W, Cin, want=None):
    rng = np.random.Generator(np.random.PCG64(1000 * seed + Cin))
    return {'B': B, 'H': H, 'W': W, 'Cin': Cin,
            'x': _sparse(rng, (B, H, W, Cin), 0.3, [-2, -1, 1, 2]).astype(np.float16),
            'dy': _sparse(rng, (B, H, W, 256), 0.2, [-2, -1, 1, 2]).astype(np.float16),
            'A': _sparse(rng, (256, Cin), 0.1, [-2, -1, 1, 2]).astype(np.float16)}


def check_layer_exact(case, dx, dA, db):
    npix = case['B'] * case['H'] * case['W']
    assert np.abs(dx).max() <= 2048 and np.all(dx == np.round(dx))
    assert npix * 2 * 2 < 2 ** 24 and 256 * 2 * 2 * INT_MUL < 2 ** 24
    assert np.all(dA * 4 == np.round(dA * 4)) and np.all(db * 4 == np.round(db * 4))


# ---- grad add: exact by construction, with the special values
def add_case(seed, B, H, W, r):
    rng = np.random.Generator(np.random.PCG64(seed))
    e = (rng.standard_normal((B, H, W, 256)) * 100).astype(np.float16)
    f = (rng.standard_normal((B, H, W, 256)) * 100).astype(np.float16)
    e[0, 0, 0, :8] = [np.nan, np.inf, -np.inf, np.inf, 0.0, 65504.0, 6e-8, -0.0]
    f[0, 0, 0, :8] = [1.0, 1.0, 2.0, -np.inf, np.nan, 65504.0, 6e-8, 0.0]
    return {'B': B, 'H': H, 'W': W, 'r': float(r), 'e': e, 'f': f}


# ---- the whole chain
def real_case(seed, B, H, W, S, T, U, want_slices=None, C=256, fch=FEAT_CHANNELS):
    """Leaves feat0 .. feat3 (standard normal, fp16), 1x1 weights N(0, 1 / Cin) and transposed-conv weights N(0, 1 / (4 C)) as fp16
    (unit variance at every level), biases N(0, 0.01), the composed forward rounded to fp16 map by map, dz = fp16(S * 1e-2 * normal)
    and F_k = fp16(S T * 1e-2 * normal)."""
    import torch
    import torch.nn.functional as F_
    from tests import fpn_backward_ref as ref
    rng = np.random.Generator(np.random.PCG64(seed))
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    feats = [rng.standard_normal((B, H >> k, W >> k, fch[k])).astype(np.float16) for k in range(4)]
    cin = [C + fch[0], C + fch[1], C + fch[2], fch[3]]
    A = [(rng.standard_normal((C, n)) / np.sqrt(n)).astype(np.float16) for n in cin]
    b = [0.1 * rng.standard_normal(C) for _ in cin]
    wup = [(rng.standard_normal((C, C, 4, 4)) / np.sqrt(4.0 * C)).astype(np.float16) for _ in range(3)]
    conv = lambda x, k: ref._r16(F_.conv2d(x, t(A[k])[:, :, None, None], t(b[k])))
    nhwc = lambda x: np.ascontiguousarray(x.permute(0, 2, 3, 1).numpy()).astype(np.float16)
    hk = conv(ref._nchw(feats[3]), 3)
    ncat, h = [None] * 3, [None] * 3
    for k in (2, 1, 0):
        h[k] = nhwc(hk)
        cat = torch.cat([ref._r16(ref.deconv(hk, t(wup[k]))), ref._nchw(feats[k])], 1)
        ncat[k] = nhwc(cat)
        hk = conv(cat, k)
    dz = (float(S) * 1e-2 * rng.standard_normal((B, H, W, C))).astype(np.float16)
    F = [(float(S) * float(T) * 1e-2 * rng.standard_normal((B, H >> (k + 1), W >> (k + 1), C))).astype(np.float16) for k in range(3)]
    return {'B': B, 'H': H, 'W': W, 'C': C, 'S': float(S), 'T': float(T), 'U': float(U), 'want_slices': want_slices,
            'dz': dz, 'ncat': ncat, 'h': h, 'feat3': feats[3], 'F': F, 'A': A, 'wup': wup}


def fixture_params(g):
    return {k[2:]: np.asarray(g[k], np.float64) for k in g.files if k.startswith('p:')}


def fixture_case(g):
    """The case of tests/golden/neck_fpn_grad_cases.npz (fp64 throughout, S = T = U = 1): G0 is dz, G1 .. G3 stand where the fusion
    path's terms arrive; the saved activations are the unrounded fp64 composed forward of the leaves."""
    from tests import fpn_backward_ref as ref
    params = fixture_params(g)
    feats = [np.asarray(g['feat%d' % i], np.float64) for i in range(4)]
    ncat, h, _ = ref.forward_composed(feats, params)
    nhwc = lambda x: np.ascontiguousarray(np.asarray(x).transpose(0, 2, 3, 1))
    G = [np.asarray(g['G%d' % i], np.float64) for i in range(4)]
    B, C, H, W = G[0].shape
    A = [ref.compose(params, k + 3)[0] for k in range(3)] + [params['kfpn_head5.weight'][:, :, 0, 0]]
    return {'B': B, 'H': H, 'W': W, 'C': C, 'S': 1.0, 'T': 1.0, 'U': 1.0, 'want_slices': None,
            'dz': nhwc(G[0]), 'ncat': [nhwc(x.numpy()) for x in ncat], 'h': [nhwc(x.numpy()) for x in h], 'feat3': nhwc(feats[3]),
            'F': [nhwc(G[k + 1]) for k in range(3)], 'A': A, 'wup': [params['kfpn_up%d.conv_tran.weight' % (k + 3)] for k in range(3)]}


def fixture_reference_grads(res, params):
    """The reference's own parameter gradients from a chain() result via the factor rule: {name: fp64 array in torch's shape}."""
    from tests import fpn_backward_ref as ref
    out = {}
    w2 = lambda n: params[n][:, :, 0, 0]
    acc = {}
    for k in range(3):
        L = k + 3
        dwh, dwp, dbh, dbp = ref.factor_rule(res['dA'][k].numpy(), res['db'][k].numpy(), w2('kfpn_head%d.weight' % (L - 1)), w2('kfpn_proj%d.weight' % L),
                                               params['kfpn_proj%d.bias' % L])
        acc['kfpn_head%d.weight' % (L - 1)], acc['kfpn_head%d.bias' % (L - 1)] = dwh[:, :, None, None], dbh
        out['kfpn_proj%d.weight' % L], out['kfpn_proj%d.bias' % L] = dwp[:, :, None, None], dbp
        out['kfpn_up%d.conv_tran.weight' % L] = res['dwup'][k].numpy()
    out.update(acc)
    out['kfpn_head5.weight'], out['kfpn_head5.bias'] = res['dA'][3].numpy()[:, :, None, None], res['db'][3].numpy()
    return out
