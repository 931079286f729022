"""Cases of the head-backward tests: saved activations, folded fp16 weights, BN scales and upstream logit gradients.

A case is a dict: B, H, W (the MAP), K (channels per head), num_conv, S (grad_scale), input_grad, want_slices (None: default),
    acts[k]   k = 0 .. num_conv: NHWC fp16 numpy, z (256 channels) then the output of conv k (G * 256 channels)
    wf[k][g]  k = 1 .. num_conv: (256, 256, 3, 3) fp16, the folded weight as a forward uses it;  wo[g]: (K[g], 256, 3, 3) fp16
    scale[k][g]  (256,) fp32 BN scale;  dlogits[g]: (B, K[g], H, W) fp32
The backward only reads saved activations (operand and mask), so an integer case may hold ANY activations.
"""
import numpy as np

K_RTM3D, K_ONE, K_16, K_SMOKE = (3, 16, 2, 2), (1, 16, 2, 2), (16, 16, 2, 2), (3, 8)


def _sparse(rng, shape, density, values):
    a = np.zeros(shape, np.float32)
    m = rng.random(shape) < density
    a[m] = rng.choice(np.asarray(values, np.float32), int(m.sum()))
    return a


def int_case(seed, B, H, W, K, num_conv, input_grad=True, want_slices=None, dead=False):
    """Small integers throughout: every intermediate of the chain stays <= 2048 in magnitude (exact in fp16) and every fp32 sum
    below 2 ** 24 (check_exact verifies it on the reference result), S = 1, BN scales are powers of two.  dead=True: the
    activations are zero on whole channels and whole rows (the mask)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    G = len(K)
    acts = [_sparse(rng, (B, H, W, 256), 0.15, [-2, -1, 1, 2]).astype(np.float16)]
    for k in range(1, num_conv + 1):
        a = _sparse(rng, (B, H, W, G * 256), 0.3, [1, 2])
        if dead:
            a[..., ::3] = 0
            a[:, ::2] = 0
        acts.append(a.astype(np.float16))
    wf = [None] + [[_sparse(rng, (256, 256, 3, 3), 0.01, [-1, 1]).astype(np.float16) for _ in range(G)] for _ in range(num_conv)]
    wo = [_sparse(rng, (k, 256, 3, 3), 0.05, [-1, 1]).astype(np.float16) for k in K]
    scale = [None] + [[rng.choice(np.asarray([0.5, 1.0, 2.0], np.float32), 256) for _ in range(G)] for _ in range(num_conv)]
    dlogits = [_sparse(rng, (B, k, H, W), 0.1, [-2, -1, 1, 2]) for k in K]
    return {'B': B, 'H': H, 'W': W, 'K': tuple(K), 'num_conv': num_conv, 'S': 1.0, 'input_grad': input_grad, 'want_slices': want_slices,
            'acts': acts, 'wf': wf, 'wo': wo, 'scale': scale, 'dlogits': dlogits}


def check_exact(case, ref):
    """The builder's promise, checked on the reference result (head_backward_ref.flat of the Q16 chain)."""
    npix = case['B'] * case['H'] * case['W']
    for name, v in ref.items():
        if name.startswith(('go', 'dh', 'dz')):
            assert np.abs(v).max() <= 2048 and np.all(v == np.round(v)), name
    amax = max(float(np.abs(a.astype(np.float32)).max()) for a in case['acts'])
    gmax = max(float(np.abs(v).max()) for n, v in ref.items() if n.startswith(('go', 'dh')))
    assert npix * amax * gmax < 2 ** 24 and 9 * 256 * len(case['K']) * gmax < 2 ** 24


# id -> builder arguments: the regimes of the issue
INT_CASES = {
    'g1_5x7_b1': dict(seed=1, B=1, H=5, W=7, K=(3,), num_conv=2),                       # every off-centre dilation-6 tap in the border
    'g2_smoke_13x20_b3': dict(seed=2, B=3, H=13, W=20, K=K_SMOKE, num_conv=2),          # an odd pixel count, the smoke table
    'g4_rtm3d_16x32_b2': dict(seed=3, B=2, H=16, W=32, K=K_RTM3D, num_conv=2),
    'g4_k1_nconv1': dict(seed=4, B=1, H=5, W=7, K=K_ONE, num_conv=1),
    'g4_k16_nconv3': dict(seed=5, B=1, H=8, W=9, K=K_16, num_conv=3),
    'more_slices_than_tiles': dict(seed=6, B=1, H=5, W=7, K=(3, 2), num_conv=2, want_slices=8),   # 35 pixels: 2 tiles
    'remainder_slice': dict(seed=7, B=3, H=13, W=20, K=(2,), num_conv=1, want_slices=7),          # 25 tiles: 4 per slice, the last holds 1
    'dead_channels_rows': dict(seed=8, B=2, H=8, W=9, K=K_RTM3D, num_conv=2, dead=True),
    'no_input_grad': dict(seed=9, B=1, H=5, W=7, K=K_RTM3D, num_conv=2, input_grad=False),
}


def real_case(seed, B, H, W, S, num_conv=2, K=K_RTM3D):
    """Random fp16-representable activations (each layer's output is the fp16-rounded fp32 forward of the layer before, as a
    device forward leaves them), synth_state_dict weights folded as plan.fold_bn folds them."""
    import torch
    import torch.nn.functional as F
    from rtm3d_amd import plan as plan_mod
    from rtm3d_amd.weights import synth_state_dict, head_table
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = synth_state_dict('DLA-34', seed=3, style='trained', header_num_conv=num_conv)
    table = head_table('rtm3d', 3)
    G = len(K)
    wf, bf, scale = [None], [None], [None]
    for k in range(1, num_conv + 1):
        ws, bs, ss = [], [], []
        for seq, _, _ in table[:G]:
            conv, bn = 'detect_header.%s.%d' % (seq, 3 * (k - 1)), 'detect_header.%s.%d' % (seq, 3 * (k - 1) + 1)
            w, b = plan_mod.fold_bn(sd, conv, bn)
            ws.append(w.astype(np.float16)); bs.append(b)
            ss.append((plan_mod._np(sd, bn + '.weight') / np.sqrt(plan_mod._np(sd, bn + '.running_var') + plan_mod.BN_EPS)).astype(np.float32))
        wf.append(ws); bf.append(bs); scale.append(ss)
    wo = [plan_mod.fold_bn(sd, 'detect_header.%s.%s' % (seq, last))[0].astype(np.float16) for seq, last, _ in table[:G]]
    z = rng.standard_normal((B, H, W, 256)).astype(np.float16)
    acts = [z]
    x = torch.from_numpy(z.astype(np.float32)).permute(0, 3, 1, 2)
    for k in range(1, num_conv + 1):
        dil = 6 if k == 1 else 1
        outs = []
        for g in range(G):
            xi = x if k == 1 else x[:, g * 256:(g + 1) * 256]
            y = F.conv2d(xi, torch.from_numpy(wf[k][g].astype(np.float32)), torch.from_numpy(bf[k][g]), dilation=dil, padding=dil)
            outs.append(torch.relu(y).to(torch.float16).to(torch.float32))
        x = torch.cat(outs, 1)
        acts.append(x.permute(0, 2, 3, 1).contiguous().numpy().astype(np.float16))
    dlogits = [(rng.standard_normal((B, k, H, W)) * 1e-2).astype(np.float32) for k in K]
    return {'B': B, 'H': H, 'W': W, 'K': tuple(K), 'num_conv': num_conv, 'S': float(S), 'input_grad': True, 'want_slices': None,
            'acts': acts, 'wf': wf, 'wo': wo, 'scale': scale, 'dlogits': dlogits}
