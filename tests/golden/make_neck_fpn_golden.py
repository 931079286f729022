#!/usr/bin/env python
"""Reference-run fixture of the neck FPN backward: tests/golden/neck_fpn_grad_cases.npz.

    python tests/golden/make_neck_fpn_golden.py <root of the reference checkout>

RUNS the reference's KeypointFPNFusion._fpn (models/nets/keypoint_fpn_fusion.py:35-46) on the CPU in fp64; this script contains no
reference source.  The module is built with a stand-in config - OUT_CHANNELS = 8 and the KFN levels 2, 3, 4, 5 (strides 4 .. 32)
with DISTINCT feature widths 8, 16, 24, 32, so that a cin / cout or level mix-up cannot pass - and ``_fpn`` is called on a list of
leaves feat0 .. feat3 at 16 x 24, 8 x 12, 4 x 6, 2 x 3, B = 2.  It replaces the list's entries in place and returns it:
out = [z0, h3, h4, h5].  loss = sum_i (out_i * G_i).sum(); loss.backward() leaves the gradients in the leaves and in every
parameter.  Stored (float64): feat<i>, G<i>, every parameter under its key p:<name> and the gradients g_feat<i>, g:<name>."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(root):
    sys.path.insert(0, root)
    from models.nets.keypoint_fpn_fusion import KeypointFPNFusion
    ns = types.SimpleNamespace
    names = ['level2', 'level3', 'level4', 'level5']
    widths = [8, 16, 24, 32]
    C = 8
    cfg = ns(MODEL=ns(KFNs=names, OUT_CHANNELS=C))
    spec = {k: ns(stride=4 << i, channels=widths[i]) for i, k in enumerate(names)}
    torch.manual_seed(22)
    m = KeypointFPNFusion(cfg, spec).double()
    rng = np.random.Generator(np.random.PCG64(23))
    B = 2
    sizes = [(16 >> i, 24 >> i) for i in range(4)]
    feats = [torch.from_numpy(rng.standard_normal((B, widths[i]) + sizes[i])).requires_grad_(True) for i in range(4)]
    G = [torch.from_numpy(rng.standard_normal((B, C) + sizes[i])) for i in range(4)]
    res = m._fpn(list(feats))
    assert len(res) == 4 and all(tuple(o.shape) == (B, C) + sizes[i] for i, o in enumerate(res))
    sum((o * g).sum() for o, g in zip(res, G)).backward()
    out = {}
    for i in range(4):
        out['feat%d' % i], out['g_feat%d' % i], out['G%d' % i] = feats[i].detach().numpy(), feats[i].grad.numpy(), G[i].numpy()
    n = 0
    for k, p in m.named_parameters():
        if k.startswith('kfpn_'):
            assert p.grad is not None, k
            out['p:' + k], out['g:' + k] = p.detach().numpy(), p.grad.numpy()
            n += 1
    assert n == 4 * 2 + 3 * 2 + 3                                             # head weight + bias, proj weight + bias, up weight
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in out.values())
    for k in sorted(out):
        print('%-36s %-16s max |v| %.4e' % (k, out[k].shape, np.abs(out[k]).max()))
    path = os.path.join(HERE, 'neck_fpn_grad_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
