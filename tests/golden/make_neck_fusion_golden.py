#!/usr/bin/env python
"""Reference-run fixture of the neck fusion backward: tests/golden/neck_fusion_grad_cases.npz.

    python tests/golden/make_neck_fusion_golden.py <root of the reference checkout>

RUNS the reference's KeypointFPNFusion (models/nets/keypoint_fpn_fusion.py) on the CPU in fp64; this script contains no reference
source.  The module is built with a stand-in config - OUT_CHANNELS = 8 and the KFN levels 2, 3, 4, 5 (strides 4 .. 32), which give
the three fused operands fusion_up3 / 4 / 5 their chains of 1 / 2 / 3 transposed convs, six weights in all - and the instance's
``_fpn`` is replaced by the identity, so that its own ``forward`` (lines 62-69: the transposed-conv chains, the detached softmax
product, the in-place sum) runs on given leaves: z0 at 16 x 24 and h3 / h4 / h5 at 8 x 12 / 4 x 6 / 2 x 3, B = 2.  The module adds
into out[0] in place, so it gets ``z0.clone()``.  loss = (z * G).sum(); loss.backward() leaves the gradients in the leaves and in
the weights.  Stored (float64): z0, h3, h4, h5, G, the weights w<L>_<j>, and the gradients g_z0, g_h3, g_h4, g_h5, gw<L>_<j>."""
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
    cfg = ns(MODEL=ns(KFNs=names, OUT_CHANNELS=8))
    spec = {k: ns(stride=4 << i, channels=8) for i, k in enumerate(names)}
    torch.manual_seed(20)
    m = KeypointFPNFusion(cfg, spec).double()
    m._fpn = lambda x: x
    rng = np.random.Generator(np.random.PCG64(21))
    B, C = 2, 8
    sizes = {'z0': (16, 24), 'h3': (8, 12), 'h4': (4, 6), 'h5': (2, 3)}
    leaves = {k: torch.from_numpy(rng.standard_normal((B, C) + hw)).requires_grad_(True) for k, hw in sizes.items()}
    G = torch.from_numpy(rng.standard_normal((B, C) + sizes['z0']))
    z = m([leaves['z0'].clone(), leaves['h3'], leaves['h4'], leaves['h5']])
    (z * G).sum().backward()
    out = {'G': G.numpy()}
    for k, t in leaves.items():
        out[k], out['g_' + k] = t.detach().numpy(), t.grad.numpy()
    n = 0
    for L in (3, 4, 5):
        for j in range(L - 2):
            w = getattr(m, 'fusion_up%d' % L)[j].conv_tran.weight
            assert tuple(w.shape) == (C, C, 4, 4) and w.grad is not None
            out['w%d_%d' % (L, j)], out['gw%d_%d' % (L, j)] = w.detach().numpy(), w.grad.numpy()
            n += 1
    assert n == 6 and all(v.dtype == np.float64 and np.isfinite(v).all() for v in out.values())
    for k in sorted(out):
        print('%-8s %-16s max |v| %.4e' % (k, out[k].shape, np.abs(out[k]).max()))
    path = os.path.join(HERE, 'neck_fusion_grad_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
