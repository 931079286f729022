#!/usr/bin/env python
"""Reference-run fixture of the loss gradient: tests/golden/loss_grad_cases.npz.

    python tests/golden/make_loss_grad_golden.py <root of the reference checkout>

RUNS the reference on the CPU for every case of tests/loss_cases.FIXTURE_CASES, with the stand-ins of make_loss_golden.py (its
import_reference and config; this script contains no reference source either).  The targets are the ones the reference's own
_build_targets made, as tests/golden/loss_cases.npz stores them.  The four logit maps are leaves that require grad; the
reference's RTM3DLoss.__call__ (models/rtm3d_loss.py:268-340) gets ``leaf.clone()`` of each, because its sigmoid_hm works in
place, and ``loss.backward()`` leaves the gradients in the leaves - once with fp32 tensors, as train.py does, and once with
every tensor .double().  Stored per case: g0..g3_f32 (float32) and g0..g3_f64 (float64), the gradients of the heat map,
ver_coor, m_off and v_off logits.  Two conditions on the inputs are asserted: no heat-map logit lies within 1e-3 of
+-logit(1e-4), so both precisions agree on which cells the clamp cuts, and the zero patterns of the two runs are equal."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_loss_golden as mk  # noqa: E402
from tests import loss_cases  # noqa: E402


def main(root):
    data_utils, ParamList, RTM3DLoss, DatasetReader = mk.import_reference(root)
    stored = np.load(os.path.join(HERE, 'loss_cases.npz'), allow_pickle=False)
    edge = float(np.log(1e-4 / (1 - 1e-4)))
    out = {}
    for name in loss_cases.FIXTURE_CASES:
        c = loss_cases.make(name)
        cfg = mk.config(c['alpha'], c['beta'])
        tg = {f: stored[name + '/' + f] for f in mk.FIELDS}
        tg.update(img_id=c['img_id'], mask=c['cls'] >= 0, noise_mask=c['noise'] != 0)
        logits = loss_cases.logits(c)
        assert (np.abs(np.abs(logits[0].astype(np.float64)) - abs(edge)) > 1e-3).all(), name
        grads = {}
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            t = ParamList((c['W'] * 4, c['H'] * 4))
            for k, v in tg.items():
                v = torch.from_numpy(np.ascontiguousarray(v))
                t.add_field(k, v.to(dt) if v.is_floating_point() else v)
            leaves = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in logits]
            loss, _ = RTM3DLoss(cfg)([leaf.clone() for leaf in leaves], t)
            loss.backward()
            grads[tag] = [(leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)).detach().numpy().copy() for leaf in leaves]
        for k in range(4):
            a, b = grads['f32'][k], grads['f64'][k]
            assert a.dtype == np.float32 and b.dtype == np.float64 and np.isfinite(a).all() and np.isfinite(b).all(), (name, k)
            assert np.array_equal(a == 0, b == 0), (name, k, 'the zero patterns of the fp32 and the fp64 run differ')
            out['%s/g%d_f32' % (name, k)], out['%s/g%d_f64' % (name, k)] = a, b
            print(name, 'map', k, 'nonzero', int((b != 0).sum()), 'max |g|', np.abs(b).max(), 'max |f32 - f64|', np.abs(a - b).max())
    path = os.path.join(HERE, 'loss_grad_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
