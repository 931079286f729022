"""Where TrainableHeads' default grad_scale comes from: the fp64 reference gradient (tests/head_backward_ref.py, R64) of the heads on
the loss-gradient fixture's labels (tests/loss_cases.py: fx_b1 and fx_b2_empty, the two on the 24 x 40 map, which a 96 x 160 image gives) with synth_state_dict weights.  The
forward (random image -> z, h1, h2, logits) and dL/dlogits (rtm3d_loss_grad) run on the device; the chain is the CPU's fp64 one.
Prints the largest magnitude of every gradient activation and the largest power of two S with S * max <= 65504 / 16.

    python tools/gpu_head_grad_scale.py >> profiles/head_backward.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtm3d_amd  # noqa: E402
from rtm3d_amd import plan as plan_mod  # noqa: E402
from rtm3d_amd.loss import RTM3DLoss  # noqa: E402
from rtm3d_amd.weights import synth_state_dict, head_table  # noqa: E402
from tests import head_backward_ref as ref, loss_cases  # noqa: E402


def main():
    cfg = rtm3d_amd.kitti_config('DLA-34')
    sd = synth_state_dict('DLA-34', seed=0, style='trained')
    model = rtm3d_amd.create_model(cfg).to('cuda')
    model.load_state_dict(sd)
    model.use_graph = False
    table = head_table('rtm3d', 3)
    fold = lambda k, seq: plan_mod.fold_bn(sd, 'detect_header.%s.%d' % (seq, 3 * (k - 1)), 'detect_header.%s.%d' % (seq, 3 * (k - 1) + 1))[0]
    wf = [None] + [[fold(k, seq).astype(np.float16) for seq, _, _ in table] for k in (1, 2)]
    wo = [plan_mod.fold_bn(sd, 'detect_header.%s.%s' % (seq, last))[0].astype(np.float16) for seq, last, _ in table]
    ones = [None] + [[np.ones(256, np.float32)] * 4] * 2
    fn = RTM3DLoss(cfg)
    top = {}
    print('grad_scale: fp64 reference gradient of the heads, synth_state_dict(seed 0, trained) weights, loss-gradient fixture labels')
    for name in ('fx_b1', 'fx_b2_empty'):
        c = loss_cases.make(name)
        B, H, W = c['B'], c['H'], c['W']
        Hp, Wp = 4 * H, 4 * W
        x = torch.from_numpy(np.random.default_rng(c['seed']).standard_normal((B, 3, Hp, Wp)).astype(np.float32)).cuda()
        logits = model.forward_logits(x)
        plan = model._plan_for(B, Hp, Wp, x.device)
        acts = [np.ascontiguousarray(plan.download(plan.plan.named[nm]).transpose(0, 2, 3, 1)).astype(np.float16) for nm in ('z', 'h1', 'h2')]
        dl = fn.grad(logits, loss_cases.batch(c))
        case = {'B': B, 'H': H, 'W': W, 'K': (3, 16, 2, 2), 'num_conv': 2, 'S': 1.0, 'input_grad': True, 'acts': acts, 'wf': wf, 'wo': wo,
                'scale': ones, 'dlogits': [d.cpu().numpy() for d in dl]}
        r = ref.flat(ref.chain(case, False))
        row = {'go': max(np.abs(r['go[%d]' % g]).max() for g in range(4)), 'dh2': np.abs(r['dh2']).max(), 'dh1': np.abs(r['dh1']).max(), 'dz': np.abs(r['dz']).max()}
        print('  %-12s B = %d, map %d x %d: max |go| %.4e  |dh2| %.4e  |dh1| %.4e  |dz| %.4e'
              % (name, B, H, W, row['go'], row['dh2'], row['dh1'], row['dz']))
        for k, v in row.items():
            top[k] = max(top.get(k, 0.0), float(v))
    big = max(top.values())
    S = 2.0 ** np.floor(np.log2(65504.0 / 16.0 / big))
    print('  largest gradient activation %.4e (%s): the largest power of two S with S * max <= 65504 / 16 = 4094 is 2 ** %d = %g'
          % (big, max(top, key=top.get), int(np.log2(S)), S))


if __name__ == '__main__':
    main()
