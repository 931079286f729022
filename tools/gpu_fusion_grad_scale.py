"""Where TrainableFusion's default fusion_scale comes from: the fp64 reference gradient (tests/neck_backward_ref.py, R64) of the
neck's fusion on the loss-gradient fixture's labels (tests/loss_cases.py: fx_b1 and fx_b2_empty, the two on the 24 x 40 map, which
a 96 x 160 image gives) with synth_state_dict weights, through the model: the forward (random image -> kfpn_h*, the up maps, u*,
z, h1, h2, logits) and dL/dlogits (rtm3d_loss_grad) run on the device, dz is the heads' fp64 chain (tests/head_backward_ref.py)
and the fusion chain behind it is the CPU's fp64 one.  Prints the largest |du_i| and |dX| of every layer, unscaled; for each
candidate T the share of the non-zero reference elements that land below fp16's smallest normal once multiplied by S T
(S = head_train.DEFAULT_GRAD_SCALE); and the largest power of two T with S T max <= 65504 / 16.

    python tools/gpu_fusion_grad_scale.py >> profiles/neck_backward.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtm3d_amd  # noqa: E402
from rtm3d_amd import plan as plan_mod  # noqa: E402
from rtm3d_amd.head_train import DEFAULT_GRAD_SCALE  # noqa: E402
from rtm3d_amd.loss import RTM3DLoss  # noqa: E402
from rtm3d_amd.weights import synth_state_dict, head_table  # noqa: E402
from tests import head_backward_ref as href, neck_backward_ref as nref, loss_cases  # noqa: E402

FP16_MIN_NORMAL = 2.0 ** -14
CANDIDATES = [2.0 ** k for k in range(0, 17, 2)]


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
    wup = [[plan_mod._np(sd, 'kfpn_fusion.fusion_up%d.%d.conv_tran.weight' % (l + 3, j)).astype(np.float16) for j in range(l + 1)] for l in range(3)]
    fn = RTM3DLoss(cfg)
    S = DEFAULT_GRAD_SCALE
    top, vals = {}, []
    print('fusion_scale: fp64 reference gradient of the fusion, synth_state_dict(seed 0, trained) weights, loss-gradient fixture labels')
    for name in ('fx_b1', 'fx_b2_empty'):
        c = loss_cases.make(name)
        B, H, W = c['B'], c['H'], c['W']
        Hp, Wp = 4 * H, 4 * W
        x = torch.from_numpy(np.random.default_rng(c['seed']).standard_normal((B, 3, Hp, Wp)).astype(np.float32)).cuda()
        logits = model.forward_logits(x)
        plan = model._plan_for(B, Hp, Wp, x.device)
        nhwc = lambda s: np.ascontiguousarray(plan.download(s).transpose(0, 2, 3, 1)).astype(np.float16)
        dl = fn.grad(logits, loss_cases.batch(c))
        hcase = {'B': B, 'H': H, 'W': W, 'K': (3, 16, 2, 2), 'num_conv': 2, 'S': 1.0, 'input_grad': True,
                 'acts': [nhwc(plan.plan.named[nm]) for nm in ('z', 'h1', 'h2')], 'wf': wf, 'wo': wo, 'scale': ones,
                 'dlogits': [d.cpu().numpy() for d in dl]}
        dz = href.chain(hcase, False)['dz'].permute(0, 2, 3, 1).numpy()          # fp64, unscaled
        ops = {op.get('name'): op for op in plan.plan.ops}
        case = {'B': B, 'H': H, 'W': W, 'levels': 3, 'C': 256, 'S': 1.0, 'T': 1.0, 'dz': dz, 'w': wup,
                'us': [nhwc(plan.plan.named['u%d' % (l + 3)]) for l in range(3)],
                'xs': [[nhwc(ops['fusion_up%d.%d' % (l + 3, j)]['inp'][0]) for j in range(l + 1)] for l in range(3)]}
        r = nref.flat(nref.chain(case, False))
        print('  %-12s B = %d, map %d x %d: max |dz| %.4e' % (name, B, H, W, np.abs(dz).max()))
        for key in sorted(k for k in r if not k.startswith('dw')):
            v = np.abs(r[key])
            lvl = int(key[3]) + 3
            what = 'du%d' % lvl if key.startswith('du') else 'dX of fusion_up%d.%s' % (lvl, key[-2])
            print('    %-22s max %.4e   median of the non-zero %.4e' % (what, v.max(), np.median(v[v > 0])))
            top[what] = max(top.get(what, 0.0), float(v.max()))
            vals.append(v[v > 0].ravel())
    vals = np.concatenate(vals)
    big = max(top.values())
    print('  S = grad_scale = 2 ** %d.  Share of the %d non-zero reference elements (every du and dX above) below fp16\'s smallest normal'
          % (int(np.log2(S)), vals.size))
    print('  2 ** -14 once multiplied by S T, and the largest scaled element:')
    for T in CANDIDATES:
        print('    T = 2 ** %-2d  below-normal share %.4f   S T max = %.4e%s'
              % (int(np.log2(T)), float((vals * S * T < FP16_MIN_NORMAL).mean()), S * T * big, '   (> 65504 / 16)' if S * T * big > 65504.0 / 16.0 else ''))
    T = 2.0 ** np.floor(np.log2(65504.0 / 16.0 / (S * big)))
    print('  largest gradient activation %.4e (%s): the largest power of two T with S T max <= 65504 / 16 = 4094 is 2 ** %d = %g'
          % (big, max(top, key=top.get), int(np.log2(T)), T))


if __name__ == '__main__':
    main()
