"""Where TrainableNeck's default fpn_scale comes from: the fp64 reference gradient (tests/fpn_backward_ref.py, R64) of the neck's FPN
half on the loss-gradient fixture's labels (tests/loss_cases.py: fx_b1 and fx_b2_empty, the two on the 24 x 40 map, which a 96 x 160
image gives) with synth_state_dict weights, through the model: the forward on the TRAINING lowering (random image -> feat*, the
concat tensors, kfpn_h*, the fusion's maps, z, h1, h2, logits) and dL/dlogits (rtm3d_loss_grad) run on the device; dz is the heads'
fp64 chain (tests/head_backward_ref.py), the fusion-path terms are the fusion's fp64 chain (tests/neck_backward_ref.py) and the FPN
chain behind them is the CPU's fp64 one.  Prints the largest |D_k|, |E_k|, |g_k| and |d feat3|, unscaled; for each candidate U the
share of the non-zero reference elements that land below fp16's smallest normal once multiplied by S U
(S = head_train.DEFAULT_GRAD_SCALE); and the largest power of two U with S U max <= 65504 / 16.

    python tools/gpu_fpn_grad_scale.py >> profiles/neck_fpn_backward.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtm3d_amd  # noqa: E402
from rtm3d_amd import plan as plan_mod, fpn_train  # noqa: E402
from rtm3d_amd.head_train import DEFAULT_GRAD_SCALE  # noqa: E402
from rtm3d_amd.loss import RTM3DLoss  # noqa: E402
from rtm3d_amd.weights import synth_state_dict, head_table  # noqa: E402
from tests import head_backward_ref as href, neck_backward_ref as nref, fpn_backward_ref as fref, loss_cases  # noqa: E402

FP16_MIN_NORMAL = 2.0 ** -14
CANDIDATES = [2.0 ** k for k in range(0, 13, 2)]


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
    wfu = [[plan_mod._np(sd, 'kfpn_fusion.fusion_up%d.%d.conv_tran.weight' % (l + 3, j)).astype(np.float16) for j in range(l + 1)] for l in range(3)]
    params = {n[len('kfpn_fusion.'):]: plan_mod._np(sd, n) for n in fpn_train.param_names()}
    A = [fref.compose(params, k + 3)[0].astype(np.float32).astype(np.float16) for k in range(3)] + [params['kfpn_head5.weight'][:, :, 0, 0].astype(np.float16)]
    wup = [params['kfpn_up%d.conv_tran.weight' % (k + 3)].astype(np.float16) for k in range(3)]
    fn = RTM3DLoss(cfg)
    S = DEFAULT_GRAD_SCALE
    top, vals = {}, []
    print('fpn_scale: fp64 reference gradient of the FPN, synth_state_dict(seed 0, trained) weights, loss-gradient fixture labels')
    for name in ('fx_b1', 'fx_b2_empty'):
        c = loss_cases.make(name)
        B, H, W = c['B'], c['H'], c['W']
        Hp, Wp = 4 * H, 4 * W
        x = torch.from_numpy(np.random.default_rng(c['seed']).standard_normal((B, 3, Hp, Wp)).astype(np.float32)).cuda()
        logits = model.forward_logits(x, neck_fold=False)
        plan = model._plan_for(B, Hp, Wp, x.device, neck_fold=False)
        nhwc = lambda s: np.ascontiguousarray(plan.download(s).transpose(0, 2, 3, 1)).astype(np.float16)
        dl = fn.grad(logits, loss_cases.batch(c))
        hcase = {'B': B, 'H': H, 'W': W, 'K': (3, 16, 2, 2), 'num_conv': 2, 'S': 1.0, 'input_grad': True,
                 'acts': [nhwc(plan.plan.named[nm]) for nm in ('z', 'h1', 'h2')], 'wf': wf, 'wo': wo, 'scale': ones,
                 'dlogits': [d.cpu().numpy() for d in dl]}
        dz = href.chain(hcase, False)['dz'].permute(0, 2, 3, 1).numpy()          # fp64, unscaled
        ops = {op.get('name'): op for op in plan.plan.ops}
        ncase = {'B': B, 'H': H, 'W': W, 'levels': 3, 'C': 256, 'S': 1.0, 'T': 1.0, 'dz': dz, 'w': wfu,
                 'us': [nhwc(plan.plan.named['u%d' % (l + 3)]) for l in range(3)],
                 'xs': [[nhwc(ops['fusion_up%d.%d' % (l + 3, j)]['inp'][0]) for j in range(l + 1)] for l in range(3)]}
        fus = nref.chain(ncase, False)
        names = fpn_train.conv_launch_names()
        case = {'B': B, 'H': H, 'W': W, 'C': 256, 'S': 1.0, 'T': 1.0, 'U': 1.0, 'dz': dz, 'A': A, 'wup': wup,
                'ncat': [nhwc(ops[names[k]]['inp'][0]) for k in range(3)], 'h': [nhwc(plan.plan.named['kfpn_h%d' % (k + 3)]) for k in range(3)],
                'feat3': nhwc(plan.plan.named['feat3']), 'F': [fus['dx'][l][0].permute(0, 2, 3, 1).numpy() for l in range(3)]}
        r = fref.flat(fref.chain(case, False))
        print('  %-12s B = %d, map %d x %d: max |dz| %.4e' % (name, B, H, W, np.abs(dz).max()))
        for key in sorted(k for k in r if k[0] in 'DEg' or k == 'dfeat3'):
            v = np.abs(r[key])
            print('    %-8s max %.4e   median of the non-zero %.4e' % (key, v.max(), np.median(v[v > 0])))
            top[key] = max(top.get(key, 0.0), float(v.max()))
            vals.append(v[v > 0].ravel())
    vals = np.concatenate(vals)
    big = max(top.values())
    print('  S = grad_scale = 2 ** %d.  Share of the %d non-zero reference elements (every map above) below fp16\'s smallest normal'
          % (int(np.log2(S)), vals.size))
    print('  2 ** -14 once multiplied by S U, and the largest scaled element:')
    for U in CANDIDATES:
        print('    U = 2 ** %-2d  below-normal share %.4f   S U max = %.4e%s'
              % (int(np.log2(U)), float((vals * S * U < FP16_MIN_NORMAL).mean()), S * U * big, '   (> 65504 / 16)' if S * U * big > 65504.0 / 16.0 else ''))
    U = 2.0 ** np.floor(np.log2(65504.0 / 16.0 / (S * big)))
    print('  largest gradient activation %.4e (%s): the largest power of two U with S U max <= 65504 / 16 = 4094 is 2 ** %d = %g'
          % (big, max(top, key=top.get), int(np.log2(U)), U))


if __name__ == '__main__':
    main()
