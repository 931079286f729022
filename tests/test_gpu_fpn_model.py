"""TrainableNeck through the model (rtm3d_amd/fpn_train.py): DLA-34, B = 2, a 64 x 96 image (16 x 24 map), synth_state_dict weights.

The forward is the model's own plan of the training lowering, so the logits must be its bits; the parameter gradients are held to
the bar of tests/test_gpu_neck_backward.py - max(4 x Q16's distance from R64, floor) - with R64 (tests/fpn_backward_ref.py plus the
factor rule) taken on the activations downloaded from the plan.  The floor of a factor-rule product follows from its factors: an
error of at most f in every dA element is at most f x max_j sum_i |Wp[j][i]| in dA Wp^T, and likewise for the other three.
"""
import numpy as np
import pytest

from tests import fpn_backward_ref as ref
from tests.test_gpu_neck_backward import _bits

pytestmark = pytest.mark.gpu

_MODEL = {}
B, H, W = 2, 64, 96


def _fixture():
    if not _MODEL:
        import torch
        from rtm3d_amd.weights import synth_state_dict
        from tests import loss_cases
        sd = synth_state_dict('DLA-34', seed=0, style='trained')
        x = torch.from_numpy(np.random.Generator(np.random.PCG64(11)).standard_normal((B, 3, H, W)).astype(np.float32)).cuda()
        rng = np.random.default_rng(7)
        case = loss_cases._case(B, H // 4, W // 4, sum([loss_cases._scene(rng, b, 4, H // 4, W // 4) for b in range(B)], []))
        _MODEL.update(sd=sd, x=x, case=case)
    return _MODEL


def _new_model(sd=None):
    import rtm3d_amd
    f = _fixture()
    m = rtm3d_amd.create_model(rtm3d_amd.kitti_config('DLA-34')).to('cuda')
    m.load_state_dict(f['sd'] if sd is None else sd)
    m.use_graph = False
    return m


def _model_case(neck, st):
    """The chain's inputs read back from the plan of the last forward and from the stages in front of the FPN."""
    from rtm3d_amd import fpn_train as ft
    rplan = st['plan']
    ops = {op.get('name'): op for op in rplan.plan.ops}
    nhwc = lambda s: np.ascontiguousarray(rplan.download(s).transpose(0, 2, 3, 1)).astype(np.float16)
    names = ft.conv_launch_names()
    fb = st['fst']['fb']
    dz = neck.heads.input_grad().cpu().numpy()
    A = [a.detach().half().cpu().numpy() for a in neck._A] + [neck._params['kfpn_fusion.kfpn_head5.weight'].detach().half().cpu().numpy().reshape(256, -1)]
    return {'B': B, 'H': H // 4, 'W': W // 4, 'C': 256, 'S': neck.S, 'T': neck.T, 'U': neck.U, 'want_slices': None, 'dz': dz,
            'ncat': [nhwc(ops[names[k]]['inp'][0]) for k in range(3)], 'h': [nhwc(rplan.plan.named['kfpn_h%d' % (k + 3)]) for k in range(3)],
            'feat3': nhwc(rplan.plan.named['feat3']), 'F': [fb.dx[l][0][:, 1:-1, 1:-1].cpu().numpy() for l in range(3)], 'A': A,
            'wup': [neck._params['kfpn_fusion.kfpn_up%d.conv_tran.weight' % L].detach().half().cpu().numpy() for L in (3, 4, 5)]}


def _reference_params(neck, res, floors=None):
    """{parameter name: fp64 gradient} of a chain() result through the factor rule on the fp32 parameters; with ``floors`` (the
    chain's per-tensor floors) the floors of the same tensors instead."""
    p = lambda n: neck._params['kfpn_fusion.' + n].detach().double().cpu().numpy()
    out = {}
    for k, L in enumerate((3, 4, 5)):
        wh, wp, bp = p('kfpn_head%d.weight' % (L - 1))[:, :, 0, 0], p('kfpn_proj%d.weight' % L)[:, :, 0, 0], p('kfpn_proj%d.bias' % L)
        if floors is None:
            dwh, dwp, dbh, dbp = ref.factor_rule(res['dA'][k].numpy(), res['db'][k].numpy(), wh, wp, bp)
            out['kfpn_up%d.conv_tran.weight' % L] = res['dwup'][k].numpy()
        else:
            fa, fb = floors['dA[%d]' % k], floors['db[%d]' % k]
            dwh = fa * np.abs(wp).sum(1).max() + fb * np.abs(bp).max()
            dwp, dbh, dbp = fa * np.abs(wh).sum(0).max(), fb, fb * np.abs(wh).sum(0).max()
            out['kfpn_up%d.conv_tran.weight' % L] = floors['dwup[%d]' % k]
        out['kfpn_head%d.weight' % (L - 1)], out['kfpn_head%d.bias' % (L - 1)] = dwh, dbh
        out['kfpn_proj%d.weight' % L], out['kfpn_proj%d.bias' % L] = dwp, dbp
    if floors is None:
        out['kfpn_head5.weight'], out['kfpn_head5.bias'] = res['dA'][3].numpy(), res['db'][3].numpy()
    else:
        out['kfpn_head5.weight'], out['kfpn_head5.bias'] = floors['dA[3]'], floors['db[3]']
    return out


def _bar(tag, got, r64, q16, floors):
    worst = 0.0
    for name in sorted(got):
        g, r, q = (np.asarray(a, np.float64).reshape(-1) for a in (got[name], r64[name], q16[name]))
        dq, dd = float(np.abs(q - r).max()), float(np.abs(g - r).max())
        ratio = dd / dq if dq > 0 else 0.0
        print('%s %s: max|ref| %.3e  Q16-R64 %.3e  device-R64 %.3e  ratio %.3f  floor %.3e' % (tag, name, np.abs(r).max(), dq, dd, ratio, floors[name]))
        assert np.isfinite(g).all(), name
        assert dd <= max(4.0 * dq, floors[name]), (name, dd, dq, floors[name])
        worst = max(worst, ratio)
    print('%s worst ratio %.3f' % (tag, worst))


def test_model_forward_backward_refresh_and_training():
    import torch
    from rtm3d_amd import head_train as ht, fpn_train as ft, optim, plan as plan_mod
    from rtm3d_amd.loss import RTM3DLoss
    from tests import loss_cases
    f = _fixture()
    x = f['x']
    plain = _new_model()
    want_logits = _bits(plain.forward_logits(x, neck_fold=False))
    default_logits = _bits(plain.forward_logits(x))
    keys = list(plain._plans)
    assert len(keys) == 2 and keys[0][-1] == 'neck_fold=False' and keys[1] == (B, H, W, x.device.index)      # a key of its own; the default key as it was

    model = _new_model()
    neck = ft.TrainableNeck(ht.TrainableHeads(model, input_grad=True))
    names = [n for n, _ in neck.named_parameters()]
    own = ft.param_names()
    assert names[-17:] == own and len(set(names)) == len(names) and set(neck.state_dict()) >= set(names)
    batch = loss_cases.batch(f['case'])
    fn = RTM3DLoss(model.config)
    logits = neck(x)
    assert all(t.grad_fn is not None for t in logits)
    assert _bits(logits) == want_logits                                        # the three refreshes reproduce the host packers' bytes
    loss, _ = fn(logits, batch)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in neck.named_parameters()}
    for k, v in grads.items():
        assert v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    assert neck.nonfinite() == 0

    # against R64 on the plan's own saved activations, the heads' dz and the fusion's terms
    st = neck._last
    case = _model_case(neck, st)
    q = ref.chain(case, True)
    r = ref.chain(case, False)
    fl = ref.floors(q)
    r64, q16, floors = _reference_params(neck, r), _reference_params(neck, q), _reference_params(neck, None, fl)
    _bar('model', {k: grads['kfpn_fusion.' + k].cpu().numpy() for k in r64}, r64, q16, floors)
    ig16, ig32 = neck.input_grads(), neck.input_grads(fp32=True)
    assert sorted(ig16) == ['feat0', 'feat1', 'feat2', 'feat3', 'kfpn_h3', 'kfpn_h4', 'kfpn_h5', 'z0']
    assert ig16['z0'].data_ptr() == neck.heads.input_grad().data_ptr()
    fr, fq = ref.flat(r, neck.S * neck.U), ref.flat(q)
    nchw = lambda t: t.permute(0, 3, 1, 2).float().cpu().numpy()
    acts = {'dfeat3': nchw(ig16['feat3'])}
    want_acts, q_acts, fl_acts = {'dfeat3': fr['dfeat3']}, {'dfeat3': fq['dfeat3']}, {'dfeat3': fl['dfeat3']}
    for k in range(3):
        acts['g[%d]' % k] = nchw(ig16['kfpn_h%d' % (k + 3)])
        acts['dfeat%d' % k] = nchw(ig16['feat%d' % k])
        want_acts['g[%d]' % k], q_acts['g[%d]' % k], fl_acts['g[%d]' % k] = fr['g[%d]' % k], fq['g[%d]' % k], fl['g[%d]' % k]
        want_acts['dfeat%d' % k], q_acts['dfeat%d' % k], fl_acts['dfeat%d' % k] = fr['D[%d]' % k][:, 256:], fq['D[%d]' % k][:, 256:], fl['D[%d]' % k]
        assert tuple(ig32['feat%d' % k].shape) == acts['dfeat%d' % k].shape and ig32['feat%d' % k].dtype == torch.float32
    _bar('model', acts, want_acts, q_acts, fl_acts)
    assert float(ig32['feat3'].abs().max()) > 0

    # the explicit call on the same forward: the same bits as autograd left in the leaves
    dl = fn.grad([t.detach() for t in logits], batch)
    explicit = neck.backward_explicit(st, dl)
    for k in grads:
        assert explicit[k].cpu().numpy().tobytes() == grads[k].cpu().numpy().tobytes(), k

    # a stale plan is refused: another forward of the shape overwrote the saved activations
    stale = neck(x)
    neck(x)
    with pytest.raises(RuntimeError, match='stale plan'):
        fn(stale, batch)[0].backward()

    # every neck parameter a multiple of 2 ** -10 in [-1, 1]: the fp64 composition is exact in any summation order, so the device's
    # A and b are the host's and the refreshed logits are a fresh model's, bit for bit
    with torch.no_grad():
        for n, p in neck.named_parameters():
            if n.startswith('kfpn_fusion.'):
                p.copy_((p * 1024).round().clamp_(-1024, 1024) / 1024)
    exact = _bits(neck(x))
    fresh = _new_model()
    neck.export_to(fresh)
    assert _bits(fresh.forward_logits(x, neck_fold=False)) == exact
    assert exact != want_logits

    # ten optimiser steps on one batch
    for p in neck.parameters():
        p.grad = None
    before = {n: neck._params[n].detach().clone() for n in own}
    solver = optim.Solver(neck, model.config)
    losses = []
    for _ in range(10):
        loss, _ = fn(neck(x), batch)
        losses.append(loss.detach())
        solver.step(loss)
    neck(x)
    losses = [float(v) for v in losses]
    print('ten Adamax steps on one batch, heads + fusion + FPN: loss %s' % ' '.join('%.4f' % v for v in losses))
    assert losses[-1] < losses[0]
    for n in own:
        assert not torch.equal(before[n], neck._params[n].detach()), n        # the FPN parameters have moved
    # after real steps the device's fp64 products may round to fp32 one step away from the host's: every packed fp16 weight equals
    # the host packer's or is adjacent to it
    sd = {k: v.detach().cpu() for k, v in neck.state_dict().items()}
    off = 0
    for k, L in enumerate((3, 4, 5)):
        w2 = plan_mod.fold_bn(sd, 'kfpn_fusion.kfpn_proj%d' % L)[0]
        wh = plan_mod.fold_bn(sd, 'kfpn_fusion.kfpn_head%d' % (L - 1))[0]
        host = (wh[:, :, 0, 0].astype(np.float64) @ w2[:, :, 0, 0].astype(np.float64)).astype(np.float32).astype(np.float16)
        dev = neck._wr[k].cpu().numpy().T
        d = np.abs(host.view(np.int16).astype(np.int32) - dev.view(np.int16).astype(np.int32))
        d = np.where((host == 0) & (dev == 0), 0, d)                          # (+0 and -0 are the same weight)
        off += int((d != 0).sum())
        assert d.max() <= 1, (L, int(d.max()))
    print('packed fp16 weights of the composed convs one step from the host packer after ten steps: %d of %d' % (off, 256 * (320 + 384 + 512)))
    assert neck.nonfinite() == 0

    # a model that never met TrainableNeck is untouched
    assert _bits(plain.forward_logits(x, neck_fold=False)) == want_logits and _bits(plain.forward_logits(x)) == default_logits


def test_model_refusals():
    from rtm3d_amd import head_train as ht, fpn_train as ft
    f = _fixture()
    m = _new_model()
    m.use_graph = True
    neck = ft.TrainableNeck(ht.TrainableHeads(m, input_grad=True))
    with pytest.raises(NotImplementedError, match='replays a captured graph'):
        neck(f['x'])
    m = _new_model()
    neck = ft.TrainableNeck(ht.TrainableHeads(m, input_grad=True))
    folded = m._plan_for(B, H, W, neck.device, 'dense', 'fp16')
    with pytest.raises(NotImplementedError, match='took the neck fold'):
        neck._state(folded, {'hst': {'shape': (B, H, W)}})
    with pytest.raises(ValueError, match='without input_grad=True'):
        ft.TrainableNeck(ht.TrainableHeads(m))
    with pytest.raises(ValueError, match='neck_fold'):
        m._plan_for(B, H, W, neck.device, 'peaks', 'fp16', neck_fold=False)
