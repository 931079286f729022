"""Neck fusion backward on the device (csrc/neck_backward.hip, rtm3d_amd/neck_train.py) against tests/neck_backward_ref.py.

Exact cases: every tensor holds small integers, so the device must equal the integer result in every output, bit for bit.
Real-valued cases: per tensor, the device's max-abs distance to R64 is at most max(4 x Q16's distance to R64, floor), the floor
being the any-order fp32 summation bound of the tensor's last reduction (neck_backward_ref.chain) - the bar of
tests/test_gpu_head_backward.py.  The measured ratios are in profiles/neck_backward.txt, section 3.
"""
import ctypes

import numpy as np
import pytest

from tests import neck_backward_cases as cases
from tests import neck_backward_ref as ref

pytestmark = pytest.mark.gpu


def _padded(a, P, dev):
    import torch
    B, H, W, C = a.shape
    t = torch.zeros(B, H + 2 * P, W + 2 * P, C, dtype=torch.float16, device=dev)
    t[:, P:P + H, P:P + W] = torch.from_numpy(np.asarray(a, np.float16)).to(dev)
    return t


def _border_zero(t, P):
    import torch
    inner = torch.zeros_like(t, dtype=torch.bool)
    inner[:, P:-P, P:-P] = True
    assert not bool(t.view(torch.int16)[~inner].any()), 'a border byte is not zero'


# --------------------------------------------------------------------------------------------------- one transposed conv, exact
def run_layer(case, want):
    """wgrad + dgrad of one transposed conv through the C entry points -> (dX NHWC, dW, non-finite count, the padded dX map)."""
    import torch
    from rtm3d_amd import _lib, head_train as ht, neck_train as nt
    lib, dev = _lib.load(), torch.device('cuda', torch.cuda.current_device())
    B, Hi, Wi = case['B'], case['Hi'], case['Wi']
    x, dy = _padded(case['x'], 1, dev), _padded(case['dy'], 1, dev)
    dx = torch.zeros(B, Hi + 2, Wi + 2, 256, dtype=torch.float16, device=dev)
    wr = nt.rotate_deconv_weights(torch.from_numpy(case['w']).to(dev))
    dw = torch.full((256, 256, 4, 4), float('nan'), dtype=torch.float32, device=dev)
    want = nt.default_slices() if want is None else want
    n_slices, _ = ht.slices(B * Hi * Wi, want)
    ws = torch.empty(int(lib.rtm3d_neck_backward_workspace_bytes(B, 1, n_slices)) // 4, dtype=torch.float32, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    xm, dym, dxm = (ht.hb_map(t.data_ptr(), 256, 1) for t in (x, dy, dx))
    _lib.check(lib.rtm3d_neck_deconv_wgrad(st, B, Hi, Wi, ctypes.byref(xm), ctypes.byref(dym), case['S'], case['T'], dw.data_ptr(), want,
                                           ws.data_ptr(), ws.numel() * 4, ctr.data_ptr()), 'neck_deconv_wgrad')
    _lib.check(lib.rtm3d_neck_deconv_dgrad(st, B, Hi, Wi, ctypes.byref(dym), wr.data_ptr(), ctypes.byref(dxm)), 'neck_deconv_dgrad')
    torch.cuda.synchronize()
    return dx[:, 1:-1, 1:-1].float().cpu().numpy(), dw.cpu().numpy(), int(ctr.item()), dx


_LAYER = {}


def _layer(cid):
    if cid not in _LAYER:
        spec = dict(cases.INT_LAYERS[cid])
        wants = spec.pop('want')
        case = cases.int_layer(**spec)
        dx, dw = ref.layer_exact(case['x'], case['w'], case['dy'], case['S'] * case['T'])
        cases.check_layer_exact(case, dx, dw)
        _LAYER[cid] = (case, wants, dx, dw)
    return _LAYER[cid]


@pytest.mark.parametrize('cid', sorted(cases.INT_LAYERS))
def test_deconv_exact_integer_cases(cid):
    case, wants, dx, dw = _layer(cid)
    for want in wants:
        gx, gw, bad, dxmap = run_layer(case, want)
        print('%s want_slices %s: dX %d of %d differ (max |ref| %g), dW %d of %d differ (max |ref| %g)'
              % (cid, want, int((gx != dx).sum()), dx.size, np.abs(dx).max(), int((gw != dw).sum()), dw.size, np.abs(dw).max()))
        assert gx.shape == dx.shape and np.array_equal(gx, dx), (cid, want)
        assert gw.shape == dw.shape and np.array_equal(gw, dw), (cid, want)
        assert np.abs(dw).max() > 0 and np.abs(dx).max() > 0
        assert bad == 0
        _border_zero(dxmap, 1)
        ax, aw, _, _ = run_layer(case, want)                                  # the second call: the same bits
        assert ax.tobytes() == gx.tobytes() and aw.tobytes() == gw.tobytes()


# --------------------------------------------------------------------------------------------------- softmax backward
@pytest.mark.parametrize('hw', [(2, 2), (6, 10), (16, 32)])
def test_softmax_backward(hw):
    import torch
    from rtm3d_amd import _lib, head_train as ht
    H, W = hw
    B, T = 2, 4.0
    case = cases.softmax_case(3, B, H, W)
    lib, dev = _lib.load(), torch.device('cuda', torch.cuda.current_device())
    u, dz = _padded(case['u'], 0, dev), _padded(case['dz'], 0, dev)
    du = torch.zeros(B, H + 2, W + 2, 256, dtype=torch.float16, device=dev)
    ws = torch.empty(int(lib.rtm3d_neck_backward_workspace_bytes(B, 1, 1)) // 4, dtype=torch.float32, device=dev)
    maps = lambda m: (_lib.HbMapC * 1)(m)
    _lib.check(lib.rtm3d_neck_softmax_grad(_lib.stream_ptr(dev), B, H, W, 1, ctypes.byref(ht.hb_map(dz.data_ptr(), 256, 0)),
                                           maps(ht.hb_map(u.data_ptr(), 256, 0)), maps(ht.hb_map(du.data_ptr(), 256, 1)), T,
                                           ws.data_ptr(), ws.numel() * 4), 'neck_softmax_grad')
    torch.cuda.synchronize()
    got = du[:, 1:-1, 1:-1].float().cpu().numpy().astype(np.float64)
    _border_zero(du, 1)
    r64 = ref.softmax_grad(ref._nchw(case['u']), T * ref._nchw(case['dz'])).permute(0, 2, 3, 1).numpy()
    q16 = r64.astype(np.float16).astype(np.float64)
    assert np.isfinite(got).all()
    dq, dd = np.abs(q16 - r64).max(), np.abs(got - r64).max()
    print('softmax %dx%d: max|ref| %.3e  Q16-R64 %.3e  device-R64 %.3e  ratio %.3f' % (H, W, np.abs(r64).max(), dq, dd, dd / dq))
    assert dd <= 4.0 * dq
    # the channel of equal values: s = 1 / (H W); the channel with one dominant pixel: s = 1 there, 0 elsewhere
    dzv = case['dz'].astype(np.float64)
    eq = (T * dzv[..., 0] / (H * W)).astype(np.float16).astype(np.float64)
    assert np.abs(got[..., 0] - eq).max() <= np.abs(eq).max() * 2.0 ** -10
    dom = case['u'][..., 1] > 0
    assert dom.sum() == B and np.array_equal(got[..., 1][dom], (T * dzv[..., 1][dom]))
    assert np.abs(got[..., 1][~dom]).max() == 0.0                             # exp(-50) dz is below fp16's smallest subnormal
    assert np.abs(got[..., 2:]).max() > 0


# --------------------------------------------------------------------------------------------------- the whole chain
def run_chain(case, want=None):
    """The chain of a case on the device -> ({name: numpy}, FusionBackward).  want: names of the dW to produce (None: all)."""
    import torch
    from rtm3d_amd import head_train as ht, neck_train as nt
    dev = torch.device('cuda')
    n = case['levels']
    fb = nt.FusionBackward(case['B'], case['H'], case['W'], dev, n, case['S'], case['T'], case['want_slices'])
    keep = [_padded(case['dz'], 0, dev)]
    us, xs, wr, dw = [], [], [], []
    for l in range(n):
        keep.append(_padded(case['us'][l], 0, dev))
        us.append(ht.hb_map(keep[-1].data_ptr(), 256, 0))
        row = []
        for j in range(l + 1):
            keep.append(_padded(case['xs'][l][j], 1, dev))
            row.append(ht.hb_map(keep[-1].data_ptr(), 256, 1))
        xs.append(row)
        wr.append([nt.rotate_deconv_weights(torch.from_numpy(case['w'][l][j]).to(dev)) for j in range(l + 1)])
        dw.append([torch.full((256, 256, 4, 4), float('nan'), dtype=torch.float32, device=dev)
                   if want is None or 'dw[%d][%d]' % (l, j) in want else None for j in range(l + 1)])
    fb.run(ht.hb_map(keep[0].data_ptr(), 256, 0), us, xs, wr, dw)
    torch.cuda.synchronize()
    out = {}
    for l in range(n):
        out['du[%d]' % l] = fb.du[l][:, 1:-1, 1:-1].permute(0, 3, 1, 2)
        for j in range(l + 1):
            out['dx[%d][%d]' % (l, j)] = fb.dx[l][j][:, 1:-1, 1:-1].permute(0, 3, 1, 2)
            out['dw[%d][%d]' % (l, j)] = dw[l][j]
    return {k: v.float().cpu().numpy() for k, v in out.items() if v is not None}, fb


def _within_bar(tag, got, r64, q16, floors):
    worst = 0.0
    for name in sorted(got):
        dq = float(np.abs(q16[name] - r64[name]).max())
        dd = float(np.abs(got[name].astype(np.float64) - r64[name]).max())
        floor = floors.get(name, 0.0)
        ratio = dd / dq if dq > 0 else float('inf') if dd > 0 else 0.0
        print('%s %s: max|ref| %.3e  Q16-R64 %.3e  device-R64 %.3e  ratio %.3f  floor %.3e'
              % (tag, name, np.abs(r64[name]).max(), dq, dd, ratio, floor))
        assert np.isfinite(got[name]).all(), name
        assert dd <= max(4.0 * dq, floor), (name, dd, dq, floor)
        worst = max(worst, ratio if np.isfinite(ratio) else 0.0)
    print('%s worst ratio %.3f' % (tag, worst))


_REAL = {}


def _real(key):
    if key not in _REAL:
        from rtm3d_amd import neck_train as nt
        B, H, W, T = key
        T = nt.DEFAULT_FUSION_SCALE if T is None else T
        case = cases.real_case(5, B, H, W, 1024.0, T)
        q = ref.chain(case, True)
        _REAL[key] = (case, ref.flat(ref.chain(case, False), case['S'] * T), ref.flat(q), ref.floors(q))
    return _REAL[key]


@pytest.mark.parametrize('key', [(2, 8, 8, 1.0), (3, 8, 8, None), (3, 16, 24, 1.0), (2, 16, 24, None)])
def test_chain_real_valued_within_four_times_q16(key):
    case, r64, q16, floors = _real(key)
    got, fb = run_chain(case)
    assert sorted(got) == sorted(r64)
    _within_bar('T=%g %dx%dx%d' % (case['T'], key[0], key[1], key[2]), got, r64, q16, floors)
    assert int(fb.nonfinite.item()) == 0
    for t in fb.du + [m for row in fb.dx for m in row]:
        _border_zero(t, 1)


def test_chain_second_run_and_each_dw_alone():
    case, _, _, _ = _real((2, 8, 8, 1.0))
    full, _ = run_chain(case)
    again, _ = run_chain(case)
    for name in full:
        assert full[name].tobytes() == again[name].tobytes(), name
    for name in ('dw[0][0]', 'dw[2][1]'):
        alone, _ = run_chain(case, want=(name,))
        assert [k for k in alone if k.startswith('dw')] == [name]
        assert alone[name].tobytes() == full[name].tobytes(), name


def test_nonfinite_dz_reaches_the_dws_and_is_counted():
    case, _, _, _ = _real((2, 8, 8, 1.0))
    case = dict(case, dz=case['dz'].copy())
    case['dz'][1, 3, 4, 7] = np.nan
    got, fb = run_chain(case)
    for l in range(3):
        # the last deconv of every chain: output channel 7, the four taps (ky even, kx odd) that meet pixel (3, 4), every ci
        hit = np.isnan(got['dw[%d][%d]' % (l, l)][:, 7])
        assert hit[:, 0::2, 1::2].all() and not hit[:, 1::2, :].any() and not hit[:, :, 0::2].any(), l
        assert np.isfinite(np.delete(got['dw[%d][%d]' % (l, l)], 7, axis=1)).all(), l      # a channel the NaN cannot reach
    assert np.isnan(got['dw[1][0]']).any() and np.isnan(got['dw[2][0]']).any()             # through the dgrad: every channel
    assert int(fb.nonfinite.item()) >= 3 * 256 * 4


# --------------------------------------------------------------------------------------------------- through the model
_MODEL = {}


def _fixture():
    """The model of e2e_dla34_small.npz (its smallest shape: B = 2, 3 x 128 x 256), its input and a label batch; built once."""
    if not _MODEL:
        import torch
        from rtm3d_amd.weights import synth_state_dict
        from tests.util import load_golden
        from tests import loss_cases
        g = load_golden('e2e_dla34_small.npz')
        B, H, W = (int(v) for v in g['shape'])
        sd = synth_state_dict(str(g['backbone']), seed=int(g['seed']), style=str(g['style']), heat_bias=float(g['heat_bias']), heat_gain=float(g['heat_gain']))
        x = torch.from_numpy(np.random.Generator(np.random.PCG64(int(g['img_seed']))).standard_normal((B, 3, H, W)).astype(np.float32)).cuda()
        rng = np.random.default_rng(7)
        case = loss_cases._case(B, H // 4, W // 4, sum([loss_cases._scene(rng, b, 4, H // 4, W // 4) for b in range(B)], []))
        _MODEL.update(sd=sd, x=x, case=case, backbone=str(g['backbone']), shape=(B, H, W))
    return _MODEL


def _new_model(sd=None):
    import rtm3d_amd
    f = _fixture()
    m = rtm3d_amd.create_model(rtm3d_amd.kitti_config(f['backbone'])).to('cuda')
    m.load_state_dict(f['sd'] if sd is None else sd)
    m.use_graph = False
    return m


def _bits(ts):
    return [t.detach().cpu().numpy().tobytes() for t in ts]


def _model_case(fusion, st):
    """The chain's inputs read back from the plan of the last forward: the saved activations, the weights as the forward used
    them and the heads' dz."""
    rplan = st['plan']
    ops = {op.get('name'): op for op in rplan.plan.ops}
    nhwc = lambda s: np.ascontiguousarray(rplan.download(s).transpose(0, 2, 3, 1)).astype(np.float16)
    us, xs, w = [], [], []
    for l, L in enumerate((3, 4, 5)):
        xs.append([nhwc(ops['fusion_up%d.%d' % (L, j)]['inp'][0]) for j in range(l + 1)])
        assert np.array_equal(xs[l][0], nhwc(rplan.plan.named['kfpn_h%d' % L]))
        us.append(nhwc(rplan.plan.named['u%d' % L]))
        w.append([fusion._params[n].detach().half().cpu().numpy() for n in fusion._wnames[l]])
    dz = fusion.heads.input_grad().cpu().numpy()
    B, H, W, _ = dz.shape
    return {'B': B, 'H': H, 'W': W, 'levels': 3, 'C': 256, 'S': fusion.S, 'T': fusion.T, 'want_slices': None, 'dz': dz, 'us': us, 'xs': xs, 'w': w}


def test_model_forward_backward_refresh_and_training():
    import torch
    from rtm3d_amd import head_train as ht, neck_train as nt, optim
    from rtm3d_amd.loss import RTM3DLoss
    from tests import loss_cases
    f = _fixture()
    x = f['x']
    plain = _new_model()
    want_logits = _bits(plain.forward_logits(x))

    model = _new_model()
    with pytest.raises(ValueError, match='without input_grad=True'):
        nt.TrainableFusion(ht.TrainableHeads(model))
    fusion = nt.TrainableFusion(ht.TrainableHeads(model, input_grad=True))
    names = [n for n, _ in fusion.named_parameters()]
    own = [n for row in nt.weight_names() for n in row]
    assert names[-6:] == own and len(set(names)) == len(names) and set(fusion.state_dict()) >= set(names)
    batch = loss_cases.batch(f['case'])
    fn = RTM3DLoss(model.config)
    logits = fusion(x)
    assert all(t.grad_fn is not None for t in logits)
    assert _bits(logits) == want_logits                                        # both refreshes reproduce the host packers' bytes
    loss, _ = fn(logits, batch)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in fusion.named_parameters()}
    for k, v in grads.items():
        assert v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    assert fusion.nonfinite() == 0

    # against R64 on the plan's own saved activations and the heads' dz: a wrong tensor, stride or level wiring shows here
    st = fusion._last
    case = _model_case(fusion, st)
    q = ref.chain(case, True)
    r64, q16, floors = ref.flat(ref.chain(case, False), case['S'] * case['T']), ref.flat(q), ref.floors(q)
    ig16, ig32 = fusion.input_grads(), fusion.input_grads(fp32=True)
    assert sorted(ig16) == ['kfpn_h3', 'kfpn_h4', 'kfpn_h5', 'z0'] and ig16['z0'].data_ptr() == fusion.heads.input_grad().data_ptr()
    got = {}
    for l, L in enumerate((3, 4, 5)):
        got['dx[%d][0]' % l] = ig16['kfpn_h%d' % L].permute(0, 3, 1, 2).float().cpu().numpy()
        assert tuple(ig32['kfpn_h%d' % L].shape) == got['dx[%d][0]' % l].shape and ig32['kfpn_h%d' % L].dtype == torch.float32
        for j, n in enumerate(fusion._wnames[l]):
            got['dw[%d][%d]' % (l, j)] = grads[n].cpu().numpy()
    _within_bar('model', got, r64, q16, floors)

    # the explicit call on the same forward: the same bits as autograd left in the leaves
    dl = fn.grad([t.detach() for t in logits], batch)
    explicit = fusion.backward_explicit(st, dl)
    for k in grads:
        assert explicit[k].cpu().numpy().tobytes() == grads[k].cpu().numpy().tobytes(), k

    # a stale plan is refused: another forward of the shape overwrote the saved activations
    stale = fusion(x)
    fusion(x)
    with pytest.raises(RuntimeError, match='stale plan'):
        fn(stale, batch)[0].backward()

    # ten optimiser steps on one batch
    for p in fusion.parameters():
        p.grad = None
    before = {n: fusion._params[n].detach().clone() for n in own}
    solver = optim.Solver(fusion, model.config)
    losses = []
    for _ in range(10):
        loss, _ = fn(fusion(x), batch)
        losses.append(loss.detach())
        solver.step(loss)
    after = _bits(fusion(x))
    losses = [float(v) for v in losses]
    print('ten Adamax steps on one batch, heads + fusion: loss %s' % ' '.join('%.4f' % v for v in losses))
    assert losses[-1] < losses[0]
    assert after != want_logits
    for n in own:
        assert not torch.equal(before[n], fusion._params[n].detach()), n      # the fusion weights have moved
    fresh = _new_model()
    fusion.export_to(fresh)
    assert _bits(fresh.forward_logits(x)) == after
    assert fusion.nonfinite() == 0

    # a model that never met TrainableFusion is untouched
    assert _bits(plain.forward_logits(x)) == want_logits


def test_model_refuses_a_graph_replayed_plan():
    from rtm3d_amd import head_train as ht, neck_train as nt
    f = _fixture()
    m = _new_model()
    m.use_graph = True
    fusion = nt.TrainableFusion(ht.TrainableHeads(m, input_grad=True))
    with pytest.raises(NotImplementedError, match='replays a captured graph'):
        fusion(f['x'])
