"""Head backward on the device (csrc/head_backward.hip, rtm3d_amd/head_train.py) against tests/head_backward_ref.py.

Exact cases: every tensor holds small integers, so the device must equal the integer result in every output, bit for bit.
Real-valued cases: per tensor, the device's max-abs distance to R64 is at most max(4 x Q16's distance to R64, floor), the floor
being the any-order fp32 summation bound of the tensor's last reduction (head_backward_ref.chain).  Measured on an MI355X
(profiles/head_backward.txt): the ratio device-to-R64 over Q16-to-R64 is 1.000 for go, every dh and dz (the device rounds the
same values), 0.95 .. 1.05 for the parameter gradients; the worst of the three cases 1.040 / 1.049 / 1.040.
"""
import numpy as np
import pytest

from tests import head_backward_cases as cases
from tests import head_backward_ref as ref

pytestmark = pytest.mark.gpu


def _padded(a, P, dev):
    import torch
    B, H, W, C = a.shape
    t = torch.zeros(B, H + 2 * P, W + 2 * P, C, dtype=torch.float16, device=dev)
    t[:, P:P + H, P:P + W] = torch.from_numpy(a).to(dev)
    return t


def run_device(case, want=None):
    """The chain of a case on the device -> ({name: numpy}, HeadBackward, raw gradient maps).  want: names of the parameter
    gradients to produce (None: all); the others are skipped (NULL outputs)."""
    import torch
    from rtm3d_amd import head_train as ht
    dev = torch.device('cuda')
    G, n, K = len(case['K']), case['num_conv'], case['K']
    hb = ht.HeadBackward(case['B'], case['H'], case['W'], K, n, dev, case['S'], case['input_grad'], case['want_slices'])
    keep = [_padded(case['acts'][0], 6, dev)] + [_padded(case['acts'][k], 1, dev) for k in range(1, n + 1)]
    acts = [ht.hb_map(keep[0].data_ptr(), 256, 6, 0, 0)] + [ht.hb_map(keep[k].data_ptr(), G * 256, 1, 0, 256) for k in range(1, n + 1)]
    wr = [None] + [ht.rotate_weights(torch.from_numpy(np.stack(case['wf'][k])).to(dev)) for k in range(1, n + 1)]
    wo = torch.zeros(G, 16, 256, 3, 3, dtype=torch.float16, device=dev)
    for g in range(G):
        wo[g, :K[g]] = torch.from_numpy(case['wo'][g]).to(dev)
    wr_out = ht.rotate_weights(wo)
    scales = [None] + [[torch.from_numpy(case['scale'][k][g]).to(dev) for g in range(G)] for k in range(1, n + 1)]
    f32 = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
    sel = lambda name, t: t if want is None or name in want else None
    dw = [None] + [[sel('dw%d[%d]' % (k, g), f32(256, 256, 3, 3)) for g in range(G)] for k in range(1, n + 1)]
    db = [None] + [[sel('db%d[%d]' % (k, g), f32(256)) for g in range(G)] for k in range(1, n + 1)]
    dwo = [sel('dwo[%d]' % g, f32(K[g], 256, 3, 3)) for g in range(G)]
    dbo = [sel('dbo[%d]' % g, f32(K[g])) for g in range(G)]
    hb.run([torch.from_numpy(d).to(dev) for d in case['dlogits']], acts, wr, wr_out, scales, dw, db, dwo, dbo)
    torch.cuda.synchronize()
    out = {}
    for k in range(1, n + 1):
        for g in range(G):
            out['dw%d[%d]' % (k, g)], out['db%d[%d]' % (k, g)] = dw[k][g], db[k][g]
    for g in range(G):
        out['dwo[%d]' % g], out['dbo[%d]' % g] = dwo[g], dbo[g]
        out['go[%d]' % g] = hb.go[:, 1:-1, 1:-1, g * 16:g * 16 + K[g]].permute(0, 3, 1, 2)
    for k in range(1, n + 1):
        P = 6 if k == 1 else 1
        out['dh%d' % k] = hb.dh[k][:, P:-P, P:-P].permute(0, 3, 1, 2)
    if case['input_grad']:
        out['dz'] = hb.dz.permute(0, 3, 1, 2)
    return {k: v.float().cpu().numpy() for k, v in out.items() if v is not None}, hb


def _borders_zero(hb):
    import torch
    for t, P in [(hb.go, 1)] + [(hb.dh[k], 6 if k == 1 else 1) for k in range(1, hb.num_conv + 1)]:
        inner = torch.zeros_like(t, dtype=torch.bool)
        inner[:, P:-P, P:-P] = True
        assert not bool(t.view(torch.int16)[~inner].any()), 'a border byte is not zero'
    # the padding channels of go (k >= K) are zero bytes too
    for g, k in enumerate(hb.K):
        assert not bool(hb.go.view(torch.int16)[..., g * 16 + k:(g + 1) * 16].any())


_EXPECT = {}


def _expected(cid):
    if cid not in _EXPECT:
        case = cases.int_case(**cases.INT_CASES[cid])
        want = ref.flat(ref.chain(case, True))
        cases.check_exact(case, want)
        _EXPECT[cid] = (case, want)
    return _EXPECT[cid]


@pytest.mark.parametrize('cid', sorted(cases.INT_CASES))
def test_exact_integer_cases(cid):
    case, want = _expected(cid)
    got, hb = run_device(case)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        bad = int((got[name] != want[name]).sum())
        print('%s %s: %d of %d elements differ, max |ref| %g' % (cid, name, bad, want[name].size, np.abs(want[name]).max()))
        assert got[name].shape == want[name].shape and bad == 0, (cid, name)
    _borders_zero(hb)
    assert int(hb.nonfinite.item()) == 0
    # the second call: the same bits
    again, _ = run_device(case)
    for name in want:
        assert got[name].tobytes() == again[name].tobytes(), name


def test_each_output_alone_equals_the_full_call():
    case, want = _expected('g2_smoke_13x20_b3')
    full, _ = run_device(case)
    for name in ('dw1[1]', 'db2[0]', 'dwo[1]', 'dbo[0]'):
        alone, _ = run_device(case, want=(name,))
        assert [k for k in alone if k.startswith(('dw', 'db'))] == [name]
        assert alone[name].tobytes() == full[name].tobytes(), name


_REAL = {}


def _real(key):
    if key not in _REAL:
        B, H, W, S = key
        case = cases.real_case(11, B, H, W, S)
        r64 = ref.chain(case, False)
        q = ref.chain(case, True)
        _REAL[key] = (case, ref.flat(r64, S), ref.flat(q), q)
    return _REAL[key]


@pytest.mark.parametrize('key', [(3, 13, 20, 1.0), (3, 13, 20, 256.0), (2, 16, 32, 1024.0)])
def test_real_valued_within_four_times_q16(key):
    case, r64, q16, qraw = _real(key)
    got, hb = run_device(case)
    worst = 0.0
    for name in sorted(r64):
        dq = float(np.abs(q16[name] - r64[name]).max())
        dd = float(np.abs(got[name].astype(np.float64) - r64[name]).max())
        base = name.split('[')[0]
        floor = qraw['floor:' + base][int(name.split('[')[1][:-1])] if 'floor:' + base in qraw else 0.0
        bar = max(4.0 * dq, floor)
        ratio = dd / dq if dq > 0 else float('inf') if dd > 0 else 0.0
        print('S=%g %dx%dx%d %s: max|ref| %.3e  Q16-R64 %.3e  device-R64 %.3e  ratio %.3f  floor %.3e'
              % (key[3], key[0], key[1], key[2], name, np.abs(r64[name]).max(), dq, dd, ratio, floor))
        assert dd <= bar, (name, dd, dq, floor)
        worst = max(worst, ratio if np.isfinite(ratio) else 0.0)
    print('worst ratio %.3f' % worst)
    assert int(hb.nonfinite.item()) == 0


def test_nonfinite_upstream_propagates_and_is_counted():
    case, _ = _expected('g1_5x7_b1')
    case = dict(case, dlogits=[d.copy() for d in case['dlogits']])
    case['dlogits'][0][0, 1, 2, 3] = np.nan
    got, hb = run_device(case)
    assert np.isnan(got['dbo[0]'][1]) and np.isnan(got['dwo[0]'][1]).any() and np.isnan(got['dw1[0]']).any()
    assert np.isfinite(got['dbo[0]'][0])                      # the neighbouring channel's sum is untouched
    assert int(hb.nonfinite.item()) > 0


# --------------------------------------------------------------------------------------------------- through the model
_MODEL = {}


def _fixture():
    """The model of e2e_dla34_small.npz (its smallest shape: B = 2, 3 x 128 x 256), its input and a label batch; built once."""
    if not _MODEL:
        import torch
        import rtm3d_amd
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


def test_model_forward_backward_refresh_and_training():
    import torch
    from rtm3d_amd import head_train as ht, optim
    from rtm3d_amd.loss import RTM3DLoss
    from tests import loss_cases
    f = _fixture()
    x = f['x']
    plain = _new_model()
    want_logits = _bits(plain.forward_logits(x))

    model = _new_model()
    heads = ht.TrainableHeads(model, input_grad=True)
    batch = loss_cases.batch(f['case'])
    fn = RTM3DLoss(model.config)
    logits = heads(x)
    assert all(t.grad_fn is not None for t in logits)
    assert _bits(logits) == want_logits                                        # the refresh reproduces the host packers' bytes
    loss, _ = fn(logits, batch)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in heads.named_parameters()}
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values())
    assert any(float(v.abs().max()) > 0 for v in grads.values())
    assert heads.nonfinite() == 0
    dz16, dz32 = heads.input_grad(), heads.input_grad(fp32=True)
    assert dz16.dtype == torch.float16 and tuple(dz32.shape) == (x.shape[0], 256, x.shape[2] // 4, x.shape[3] // 4)

    # the explicit call on the same forward: the same bits as autograd left in the leaves
    st = heads._last
    dl = fn.grad([t.detach() for t in logits], batch)
    explicit = heads.backward_explicit(st, dl)
    for k in grads:
        assert explicit[k].cpu().numpy().tobytes() == grads[k].cpu().numpy().tobytes(), k

    # a stale plan is refused: another forward of the shape overwrote the saved activations
    stale = heads(x)
    heads(x)
    with pytest.raises(RuntimeError, match='stale plan'):
        fn(stale, batch)[0].backward()

    # optimiser step, automatic refresh, then a fresh Model loaded from the exported parameters gives the same logits
    for p in heads.parameters():
        p.grad = None
    cfg = model.config.clone() if hasattr(model.config, 'clone') else model.config
    solver = optim.Solver(heads, cfg)
    losses = []
    for _ in range(10):
        loss, _ = fn(heads(x), batch)
        losses.append(loss.detach())
        solver.step(loss)                                                      # zero_grad, backward, the Adamax launch
    after = _bits(heads(x))
    losses = [float(v) for v in losses]
    print('ten Adamax steps on one batch: loss %s' % ' '.join('%.4f' % v for v in losses))
    assert losses[-1] < losses[0]
    assert after != want_logits
    fresh = _new_model()
    heads.export_to(fresh)
    assert _bits(fresh.forward_logits(x)) == after

    # a model that never met TrainableHeads is untouched
    assert _bits(plain.forward_logits(x)) == want_logits


def test_model_refusals():
    import rtm3d_amd
    from rtm3d_amd import head_train as ht
    f = _fixture()
    m = _new_model()
    with pytest.raises(ValueError, match='no power of two'):
        ht.TrainableHeads(m, grad_scale=100.0)
    m.use_graph = True
    heads = ht.TrainableHeads(m)
    with pytest.raises(NotImplementedError, match='replays a captured graph'):
        heads(f['x'])
    mx = rtm3d_amd.Model(rtm3d_amd.kitti_config(f['backbone']), head_precision='mxfp8').to('cuda')
    with pytest.raises(NotImplementedError, match='mxfp8'):
        ht.TrainableHeads(mx)
