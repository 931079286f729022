"""GPU: the loss gradient on the device (rtm3d_loss_grad through rtm3d_amd.loss.RTM3DLoss) against the numpy restatement
tests/loss_grad_ref.py and the reference-run fixture tests/golden/loss_grad_cases.npz.

Bars (include/rtm3d_hip.h, "loss gradient"): NaN and zero patterns equal, every zero of the regression maps +0.0f bitwise;
per map the max abs error against the restatement's fp32 run within max(4 x the distance between the restatement's fp32 and
fp64 runs, 4 fp32 ulp of the map's largest magnitude) - the device's expf, logf and powf are not numpy's to the last bit, every
other operation is the same fp32 operation in the same order -, and against the reference's fp64 gradient within max(4 x the
reference's own fp32-vs-fp64 distance, the same floor).  Both distances are computed on the CPU and printed."""
import ctypes

import numpy as np
import pytest
import torch

from rtm3d_amd import _lib, loss as L
from tests import loss_cases as lc, loss_grad_cases as gc, loss_grad_ref as gref
from tests.util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def to_dev(arrays, dev):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]          # (a copy: the cases' arrays are read-only)


def loss_of(spec):
    c, w = spec['case'], spec['weights']
    return L.RTM3DLoss({'MODEL': {'FOCAL_LOSS_ALPHA': c['alpha'], 'FOCAL_LOSS_BEDA': c['beta']},
                        'TRAINING': {'W_MKF': w[0], 'W_VFM': w[1], 'W_M_OFF': w[2], 'W_V_OFF': w[3]}})


def device_grad(spec, dev, **kw):
    """-> the four maps of RTM3DLoss.grad as numpy arrays (None where not wanted)."""
    fn = loss_of(spec)
    g = fn.grad(to_dev(spec['logits'], dev), lc.batch(spec['case']), upstream=spec['upstream'], **kw)
    torch.cuda.synchronize()
    assert len(g) == 4
    return [None if a is None else a.cpu().numpy() for a in g]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', gc.ALL_CASES)
def test_gradient_matches_the_restatement(dev, name):
    """Every case of the forward's tests and every regime the backward adds (collisions on m_proj and v_proj cells, the clamp,
    num_pos = 0, empty selections, sign(0), non-finite logits, powf, zero and negative weights, an upstream factor).  Measured
    on an MI355X: the three regression maps equal the restatement to the last bit on every case; heat map max abs error 3.3e-9
    .. 4.2e-7, 0.4 .. 1.4 times the restatement's fp32-vs-fp64 distance (bar 4 x; closest: 'borders' 7.5e-8 against 2.1e-7);
    against the reference's fp64 run the heat map 7.1e-8 .. 5.7e-7 (bars 2.5e-7 .. 2.3e-6), the regression maps at most 1.2e-9."""
    r = gc.restated(name)
    spec = r['spec']
    got = device_grad(spec, dev)
    g = load_golden('loss_grad_cases.npz') if name in lc.FIXTURE_CASES else None
    for k, what in enumerate(gc.MAPS):
        assert got[k].dtype == np.float32
        d, bar = gc.restatement_bar(r, k)
        err = gc.compare(got[k], r['g32'][k], bar, (name, what))
        print(name, what, 'restatement fp32-vs-fp64 distance %.3g, bar %.3g, device error %.3g' % (d, bar, err))
        if k > 0:
            assert not np.signbit(got[k][got[k] == 0]).any(), (name, what, 'a zero that is not +0.0f')
        if g is not None:
            f64, fbar = gc.fixture_bar(g, name, k)
            ef = gc.compare(got[k], f64, fbar, (name, what, 'fixture'))
            print(name, what, 'device error vs the reference fp64 run %.3g, bar %.3g' % (ef, fbar))


def test_backward_fills_the_leaves_like_the_explicit_call(dev):
    r = gc.restated('fx_b1')
    c = r['spec']['case']
    lg, bt = to_dev(r['spec']['logits'], dev), lc.batch(c)
    fn = L.RTM3DLoss()
    plain_loss, plain_items = fn(lg, bt)
    assert plain_loss.grad_fn is None and not plain_loss.requires_grad
    explicit = fn.grad(lg, bt)
    twice = fn.grad(lg, bt, upstream=2.0)
    leaves = [t.clone().requires_grad_(True) for t in lg]
    bt.to(dev).table(c['H'], c['W'])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')              # neither the forward nor the backward waits for the device
    try:
        loss, items = fn(leaves, bt)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert loss.grad_fn is not None and loss.shape == () and not items.requires_grad and items.grad_fn is None
    assert same_bits(items.cpu().numpy(), plain_items.cpu().numpy()) and float(loss.detach()) == float(plain_loss)
    for leaf, e in zip(leaves, explicit):
        assert leaf.grad is not None and same_bits(leaf.grad.cpu().numpy(), e.cpu().numpy())
    # the upstream factor arrives as a device scalar
    leaves = [t.clone().requires_grad_(True) for t in lg]
    (2 * fn(leaves, bt)[0]).backward()
    for leaf, e, e1 in zip(leaves, twice, explicit):
        assert same_bits(leaf.grad.cpu().numpy(), e.cpu().numpy())
    assert not same_bits(twice[0].cpu().numpy(), explicit[0].cpu().numpy())
    # only some maps require grad: the others are neither computed nor filled
    leaves = [t.clone().requires_grad_(k in (0, 2)) for k, t in enumerate(lg)]
    fn(leaves, bt)[0].backward()
    assert leaves[1].grad is None and leaves[3].grad is None
    assert same_bits(leaves[0].grad.cpu().numpy(), explicit[0].cpu().numpy()) and same_bits(leaves[2].grad.cpu().numpy(), explicit[2].cpu().numpy())
    # no_grad, and maps that do not require grad: today's call, bit for bit
    leaves = [t.clone().requires_grad_(True) for t in lg]
    with torch.no_grad():
        l0, i0 = fn(leaves, bt)
    assert l0.grad_fn is None and same_bits(i0.cpu().numpy(), plain_items.cpu().numpy()) and same_bits(l0.cpu().numpy(), plain_loss.cpu().numpy())
    # a second derivative does not exist
    leaves = [t.clone().requires_grad_(True) for t in lg]
    g0, = torch.autograd.grad(fn(leaves, bt)[0], leaves[0], create_graph=True)
    with pytest.raises(RuntimeError, match='does not require grad|once_differentiable'):
        g0.sum().backward()


def test_two_calls_are_bit_identical(dev):
    for name in ('fx_b1', 'many', 'collide'):
        spec = gc.restated(name)['spec']
        a, b = device_grad(spec, dev), device_grad(spec, dev)
        assert all(same_bits(x, y) for x, y in zip(a, b)), name


def test_each_output_alone_equals_the_full_call(dev):
    for name in ('fx_b1', 'collide'):
        spec = gc.restated(name)['spec']
        full = device_grad(spec, dev)
        for k in range(4):
            want = tuple(j == k for j in range(4))
            one = device_grad(spec, dev, want=want)
            assert all(one[j] is None for j in range(4) if j != k) and same_bits(one[k], full[k]), (name, k)


def test_unaligned_maps_take_the_scalar_path(dev):
    """W % 4 == 0, but inputs and outputs that start 4 bytes into their allocations: no 16-byte access applies; bit-equal."""
    spec = gc.restated('fx_b1')['spec']
    c = spec['case']
    lg, bt = to_dev(spec['logits'], dev), lc.batch(c)

    def shifted(t, fill=None):
        flat = torch.full((t.numel() + 5,), 7.0, dtype=torch.float32, device=dev)
        v = flat[1:1 + t.numel()].view(t.shape)
        if fill is None:
            v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return flat, v

    fn = L.RTM3DLoss()
    full = fn.grad(lg, bt)
    ins = [shifted(t) for t in lg]
    outs = [shifted(t, fill=True) for t in lg]
    got = fn.grad([v for _, v in ins], bt, out=[v for _, v in outs])
    torch.cuda.synchronize()
    for (flat, v), g, f in zip(outs, got, full):
        assert g.data_ptr() == v.data_ptr() and same_bits(g.cpu().numpy(), f.cpu().numpy())
        assert flat[0].item() == 7.0 and (flat[1 + v.numel():] == 7.0).all()           # nothing written outside the map
    # aligned inputs into unaligned outputs and the other way round
    outs = [shifted(t, fill=True) for t in lg]
    for g, f in zip(fn.grad(lg, bt, out=[v for _, v in outs]), full):
        assert same_bits(g.cpu().numpy(), f.cpu().numpy())
    for g, f in zip(fn.grad([v for _, v in ins], bt), full):
        assert same_bits(g.cpu().numpy(), f.cpu().numpy())


def test_refusals(dev):
    spec = gc.restated('fx_b1')['spec']
    c = spec['case']
    lg, bt = to_dev(spec['logits'], dev), lc.batch(c)
    fn = L.RTM3DLoss()
    fn(lg, bt)
    lib, counts, tab = _lib.load(), fn.counts, bt.table(c['H'], c['W'])
    outs = [torch.empty_like(t) for t in lg]
    p = lambda t: None if t is None else t.data_ptr()

    def call(B=c['B'], C=c['C'], H=c['H'], W=c['W'], ins=lg, N=bt.N, params=fn._params, counts=counts, up=None, outs=outs):
        return lib.rtm3d_loss_grad(_lib.stream_ptr(dev), B, C, H, W, p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), bt._dev[2].data_ptr(),
                                   tab.data_ptr(), N, ctypes.byref(params) if params is not None else None, p(counts), p(up),
                                   p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]))

    assert call() == 0
    for kw, word in ((dict(B=0), b'bad sizes'), (dict(C=70000), b'bad sizes'), (dict(N=-1), b'bad sizes'), (dict(H=1 << 20, W=1 << 12), b'int index'),
                     (dict(H=1 << 14, W=1 << 13), b'16 x'),
                     (dict(ins=[lg[0], None, lg[2], lg[3]]), b'null pointer'), (dict(params=None), b'null pointer'),
                     (dict(params=_lib.LossParamsC(0.0, 4.0, (ctypes.c_float * 4)(1, 1, 1, 1))), b'alpha'),
                     (dict(params=_lib.LossParamsC(2.0, 4.0, (ctypes.c_float * 4)(1, float('nan'), 1, 1))), b'NaN'),
                     (dict(counts=None), b'd_counts'), (dict(outs=[None] * 4), b'no output'),
                     (dict(outs=[lg[0], None, None, None]), b'is input'), (dict(outs=[None, None, lg[1], None]), b'is input'),
                     (dict(up=outs[3].view(-1)[:1]), b'is input')):
        assert call(**kw) != 0, kw
        assert word in lib.rtm3d_last_error(), (kw, lib.rtm3d_last_error())
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='want'):
        fn.grad(lg, bt, want=(False,) * 4)
    with pytest.raises(ValueError, match='counts'):
        fn.grad(lg, bt, counts=counts.long())
    with pytest.raises(ValueError, match='out'):
        fn.grad(lg, bt, out=[outs[0].double(), None, None, None])
    with pytest.raises(ValueError, match='upstream'):
        fn.grad(lg, bt, upstream=torch.ones(2, device=dev))


def test_descent_on_the_heat_map_lowers_the_main_item(dev):
    """20 steps x -= lr * g on the heat map (which is smooth) from fx_b1's logits.  lr = 2: the restatement's own descent on the
    CPU decreases at every step - asserted here before the device is used."""
    r = gc.restated('fx_b1')
    spec, hm = r['spec'], r['m_hm']
    lr, steps = 2.0, 20
    x = np.array(spec['logits'][0])
    trace = [gref.main_item(x, hm)]
    for _ in range(steps):
        x = (x - np.float32(lr) * gref.heat_grad(x, hm, r['counts'][0], 2.0, 4.0, 1.0, 1.0, np.float32)).astype(np.float32)
        trace.append(gref.main_item(x, hm))
    assert all(b < a for a, b in zip(trace, trace[1:])), trace
    lg, bt = to_dev(spec['logits'], dev), lc.batch(spec['case'])
    fn = L.RTM3DLoss()
    start = float(fn(lg, bt)[1][0])
    for _ in range(steps):
        g = fn.grad(lg, bt, want=(True, False, False, False))[0]
        lg[0].sub_(lr * g)
    end = float(fn(lg, bt)[1][0])
    print('main item: CPU %.6f -> %.6f, device %.6f -> %.6f' % (trace[0], trace[-1], start, end))
    assert end < start
