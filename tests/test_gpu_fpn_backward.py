"""Neck FPN backward on the device (csrc/neck_fpn_backward.hip, rtm3d_amd/fpn_train.py) against tests/fpn_backward_ref.py.

Exact cases: every tensor holds small integers, so the device must equal the integer result in every output, bit for bit.
Real-valued cases: per tensor, the device's max-abs distance to R64 is at most max(4 x Q16's distance to R64, floor), the floor
being the any-order fp32 summation bound of the tensor's last reduction (fpn_backward_ref.chain) - the bar of
tests/test_gpu_neck_backward.py.  The measured ratios are in profiles/neck_fpn_backward.txt, section 3.
"""
import ctypes

import numpy as np
import pytest

from tests import fpn_backward_cases as cases
from tests import fpn_backward_ref as ref
from tests.test_gpu_neck_backward import _padded, _border_zero, _within_bar

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------- one 1x1 conv, exact
def run_layer(case, want, xborder, outputs=('dA', 'db')):
    """wgrad + dgrad of one 1x1 conv through the C entry points -> (dX NHWC, dA, db, non-finite count, the padded dX map)."""
    import torch
    from rtm3d_amd import _lib, head_train as ht, fpn_train as ft
    lib, dev = _lib.load(), torch.device('cuda', torch.cuda.current_device())
    B, H, W, Cin = case['B'], case['H'], case['W'], case['Cin']
    x, dy = _padded(case['x'], xborder, dev), _padded(case['dy'], 0, dev)
    dx = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float16, device=dev)
    wr = ft.transpose_weights(torch.from_numpy(case['A']).to(dev))
    dA = torch.full((256, Cin, 1, 1), float('nan'), dtype=torch.float32, device=dev) if 'dA' in outputs else None
    db = torch.full((256,), float('nan'), dtype=torch.float32, device=dev) if 'db' in outputs else None
    want = ft.default_slices(Cin) if want is None else want
    n_slices, _ = ht.slices(B * H * W, want)
    ws = torch.empty(int(lib.rtm3d_fpn_backward_workspace_bytes(Cin, n_slices)) // 4, dtype=torch.float32, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    xm, dym, dxm = ht.hb_map(x.data_ptr(), Cin, xborder), ht.hb_map(dy.data_ptr(), 256, 0), ht.hb_map(dx.data_ptr(), Cin, 1)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.check(lib.rtm3d_fpn_conv1x1_wgrad(st, B, H, W, Cin, ctypes.byref(xm), ctypes.byref(dym), cases.INT_INV, ptr(dA), ptr(db), want,
                                           ws.data_ptr(), ws.numel() * 4, ctr.data_ptr()), 'fpn_conv1x1_wgrad')
    _lib.check(lib.rtm3d_fpn_conv1x1_dgrad(st, B, H, W, Cin, ctypes.byref(dym), wr.data_ptr(), cases.INT_MUL, ctypes.byref(dxm)), 'fpn_conv1x1_dgrad')
    torch.cuda.synchronize()
    num = lambda t: t.cpu().numpy() if t is not None else None
    return dx[:, 1:-1, 1:-1].float().cpu().numpy(), num(dA), num(db), int(ctr.item()), dx


_LAYER = {}


def _layer(cid, Cin):
    if (cid, Cin) not in _LAYER:
        spec = dict(cases.INT_LAYERS[cid])
        wants = spec.pop('want')
        case = cases.int_layer(Cin=Cin, **spec)
        dx, dA, db = ref.layer_exact(case['x'], case['A'], case['dy'], cases.INT_INV, cases.INT_MUL)
        cases.check_layer_exact(case, dx, dA, db)
        _LAYER[(cid, Cin)] = (case, wants, dx, dA.reshape(256, Cin, 1, 1), db)
    return _LAYER[(cid, Cin)]


@pytest.mark.parametrize('Cin', cases.INT_CIN)
@pytest.mark.parametrize('cid', sorted(cases.INT_LAYERS))
def test_conv1x1_exact_integer_cases(cid, Cin):
    case, wants, dx, dA, db = _layer(cid, Cin)
    for xborder in (0, 1):
        for want in wants:
            gx, gA, gb, bad, dxmap = run_layer(case, want, xborder)
            print('%s Cin %d border %d want_slices %s: dX %d of %d differ (max |ref| %g), dA %d of %d (max %g), db %d of %d (max %g)'
                  % (cid, Cin, xborder, want, int((gx != dx).sum()), dx.size, np.abs(dx).max(), int((gA != dA).sum()), dA.size, np.abs(dA).max(),
                     int((gb != db).sum()), db.size, np.abs(db).max()))
            assert gx.shape == dx.shape and np.array_equal(gx, dx), (cid, Cin, xborder, want)
            assert gA.shape == dA.shape and np.array_equal(gA, dA), (cid, Cin, xborder, want)
            assert gb.shape == db.shape and np.array_equal(gb, db), (cid, Cin, xborder, want)
            assert np.abs(dA).max() > 0 and np.abs(dx).max() > 0 and np.abs(db).max() > 0
            assert bad == 0
            _border_zero(dxmap, 1)
            ax, aA, ab, _, _ = run_layer(case, want, xborder)                 # the second call: the same bits
            assert ax.tobytes() == gx.tobytes() and aA.tobytes() == gA.tobytes() and ab.tobytes() == gb.tobytes()


def test_conv1x1_each_output_alone_and_a_slice_of_a_wider_map():
    """A NULL output is skipped and the other holds the bits of the full call; X and dX may be channels of a wider tensor."""
    import torch
    from rtm3d_amd import _lib, head_train as ht, fpn_train as ft
    case, _, dx, dA, db = _layer('b3_3x5', 320)
    _, fA, fb, _, _ = run_layer(case, None, 1)
    _, oA, ob, _, _ = run_layer(case, None, 1, outputs=('dA',))
    assert ob is None and oA.tobytes() == fA.tobytes()
    _, oA, ob, _, _ = run_layer(case, None, 1, outputs=('db',))
    assert oA is None and ob.tobytes() == fb.tobytes()
    lib, dev = _lib.load(), torch.device('cuda', torch.cuda.current_device())
    B, H, W, Cin = case['B'], case['H'], case['W'], 64
    wide = np.zeros((B, H, W, 384), np.float16)
    wide[..., 320:] = 7                                                       # a neighbour's channels: never read, never written
    wide[..., 256:320] = case['x'][..., :64]
    x = _padded(wide, 1, dev)
    dy = _padded(case['dy'], 0, dev)
    dxw = torch.full((B, H, W, 384), 5.0, dtype=torch.float16, device=dev)
    A = np.ascontiguousarray(case['A'][:, :64])
    dAo = torch.empty(256, 64, 1, 1, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.rtm3d_fpn_backward_workspace_bytes(64, 2)) // 4, dtype=torch.float32, device=dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    xm, dym, dxm = ht.hb_map(x.data_ptr(), 384, 1, 256), ht.hb_map(dy.data_ptr(), 256, 0), ht.hb_map(dxw.data_ptr(), 384, 0, 256)
    _lib.check(lib.rtm3d_fpn_conv1x1_wgrad(st, B, H, W, 64, ctypes.byref(xm), ctypes.byref(dym), cases.INT_INV, dAo.data_ptr(), None, 2,
                                           ws.data_ptr(), ws.numel() * 4, ctr.data_ptr()), 'fpn_conv1x1_wgrad')
    _lib.check(lib.rtm3d_fpn_conv1x1_dgrad(st, B, H, W, 64, ctypes.byref(dym), ft.transpose_weights(torch.from_numpy(A).to(dev)).data_ptr(),
                                           cases.INT_MUL, ctypes.byref(dxm)), 'fpn_conv1x1_dgrad')
    torch.cuda.synchronize()
    rx, rA, _ = ref.layer_exact(case['x'][..., :64], A, case['dy'], cases.INT_INV, cases.INT_MUL)
    assert np.array_equal(dAo.cpu().numpy().reshape(256, 64), rA)
    got = dxw.float().cpu().numpy()
    assert np.array_equal(got[..., 256:320], rx) and (got[..., :256] == 5).all() and (got[..., 320:] == 5).all()


# --------------------------------------------------------------------------------------------------- grad add
@pytest.mark.parametrize('shape_r', [((1, 1, 1), 1.0), ((2, 3, 5), 0.25), ((3, 8, 12), 4.0)])
def test_grad_add_exact_and_special_values(shape_r):
    import torch
    from rtm3d_amd import _lib, head_train as ht
    (B, H, W), r = shape_r
    c = cases.add_case(9, B, H, W, r)
    lib, dev = _lib.load(), torch.device('cuda', torch.cuda.current_device())
    e, f = _padded(c['e'], 0, dev), _padded(c['f'], 1, dev)
    g = torch.zeros(B, H + 4, W + 4, 320, dtype=torch.float16, device=dev)
    _lib.check(lib.rtm3d_fpn_grad_add(_lib.stream_ptr(dev), B, H, W, ctypes.byref(ht.hb_map(e.data_ptr(), 256, 0)),
                                      ctypes.byref(ht.hb_map(f.data_ptr(), 256, 1)), r, ctypes.byref(ht.hb_map(g.data_ptr(), 320, 2, 64))), 'fpn_grad_add')
    torch.cuda.synchronize()
    want = ref.add_exact(c['e'], c['f'], r)
    got = g[:, 2:-2, 2:-2, 64:].cpu().numpy()
    assert got.view(np.uint16)[~np.isnan(want)].tobytes() == want.view(np.uint16)[~np.isnan(want)].tobytes()
    assert np.isnan(got[np.isnan(want)]).all() and np.isnan(want).sum() == 3
    assert np.isinf(got[0, 0, 0, 1:3]).all() and got[0, 0, 0, 5] == np.inf
    assert not bool(g[..., :64].view(torch.int16).any())
    _border_zero(g, 2)


# --------------------------------------------------------------------------------------------------- the whole chain
def run_chain(case, want=None):
    """The chain of a case on the device -> ({name: numpy}, FpnBackward).  want: names of the parameter gradients to produce."""
    import torch
    from rtm3d_amd import head_train as ht, neck_train as nt, fpn_train as ft
    dev = torch.device('cuda')
    fch = [case['ncat'][k].shape[3] - 256 for k in range(3)] + [case['feat3'].shape[3]]
    fp = ft.FpnBackward(case['B'], case['H'], case['W'], dev, fch, case['S'], case['T'], case['U'], case['want_slices'])
    keep = [_padded(case['dz'], 0, dev)]
    up = lambda a, P, C: (keep.append(_padded(a, P, dev)), ht.hb_map(keep[-1].data_ptr(), C, P))[1]
    ncat = [up(case['ncat'][k], 1, fp.cin[k]) for k in range(3)]
    h = [up(case['h'][k], 1, 256) for k in range(3)]
    F = [up(case['F'][k], 1, 256) for k in range(3)]
    feat3 = up(case['feat3'], 0, fp.cin[3])
    wr = [ft.transpose_weights(torch.from_numpy(np.asarray(case['A'][k], np.float16)).to(dev)) for k in range(4)]
    wur = [nt.rotate_deconv_weights(torch.from_numpy(np.asarray(case['wup'][k], np.float16)).to(dev)) for k in range(3)]
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
    on = lambda name: want is None or name in want
    dA = [nan(256, fp.cin[k], 1, 1) if on('dA[%d]' % k) else None for k in range(4)]
    db = [nan(256) if on('db[%d]' % k) else None for k in range(4)]
    dwu = [nan(256, 256, 4, 4) if on('dwup[%d]' % k) else None for k in range(3)]
    fp.run(ht.hb_map(keep[0].data_ptr(), 256, 0), ncat, h, feat3, F, wr, wur, dA, db, dwu)
    torch.cuda.synchronize()
    out = {'dfeat3': fp.dfeat3.permute(0, 3, 1, 2)}
    for k in range(3):
        out['D[%d]' % k] = fp.D[k][:, 1:-1, 1:-1].permute(0, 3, 1, 2)
        out['E[%d]' % k], out['g[%d]' % k] = fp.E[k].permute(0, 3, 1, 2), fp.g[k].permute(0, 3, 1, 2)
        out['dwup[%d]' % k] = dwu[k]
    for k in range(4):
        out['dA[%d]' % k] = dA[k].view(256, fp.cin[k]) if dA[k] is not None else None
        out['db[%d]' % k] = db[k]
    return {k: v.float().cpu().numpy() for k, v in out.items() if v is not None}, fp


_REAL = {}


def _real(key):
    if key not in _REAL:
        T, U, want = key
        case = cases.real_case(6, 2, 16, 24, 1024.0, T, U, want_slices=want)
        q = ref.chain(case, True)
        _REAL[key] = (case, ref.flat(ref.chain(case, False), case['S'] * U), ref.flat(q), ref.floors(q))
    return _REAL[key]


@pytest.mark.parametrize('key', [(4.0, 4.0, None), (16.0, 4.0, 3)])
def test_chain_real_valued_within_four_times_q16(key):
    case, r64, q16, floors = _real(key)
    got, fp = run_chain(case)
    assert sorted(got) == sorted(r64)
    _within_bar('T=%g U=%g 2x16x24' % (key[0], key[1]), got, r64, q16, floors)
    assert int(fp.nonfinite.item()) == 0
    for t in fp.D:
        _border_zero(t, 1)


def test_chain_second_run_and_each_gradient_alone():
    case, _, _, _ = _real((4.0, 4.0, None))
    full, _ = run_chain(case)
    again, _ = run_chain(case)
    for name in full:
        assert full[name].tobytes() == again[name].tobytes(), name
    for name in ('dA[1]', 'db[3]', 'dwup[2]'):
        alone, _ = run_chain(case, want=(name,))
        assert [k for k in alone if k[:2] in ('dA', 'db', 'dw')] == [name]
        assert alone[name].tobytes() == full[name].tobytes(), name


def test_nonfinite_dz_reaches_the_gradients_and_is_counted():
    case, _, _, _ = _real((4.0, 4.0, None))
    case = dict(case, dz=case['dz'].copy())
    case['dz'][1, 3, 4, 7] = np.nan
    got, fp = run_chain(case)
    assert np.isnan(got['dA[0]'][7]).all() and np.isfinite(np.delete(got['dA[0]'], 7, axis=0)).all()      # output channel 7, every ci
    assert np.isnan(got['db[0]'][7]) and np.isfinite(np.delete(got['db[0]'], 7)).all()
    assert np.isnan(got['D[0]'][1, :, 3, 4]).all() and np.isfinite(got['D[0]'][0]).all()                   # through the dgrad: every channel of the pixel
    for k in (1, 2, 3):
        assert np.isnan(got['dA[%d]' % k]).any(), k
    assert int(fp.nonfinite.item()) >= 320 + 1
