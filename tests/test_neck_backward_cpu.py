"""Neck fusion backward without a GPU: the two CPU yardsticks (tests/neck_backward_ref.py) against the reference-run fixture and
against each other, and every refusal that needs no device."""
import ctypes

import numpy as np
import pytest
import torch

from rtm3d_amd import _lib
from tests import neck_backward_cases as cases
from tests import neck_backward_ref as ref
from tests.util import load_golden

E_NULL, E_SHAPE, E_LEVELS, E_CHANNELS, E_MULTIPLE, E_SCALE, E_SLICES, E_BORDER, E_ALIGN, E_WORKSPACE = range(1, 11)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_r64_equals_the_reference_run():
    """R64 on the fixture's leaves against what the reference's own forward and loss.backward() left: the same fp64 arithmetic
    in another order, so 1e-12 relative.  Pins the detach, the tap geometry and the (ci, co, ky, kx) weight layout."""
    g = load_golden('neck_fusion_grad_cases.npz')
    case = cases.fixture_case(g)
    assert (case['B'], case['H'], case['W'], case['C']) == (2, 16, 24, 8)
    r = ref.chain(case, False)
    assert np.array_equal(np.asarray(g['g_z0']), np.asarray(g['G']))                       # dz0 = dz
    for l, L in enumerate((3, 4, 5)):
        d = _rel(r['dx'][l][0].numpy(), np.asarray(g['g_h%d' % L]))
        print('d kfpn_h%d: relative distance %.3e' % (L, d))
        assert d <= 1e-12, L
        for j in range(l + 1):
            d = _rel(r['dw'][l][j].numpy(), np.asarray(g['gw%d_%d' % (L, j)]))
            print('d fusion_up%d.%d: relative distance %.3e' % (L, j, d))
            assert d <= 1e-12, (L, j)
    # the written-out sums of the rule (layer_exact) are the same function as the autograd layer
    x, w, dy = case['xs'][2][1], case['w'][2][1], r['dx'][2][2].permute(0, 2, 3, 1).numpy()
    dx, dw = ref.layer_exact(x, w, dy, 1.0)
    assert _rel(dx.transpose(0, 3, 1, 2), r['dx'][2][1].numpy()) <= 1e-12 and _rel(dw, r['dw'][2][1].numpy()) <= 1e-12


def test_a_softmax_that_is_not_detached_differs():
    """The fixture tells the detached product from the full derivative of u * softmax(u)."""
    g = load_golden('neck_fusion_grad_cases.npz')
    case = cases.fixture_case(g)
    u = ref._nchw(case['us'][0]).requires_grad_(True)
    b, c, h, w = u.shape
    full = torch.autograd.grad(u * torch.softmax(u.view(b, c, -1), dim=-1).view(b, c, h, w), [u], ref._nchw(case['dz']))[0]
    assert _rel(full.numpy(), ref.chain(case, False)['du'][0].numpy()) > 1e-3


@pytest.mark.parametrize('key', [(2, 8, 8, 1.0), (3, 16, 24, 1.0), (2, 16, 24, None)])
def test_q16_against_r64(key):
    from rtm3d_amd import neck_train as nt
    B, H, W, T = key
    T = nt.DEFAULT_FUSION_SCALE if T is None else T
    S = 1024.0
    case = cases.real_case(5, B, H, W, S, T)
    r64, q = ref.chain(case, False), ref.chain(case, True)
    fr, fq, fl = ref.flat(r64, S * T), ref.flat(q), ref.floors(q)
    for name in sorted(fr):
        assert np.isfinite(fq[name]).all() and np.isfinite(fr[name]).all(), name
        print('T=%g %dx%dx%d %s: max|ref| %.3e  Q16-R64 %.3e  floor %.3e'
              % (T, B, H, W, name, np.abs(fr[name]).max(), np.abs(fq[name] - fr[name]).max(), fl.get(name, 0.0)))
        assert np.abs(fq[name] - fr[name]).max() <= 2e-3 * np.abs(fr[name]).max() + 2.0 ** -24, name      # fp16: 2^-11 per rounding, a few in a row


# ---------------------------------------------------------------------------------------------------- refusals
def _err():
    return _lib.load().rtm3d_last_error().decode()


@pytest.mark.parametrize('args, code, word', [
    ((0, 16, 24, 3, 1.0, 1.0), E_SHAPE, 'B, H, W'),
    ((2, 16, 24, 0, 1.0, 1.0), E_LEVELS, 'levels'),
    ((2, 16, 24, 4, 1.0, 1.0), E_LEVELS, 'levels'),
    ((2, 12, 24, 3, 1.0, 1.0), E_MULTIPLE, 'multiples of 8'),
    ((2, 16, 20, 3, 1.0, 1.0), E_MULTIPLE, 'multiples of 8'),
    ((2, 16, 24, 3, 3.0, 1.0), E_SCALE, 'grad_scale'),
    ((2, 16, 24, 3, 1.0, 0.0), E_SCALE, 'fusion_scale'),
    ((2, 16, 24, 3, 2.0 ** 100, 2.0 ** 100), E_SCALE, 'fp32 range'),
])
def test_check_refuses_by_name(args, code, word):
    assert _lib.load().rtm3d_neck_backward_check(*args) == code
    assert word in _err()


def test_check_accepts_and_workspace_bytes():
    lib = _lib.load()
    assert lib.rtm3d_neck_backward_check(2, 16, 24, 3, 16384.0, 64.0) == 0
    assert lib.rtm3d_neck_backward_check(32, 96, 320, 3, 16384.0, 1.0) == 0
    assert lib.rtm3d_neck_backward_check(1, 2, 2, 1, 1.0, 1.0) == 0
    assert lib.rtm3d_neck_backward_workspace_bytes(2, 3, 4) == 4 * 16 * 256 * 256 * 4          # the wgrad partials are the larger need
    assert lib.rtm3d_neck_backward_workspace_bytes(2048, 3, 1) == 3 * 2048 * 33 * 2 * 256 * 4   # here the softmax statistics
    assert lib.rtm3d_neck_backward_workspace_bytes(2, 4, 4) == 0 and lib.rtm3d_neck_backward_workspace_bytes(2, 3, 257) == 0


def _map(addr=4096, C=256, P=1, coff=0):
    return _lib.HbMapC(ctypes.c_void_p(addr), C, P, coff, 0)


def test_launch_functions_refuse_on_the_host_before_any_launch():
    """Made-up addresses: a refusal comes from the host checks, which touch neither the device nor the memory."""
    lib = _lib.load()
    ws, big = 1 << 20, 1 << 30
    ctr = 1 << 12
    wgrad = lambda x, dy, want=4, wsb=big, w=ws, dw=1 << 16, S=1.0: lib.rtm3d_neck_deconv_wgrad(
        None, 2, 4, 6, ctypes.byref(x) if x is not None else None, ctypes.byref(dy), S, 1.0, dw, want, w, wsb, ctr)
    assert wgrad(None, _map()) == E_NULL and 'null' in _err()
    assert wgrad(_map(addr=0), _map()) == E_NULL and 'NULL' in _err()
    assert wgrad(_map(), _map(P=0)) == E_BORDER and 'border' in _err()
    assert wgrad(_map(addr=4104), _map()) == E_ALIGN and 'multiple of 16' in _err()
    assert wgrad(_map(), _map(), w=ws + 8) == E_ALIGN
    assert wgrad(_map(C=128), _map()) == E_CHANNELS and 'channels' in _err()
    assert wgrad(_map(C=320, coff=72), _map()) == E_CHANNELS
    assert wgrad(_map(), _map(), wsb=1024) == E_WORKSPACE and 'workspace' in _err()
    assert wgrad(_map(), _map(), want=0) == E_SLICES and 'slices' in _err()
    assert wgrad(_map(), _map(), S=3.0) == E_SCALE
    dgrad = lambda dy, wr, dx: lib.rtm3d_neck_deconv_dgrad(None, 2, 4, 6, ctypes.byref(dy), wr, ctypes.byref(dx))
    assert dgrad(_map(), None, _map()) == E_NULL
    assert dgrad(_map(P=0), 4096, _map()) == E_BORDER
    assert dgrad(_map(), 4100, _map()) == E_ALIGN
    maps = lambda *m: (_lib.HbMapC * len(m))(*m)
    sm = lambda n, u, du, wsb=big, T=1.0: lib.rtm3d_neck_softmax_grad(None, 2, 16, 24, n, ctypes.byref(_map(P=0)), u, du, T, ws, wsb)
    assert sm(1, None, maps(_map())) == E_NULL
    assert sm(4, maps(_map()), maps(_map())) == E_LEVELS
    assert sm(2, maps(_map(), _map()), maps(_map(), _map(P=0))) == E_BORDER
    assert sm(1, maps(_map()), maps(_map()), wsb=64) == E_WORKSPACE
    assert sm(1, maps(_map()), maps(_map()), T=5.0) == E_SCALE


def test_header_names_the_codes():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rtm3d_hip.h')).read()
    for name, v in (('NULL', E_NULL), ('SHAPE', E_SHAPE), ('LEVELS', E_LEVELS), ('CHANNELS', E_CHANNELS), ('MULTIPLE', E_MULTIPLE), ('SCALE', E_SCALE),
                    ('SLICES', E_SLICES), ('BORDER', E_BORDER), ('ALIGN', E_ALIGN), ('WORKSPACE', E_WORKSPACE), ('LAUNCH', 11)):
        assert re.search(r'RTM3D_NB_E_%s = %d\b' % (name, v), hdr), name
    assert 'neck fusion backward' in hdr


def test_constructors_refuse_without_a_gpu():
    from rtm3d_amd import head_train as ht, neck_train as nt
    with pytest.raises(ValueError, match='fusion_scale = 3.0 is no power of two'):
        nt.FusionBackward(2, 16, 24, 'cpu', fusion_scale=3.0)
    with pytest.raises(ValueError, match='grad_scale = 100.0 is no power of two'):
        nt.FusionBackward(2, 16, 24, 'cpu', grad_scale=100.0)
    with pytest.raises(RuntimeError, match='multiples of 8'):
        nt.FusionBackward(2, 16, 20, 'cpu')
    with pytest.raises(RuntimeError, match='levels'):
        nt.FusionBackward(2, 16, 24, 'cpu', levels=4)
    with pytest.raises(TypeError, match='must be a TrainableHeads'):
        nt.TrainableFusion(object())
    heads = object.__new__(ht.TrainableHeads)
    heads._want_dz = False
    with pytest.raises(ValueError, match='without input_grad=True'):
        nt.TrainableFusion(heads)
    heads._want_dz = True
    with pytest.raises(ValueError, match='no power of two'):
        nt.TrainableFusion(heads, fusion_scale=12.0)
    assert ht._is_pow2(nt.DEFAULT_FUSION_SCALE)


def test_rotate_and_names():
    from rtm3d_amd import neck_train as nt
    w = torch.arange(3 * 5 * 16, dtype=torch.float32).reshape(3, 5, 4, 4).half()
    r = nt.rotate_deconv_weights(w)
    assert tuple(r.shape) == (16, 3, 5) and r.is_contiguous()
    assert float(r[4 * 2 + 1, 2, 4]) == float(w[2, 4, 2, 1])
    assert nt.weight_names() == [['kfpn_fusion.fusion_up3.0.conv_tran.weight'],
                                 ['kfpn_fusion.fusion_up4.%d.conv_tran.weight' % j for j in range(2)],
                                 ['kfpn_fusion.fusion_up5.%d.conv_tran.weight' % j for j in range(3)]]
    # the phase split of the gather tables is the plan's: sending a weight through it gives the plan's op weights
    from rtm3d_amd import plan as plan_mod
    wt = np.random.default_rng(0).standard_normal((6, 7, 4, 4)).astype(np.float32)
    P = plan_mod.Plan(1, 4, 4)
    P.deconv(P.tensor(4, 4, 6, 1), P.tensor(8, 8, 7, 0), wt, name='d')
    assert np.array_equal(np.stack(nt._deconv_group_src(wt), 0), P.ops[-1]['w'])
