"""Neck FPN backward without a GPU: the CPU yardsticks (tests/fpn_backward_ref.py) against the reference-run fixture and against
each other, the training lowering, the gather tables and every refusal that needs no device."""
import ctypes

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import fpn_backward_cases as cases
from tests import fpn_backward_ref as ref
from tests.util import load_golden

E_NULL, E_SHAPE, E_CIN, E_CHANNELS, E_SCALE, E_SLICES, E_BORDER, E_ALIGN, E_WORKSPACE = range(1, 10)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---------------------------------------------------------------------------------------------------- yardsticks
def test_r64_equals_the_reference_run():
    """fp64 autograd over the function as the reference writes it (head, up, cat, proj, every conv on its own) against what the
    reference's own _fpn and loss.backward() left: 1e-12 relative.  Pins the level order, the cat order [up | feat] and the layouts."""
    g = load_golden('neck_fpn_grad_cases.npz')
    params = cases.fixture_params(g)
    assert sorted(params) == sorted(ref.param_names())
    feats, G = [g['feat%d' % i] for i in range(4)], [g['G%d' % i] for i in range(4)]
    assert [f.shape for f in feats] == [(2, 8, 16, 24), (2, 16, 8, 12), (2, 24, 4, 6), (2, 32, 2, 3)]
    gf, gp, _ = ref.autograd_uncomposed(feats, params, G)
    for i in range(4):
        assert _rel(gf['feat%d' % i], g['g_feat%d' % i]) <= 1e-12, i
    for k in sorted(gp):
        assert _rel(gp[k], g['g:' + k]) <= 1e-12, k


def test_composed_chain_and_factor_rule_equal_the_reference_run():
    """The backward of the COMPOSED convs (the plan's function) plus the factor rule against the fixture: the identity is exact,
    so 1e-12 relative on every parameter and every feature gradient."""
    g = load_golden('neck_fpn_grad_cases.npz')
    case, params = cases.fixture_case(g), cases.fixture_params(g)
    assert (case['B'], case['H'], case['W'], case['C']) == (2, 16, 24, 8)
    r = ref.chain(case, False)
    got = cases.fixture_reference_grads(r, params)
    assert sorted(got) == sorted(params)
    for k in sorted(got):
        d = _rel(got[k], g['g:' + k])
        print('d %s: relative distance %.3e' % (k, d))
        assert got[k].shape == g['g:' + k].shape and d <= 1e-12, k
    C = case['C']
    for k in range(3):
        assert _rel(r['D'][k][:, C:].numpy(), g['g_feat%d' % k]) <= 1e-12, k
    assert _rel(r['dfeat3'].numpy(), g['g_feat3']) <= 1e-12
    # the composed forward is the reference's function
    _, _, outs = ref.autograd_uncomposed([g['feat%d' % i] for i in range(4)], params, [g['G%d' % i] for i in range(4)])
    ncat, h, z0 = ref.forward_composed([g['feat%d' % i] for i in range(4)], params)
    assert _rel(z0.numpy(), outs[0].numpy()) <= 1e-12
    for k in range(3):
        assert _rel(h[k].numpy(), outs[k + 1].numpy()) <= 1e-12
    # the written-out sums of the rule (layer_exact) are the same function as the chain's level 1
    dy = r['g'][0].permute(0, 2, 3, 1).numpy()
    dx, dA, db = ref.layer_exact(case['ncat'][1], case['A'][1], dy, 1.0, 1.0)
    assert _rel(dx.transpose(0, 3, 1, 2), r['D'][1].numpy()) <= 1e-12 and _rel(dA, r['dA'][1].numpy()) <= 1e-12 and _rel(db, r['db'][1].numpy()) <= 1e-12


def test_a_chain_without_the_fusion_terms_differs():
    """The fixture tells the full gradient at kfpn_h* from the kfpn_up path alone."""
    g = load_golden('neck_fpn_grad_cases.npz')
    case = cases.fixture_case(g)
    bare = dict(case, F=[np.zeros_like(f) for f in case['F']])
    assert _rel(ref.chain(bare, False)['dA'][1].numpy(), ref.chain(case, False)['dA'][1].numpy()) > 1e-2


@pytest.mark.parametrize('key', [(2, 8, 8, 4.0, 4.0), (2, 16, 24, 16.0, 4.0)])
def test_q16_against_r64(key):
    B, H, W, T, U = key
    S = 1024.0
    case = cases.real_case(6, B, H, W, S, T, U)
    r64, q = ref.chain(case, False), ref.chain(case, True)
    fr, fq, fl = ref.flat(r64, S * U), ref.flat(q), ref.floors(q)
    assert sorted(fr) == sorted(fq) == sorted(fl)
    for name in sorted(fr):
        assert np.isfinite(fq[name]).all() and np.isfinite(fr[name]).all(), name
        print('%s %s: max|ref| %.3e  Q16-R64 %.3e  floor %.3e' % (key, name, np.abs(fr[name]).max(), np.abs(fq[name] - fr[name]).max(), fl[name]))
        assert np.abs(fq[name]).max() < 65504.0 / 4
        assert np.abs(fq[name] - fr[name]).max() <= 4e-3 * np.abs(fr[name]).max() + 2.0 ** -24, name     # fp16: 2^-11 per rounding, up to seven in a row


def test_add_exact_specials():
    c = cases.add_case(1, 1, 2, 3, 0.5)
    g = ref.add_exact(c['e'], c['f'], c['r'])
    assert np.isnan(g[0, 0, 0, 0]) and g[0, 0, 0, 1] == np.inf and g[0, 0, 0, 2] == -np.inf and np.isnan(g[0, 0, 0, 3]) and np.isnan(g[0, 0, 0, 4])
    assert g[0, 0, 0, 5] == np.inf                                            # 65504 + 32752 rounds to Inf in fp16
    assert np.isfinite(g[0, 1:]).all()


# ---------------------------------------------------------------------------------------------------- the training lowering
_PLAN = {}


def _bench_plan():
    if not _PLAN:
        from rtm3d_amd import plan as plan_mod
        from rtm3d_amd.weights import synth_state_dict
        sd = synth_state_dict('DLA-34', seed=0)
        _PLAN['P'] = plan_mod.build_plan(sd, 'DLA-34', 32, 384, 1280)
    return _PLAN['P']


def _shape_of(low):
    return ([(L['kind'], L['name'], tuple(L['ops']), L.get('kernel'), L.get('bn_tile'), L['write_out']) for L in low['launches']],
            dict(low['widen']), sorted(low['unwritten']), sorted(low['s2d_only']), dict(low['stat_slots']))


def test_training_lowering_keeps_the_fpn_plain():
    from rtm3d_amd import plan as plan_mod, fpn_train
    P = _bench_plan()
    low = plan_mod.lower(P, neck_fold=False)
    assert not low['s2d_only'] and not low['widen']
    names = [L['name'] for L in low['launches']]
    kfpn = [n for n in names if n.startswith('kfpn_') and n != 'kfpn_softmax_fuse']
    assert kfpn == ['kfpn_head5', 'kfpn_up5', 'kfpn_proj5+head4', 'kfpn_up4', 'kfpn_proj4+head3', 'kfpn_up3', 'kfpn_proj3+head2']
    assert set(fpn_train.conv_launch_names()) <= set(names)
    by = {L['name']: L for L in low['launches']}
    for k, n in enumerate(fpn_train.conv_launch_names()):
        L = by[n]
        assert L['kind'] == 'conv' and L['write_out'] and L['s2d_out'] is None and L['in_s2d'] is None and len(L['ops']) == 1
        assert tuple(L['op']['w'].shape) == (1, 1, 256, (320, 384, 512, 512)[k])
        inp = L['op']['inp'][0]
        assert (inp.coff, inp.C) == (0, (320, 384, 512, 512)[k])
    named = P.named
    for k in range(3):                       # feat_k: a plain slice of the concat tensor behind the 256 up channels, border 1
        f, cat = named['feat%d' % k], by[fpn_train.conv_launch_names()[k]]['op']['inp'][0]
        assert f.tid == cat.tid and f.coff == 256 and f.C == (64, 128, 256)[k] and P.tensors[f.tid]['pad'] == 1
        up = by['kfpn_up%d' % (k + 3)]['op']
        assert up['out'][0].tid == cat.tid and (up['out'][0].coff, up['out'][0].C) == (0, 256)
    for key in [(named[n].tid, named[n].coff, named[n].C) for n in ('z0', 'kfpn_h3', 'kfpn_h4', 'kfpn_h5', 'feat3')]:
        assert key not in low['unwritten']
    # the default lowering is unchanged: None means the module's switch
    default = plan_mod.lower(P)
    assert plan_mod.FOLD_NECK_UP
    assert _shape_of(default) == _shape_of(plan_mod.lower(P, neck_fold=None)) == _shape_of(plan_mod.lower(P, neck_fold=True))
    assert default['widen'] and len(low['launches']) == len(default['launches']) + 3
    assert _shape_of(default) != _shape_of(low)


def test_gather_tables_match_the_packed_sizes():
    """Every gather table has the size of the array its launch's packer makes, holds every source index exactly once, and sends
    a weight through to the packer's own bytes."""
    from rtm3d_amd import plan as plan_mod, fpn_train
    P = _bench_plan()
    low = plan_mod.lower(P, neck_fold=False)
    launches, packed = {}, {}
    want = set(fpn_train.conv_launch_names()) | {'kfpn_up%d' % L for L in (3, 4, 5)}
    for L in low['launches']:
        if L['name'] in want:
            op, bn = L['op'], L['bn_tile']
            pack = plan_mod._CONV_PACKING[L['kernel']](op, bn)[2]
            launches[L['name']] = (pack, -(-op['cout'] // bn) * bn if bn else op['cout'])
            packed[L['name']] = np.concatenate([np.asarray(pack(op['w'][g])).reshape(-1) for g in range(op['groups'])])
    assert set(launches) == want
    cin = [320, 384, 512, 512]
    sizes = {n: s for n, s in zip(fpn_train.param_names(), [256 * 512, 256, 256 * 256 * 16, 256 * 512, 256, 256 * 256, 256, 256 * 256 * 16, 128 * 384, 128,
                                                             256 * 128, 256, 256 * 256 * 16, 64 * 320, 64, 256 * 64, 256])}
    off, at = {}, 0
    for n in fpn_train.param_names():
        off[n], at = at, at + sizes[n]
    doff = {}
    for key, n in [(('A', k), 256 * cin[k]) for k in range(3)] + [(('b', k), 256) for k in range(3)]:
        doff[key], at = at, at + n
    tables = fpn_train.gather_tables(off, doff, cin, launches)
    arena = np.zeros(at, np.float32)
    by = {L['name']: L['op'] for L in low['launches'] if L['name'] in want}
    for k, n in enumerate(fpn_train.conv_launch_names()):
        w0 = doff[('A', k)] if k < 3 else off['kfpn_fusion.kfpn_head5.weight']
        arena[w0:w0 + 256 * cin[k]] = by[n]['w'][0, 0].reshape(-1)
    for L in (3, 4, 5):
        ops = P.ops[[op.get('name') for op in P.ops].index('kfpn_up%d' % L)]
        # invert the phase split: the arena holds torch's (ci, co, 4, 4) weight
        idx = np.arange(256 * 256 * 16).reshape(256, 256, 4, 4)
        from rtm3d_amd import neck_train as nt
        flat = np.zeros(256 * 256 * 16, np.float32)
        for gsrc, gw in zip(nt._deconv_group_src(idx), ops['w']):
            flat[gsrc.reshape(-1)] = gw.reshape(-1)
        w0 = off['kfpn_fusion.kfpn_up%d.conv_tran.weight' % L]
        arena[w0:w0 + flat.size] = flat
    for name, (wperm, bperm) in tables.items():
        assert wperm.dtype == np.int32 and wperm.size == packed[name].size, name
        live = wperm[wperm >= 0]
        assert live.max() < at and len(np.unique(live)) == live.size, name
        got = np.where(wperm >= 0, arena[np.maximum(wperm, 0)], 0.0).astype(np.float16)
        assert got.tobytes() == np.asarray(packed[name], np.float16).tobytes(), name
        if bperm is not None:
            assert bperm.size == launches[name][1] and np.array_equal(bperm[:256] - bperm[0], np.arange(256)) and (bperm[256:] == -1).all()


# ---------------------------------------------------------------------------------------------------- refusals
def _err():
    return _lib.load().rtm3d_last_error().decode()


@pytest.mark.parametrize('args, code, word', [
    ((0, 16, 24, 320, 1.0), E_SHAPE, 'B, H, W'),
    ((2, 16, 24, 0, 1.0), E_CIN, 'multiples of 64'),
    ((2, 16, 24, 96, 1.0), E_CIN, 'multiples of 64'),
    ((2, 16, 24, 1088, 1.0), E_CIN, 'multiples of 64'),
    ((2, 16, 24, 320, 3.0), E_SCALE, 'power of two'),
    ((2, 16, 24, 320, 0.0), E_SCALE, 'power of two'),
    ((2, 16, 24, 320, 2.0 ** -130), E_SCALE, 'reciprocal'),
])
def test_check_refuses_by_name(args, code, word):
    assert _lib.load().rtm3d_fpn_backward_check(*args) == code
    assert word in _err()


def test_check_accepts_and_workspace_bytes():
    lib = _lib.load()
    assert lib.rtm3d_fpn_backward_check(2, 16, 24, 320, 2.0 ** -14) == 0
    assert lib.rtm3d_fpn_backward_check(32, 96, 320, 1024, 4.0) == 0
    assert lib.rtm3d_fpn_backward_check(1, 1, 1, 64, 1.0) == 0
    assert lib.rtm3d_fpn_backward_workspace_bytes(320, 4) == (4 * 256 * 320 + 1024 * 256) * 4
    assert lib.rtm3d_fpn_backward_workspace_bytes(96, 4) == 0 and lib.rtm3d_fpn_backward_workspace_bytes(320, 257) == 0
    assert lib.rtm3d_fpn_backward_workspace_bytes(320, 0) == 0


def _map(addr=4096, C=256, P=1, coff=0):
    return _lib.HbMapC(ctypes.c_void_p(addr), C, P, coff, 0)


def test_launch_functions_refuse_on_the_host_before_any_launch():
    """Made-up addresses: a refusal comes from the host checks, which touch neither the device nor the memory."""
    lib = _lib.load()
    ws, big, ctr = 1 << 20, 1 << 30, 1 << 12
    ref_ = lambda m: ctypes.byref(m) if m is not None else None
    wgrad = lambda x, dy, Cin=320, inv=1.0, want=4, wsb=big, w=ws, dA=1 << 16, db=1 << 14: lib.rtm3d_fpn_conv1x1_wgrad(
        None, 2, 4, 6, Cin, ref_(x), ref_(dy), inv, dA, db, want, w, wsb, ctr)
    X = lambda **kw: _map(**dict(dict(C=320), **kw))
    assert wgrad(None, _map()) == E_NULL and 'null' in _err()
    assert wgrad(X(addr=0), _map()) == E_NULL and 'NULL' in _err()
    assert wgrad(X(), _map(), Cin=100) == E_CIN and 'Cin' in _err()
    assert wgrad(X(C=256), _map()) == E_CHANNELS and 'channels' in _err()
    assert wgrad(X(), _map(C=128)) == E_CHANNELS
    assert wgrad(X(C=384, coff=72), _map()) == E_CHANNELS
    assert wgrad(X(), _map(), inv=3.0) == E_SCALE and 'inv' in _err()
    assert wgrad(X(), _map(), want=0) == E_SLICES and 'slices' in _err()
    assert wgrad(X(P=65), _map()) == E_BORDER and 'border' in _err()
    assert wgrad(X(addr=4104), _map()) == E_ALIGN and 'multiple of 16' in _err()
    assert wgrad(X(), _map(), w=ws + 8) == E_ALIGN and wgrad(X(), _map(), dA=(1 << 16) + 4) == E_ALIGN
    assert wgrad(X(), _map(), wsb=1024) == E_WORKSPACE and 'workspace' in _err()
    dgrad = lambda dy, wr, dx, Cin=320, mul=1.0: lib.rtm3d_fpn_conv1x1_dgrad(None, 2, 4, 6, Cin, ref_(dy), wr, mul, ref_(dx))
    assert dgrad(_map(), None, X()) == E_NULL
    assert dgrad(_map(), 4096, None) == E_NULL
    assert dgrad(_map(), 4100, X()) == E_ALIGN
    assert dgrad(_map(), 4096, X(), Cin=32) == E_CIN
    assert dgrad(_map(), 4096, X(C=256)) == E_CHANNELS
    assert dgrad(_map(), 4096, X(), mul=6.0) == E_SCALE and 'mul' in _err()
    assert dgrad(_map(P=-1), 4096, X()) == E_BORDER
    add = lambda e, f, g, r=1.0, B=2: lib.rtm3d_fpn_grad_add(None, B, 4, 6, ref_(e), ref_(f), r, ref_(g))
    assert add(None, _map(), _map()) == E_NULL
    assert add(_map(), _map(), _map(), B=0) == E_SHAPE
    assert add(_map(), _map(C=128), _map()) == E_CHANNELS
    assert add(_map(), _map(), _map(), r=0.3) == E_SCALE and 'r =' in _err()
    assert add(_map(), _map(addr=4100), _map()) == E_ALIGN
    assert add(_map(), _map(), _map(P=100)) == E_BORDER


def test_header_names_the_codes_and_the_abi_version_stays():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rtm3d_hip.h')).read()
    for name, v in (('NULL', E_NULL), ('SHAPE', E_SHAPE), ('CIN', E_CIN), ('CHANNELS', E_CHANNELS), ('SCALE', E_SCALE),
                    ('SLICES', E_SLICES), ('BORDER', E_BORDER), ('ALIGN', E_ALIGN), ('WORKSPACE', E_WORKSPACE), ('LAUNCH', 10)):
        assert re.search(r'RTM3D_FB_E_%s = %d\b' % (name, v), hdr), name
    assert 'neck FPN backward' in hdr and re.search(r'#define RTM3D_ABI_VERSION 9\b', hdr)


def test_constructors_refuse_without_a_gpu():
    from rtm3d_amd import head_train as ht, fpn_train as ft
    with pytest.raises(ValueError, match='fpn_scale = 3.0 is no power of two'):
        ft.FpnBackward(2, 16, 24, 'cpu', fpn_scale=3.0)
    with pytest.raises(ValueError, match='grad_scale = 100.0 is no power of two'):
        ft.FpnBackward(2, 16, 24, 'cpu', grad_scale=100.0, fpn_scale=4.0)
    with pytest.raises(ValueError, match='multiples of 8'):
        ft.FpnBackward(2, 16, 20, 'cpu', fpn_scale=4.0)
    with pytest.raises(RuntimeError, match='multiples of 64'):
        ft.FpnBackward(2, 16, 24, 'cpu', feat_channels=(64, 128, 256, 500), fpn_scale=4.0)
    with pytest.raises(ValueError, match='four feature widths'):
        ft.FpnBackward(2, 16, 24, 'cpu', feat_channels=(64, 128, 256), fpn_scale=4.0)
    with pytest.raises(TypeError, match='must be a TrainableHeads'):
        ft.TrainableNeck(object())
    assert ht._is_pow2(ft.DEFAULT_FPN_SCALE)
    assert ft.param_names()[:5] == ['kfpn_fusion.kfpn_head5.weight', 'kfpn_fusion.kfpn_head5.bias', 'kfpn_fusion.kfpn_up5.conv_tran.weight',
                                    'kfpn_fusion.kfpn_proj5.weight', 'kfpn_fusion.kfpn_proj5.bias'] and len(ft.param_names()) == 17
    import torch
    a = torch.arange(256 * 64, dtype=torch.float32).reshape(256, 64, 1, 1).half()
    t = ft.transpose_weights(a)
    assert tuple(t.shape) == (64, 256) and t.is_contiguous() and float(t[3, 5]) == float(a[5, 3, 0, 0])
