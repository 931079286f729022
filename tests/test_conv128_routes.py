"""The host mirror of where the 128-pixel and halo conv kernels run a launch (tests/conv128_routes.py), checked by hand-worked
launches; the GPU cases of tests/test_gpu_conv128.py against it; and a coverage guard: every regime the product plans send to
these kernels is one that some GPU case runs."""
import numpy as np
import pytest

from rtm3d_amd import _lib, plan as plan_mod, weights
from tests import conv128_routes as cr
from tests import test_gpu_conv128 as gpu_cases
from tests.abi_recorder import pin_switches, record


def test_route_of_names():
    assert cr.route_of('conv3x3_mfma') == 'one_stage' and cr.route_of('conv1x1_mfma_deep') == 'deep'
    assert cr.route_of('deconv4x4_phase_mfma_deep_splitk') == 'deep_splitk'
    assert [cr.route_of(n) for n in ('conv3x3_c64_halo', 'conv3x3_c128_halo', 'conv3x3s2_c64_halo')] == ['c64_halo', 'c128_halo', 'c64s2_halo']
    for bad in ('conv3x3_mfma256', 'conv1x1_mfma256_1tile', 'conv3x3_mfma256_halo', 'deconv4x4_phase_mfma256_lattice',
                'conv3x3_mfma_splitk', 'conv_smallc_regmfma', 'conv3x3_headout_halo'):
        with pytest.raises(ValueError):
            cr.route_of(bad)


def test_admit_mfma128_by_hand():
    # DLA-34 bs=1 level5 3x3 512 -> 512 (12 x 40 = 480 px): 4 pixel tiles x 8 channel tiles = 32 workgroups, 72 k-steps
    r = cr.admit_mfma128(480, 512, 512, 9)
    assert (r['route'], r['MT'], r['NT'], r['wgs'], r['ksteps'], r['ks']) == ('deep_splitk', 4, 8, 32, 72, 8)
    assert r['ranges'][:2] == [(0, 9), (9, 18)] and r['slab_floats'] == 8 * 32 * 128 * 64
    assert r['grid'] == (64, 1, 8) and r['empty_xcds'] == 4 and r['idle'] == 4 * 8 * 8     # chunk 1: XCDs 4-7 have no tile
    # the boundaries: wgs * 2 <= cus, ksteps >= 8, wgs <= cus
    assert cr.admit_mfma128(128 * 128, 64, 64, 9)['ks'] == 2
    assert cr.admit_mfma128(129 * 128, 64, 64, 9)['route'] == 'deep'
    assert cr.admit_mfma128(256 * 128, 64, 64, 9)['route'] == 'deep'
    assert cr.admit_mfma128(257 * 128, 64, 64, 9)['route'] == 'one_stage'
    assert cr.admit_mfma128(2048, 448, 64, 1)['route'] == 'deep' and cr.admit_mfma128(2048, 512, 64, 1)['ks'] == 2
    # ks capped by ksteps // 4 and by 16; uneven ranges
    r = cr.admit_mfma128(1664, 64, 64, 13)
    assert (r['wgs'], r['ks'], r['ranges']) == (13, 3, [(0, 4), (4, 8), (8, 13)])
    assert cr.admit_mfma128(2048, 512, 128, 9, bn=128)['ks'] == 16
    # BN 16 / 32 and NCHW always run one-stage; NCHW pads a ragged cout to the tile
    assert cr.admit_mfma128(128, 64, 64, 9, bn=32)['route'] == 'one_stage'
    r = cr.admit_mfma128(600, 64, 3, 9, bn=16, nchw=True)
    assert (r['route'], r['cout_pad'], r['MT'], r['empty_xcds'], r['grid']) == ('one_stage', 16, 5, 3, (8, 1, 1))
    # groups multiply the workgroups: four transposed-conv phases of 16 pixel tiles
    r = cr.admit_mfma128(2048, 128, 64, 4, groups=4)
    assert (r['wgs'], r['ks'], r['grid']) == (64, 2, (16, 4, 2))
    # ragged MT: 212 pixel tiles in chunks of 27, the last XCD gets 23
    r = cr.admit_mfma128(27090, 64, 128, 9)
    assert (r['MT'], r['chunk'], r['grid'][0], r['idle']) == (212, 27, 432, 8)


def test_halo_regimes_by_hand():
    assert cr.halo('c64_halo', 1, 96, 320) == {'total': 120, 'grid': 120, 'single': True, 'first_draw_busy': None, 'mod3': None}
    r = cr.halo('c64_halo', 32, 96, 320)
    assert (r['total'], r['grid'], r['single'], r['first_draw_busy'], r['mod3']) == (3840, 256, False, 256, 0)
    r = cr.halo('c128_halo', 1, 8, 4128, 256)
    assert (r['total'], r['first_draw_busy'], r['mod3']) == (258, 86, 0)
    assert cr.halo('c128_halo', 4, 64, 256, 128)['single'] and not cr.halo('c128_halo', 1, 8, 8224, 128)['single']
    assert cr.halo('c64s2_halo', 8, 48, 160)['total'] == 8 * 12 * 5


def test_gpu_cases_match_the_mirror():
    """Every GPU case's declared route and regime is what the mirror says (so a wrong case table shows up without a GPU)."""
    for name, sp in list(gpu_cases.CASES.items()) + list(gpu_cases.CHAIN.items()):
        gpu_cases.check_regime(sp)
    splits = {gpu_cases.mirror(sp)['ks'] for sp in gpu_cases.CASES.values() if sp['route'] == 'deep_splitk'}
    assert {2, 3, 4, 5, 8, 9, 16} <= splits, splits
    c128 = {(sp['cin'], sp['cout']) for sp in gpu_cases.CASES.values() if sp['kernel'] == 'c128_halo'}
    assert {(ci, co) for ci in (128, 256, 384, 512) for co in (128, 256, 384)} <= c128
    for kernel in ('c64_halo', 'c128_halo'):
        totals = {gpu_cases.mirror(sp)['total'] for sp in gpu_cases.CASES.values() if sp['kernel'] == kernel}
        assert {1, 256, 257, 258, 259} <= totals and max(totals) >= 768, (kernel, totals)


_KERNELS = {_lib.CONV_MFMA128: 'mfma128', _lib.CONV_C64_HALO: 'c64_halo', _lib.CONV_C128_HALO: 'c128_halo', _lib.CONV_C64S2_HALO: 'c64s2_halo'}


def product_regimes(calls):
    """Regime keys of the rtm3d_op_conv launches of a recorded call log that run on the 128-pixel or halo kernels."""
    tensors, keys = [], {}
    for fn, args in calls:
        if fn == 'rtm3d_tensor_create':
            tensors.append(args)
        if fn != 'rtm3d_op_conv' or args[0]['kernel'] not in _KERNELS:
            continue
        d = args[0]
        kernel, G, B = _KERNELS[d['kernel']], d['groups'], tensors[d['in_tensor']][0]
        s2d = 'input' if d['in_s2d'] else ('' if not d['s2d_tensor'] else ('only' if d['out_tensor'] < 0 else 'copy'))
        flags = dict(nchw=d['out_nchw_f32'] > 0, res=d['res_tensor'] >= 0, s2d=s2d, grouped=G > 1,
                     tap_dc=any(any(dc[:d['ntaps']]) for dc in d['tap_dc'][:G]), stride=d['in_stride'], out_scale=d['out_scale'])
        if kernel == 'mfma128':
            r = cr.admit_mfma128(B * d['Hm'] * d['Wm'], d['cin'], d['cout'], d['ntaps'], G, d['bn_tile'], d['out_nchw_f32'] > 0)
            key = cr.regime_key(kernel, r['route'], r['bn'], r['ks'], **flags)
        else:
            key = cr.regime_key(kernel, kernel, single=cr.halo(kernel, B, d['Hm'], d['Wm'], d['cout'])['single'], **flags)
        keys.setdefault(key, d)
    return keys


def test_every_product_regime_has_a_gpu_case(monkeypatch):
    pin_switches(monkeypatch)
    sds = {bb: weights.synth_state_dict(bb, 3, 'trained') for bb in ('DLA-34', 'RESNET-18', 'RESNET-34')}
    plans = [('DLA-34', B, H) for B in (1, 2, 32) for H in (384, 416)] + [('RESNET-18', 8, 384), ('RESNET-34', 8, 384)]
    builds = [lambda bb=bb, B=B, H=H: plan_mod.build_plan(sds[bb], bb, B, H, 1280) for bb, B, H in plans]
    builds.append(lambda: plan_mod.build_peak_plan(sds['DLA-34'], 3200, (96, 320)))
    covered = {gpu_cases.regime(sp) for sp in gpu_cases.CASES.values()}
    missing = {}
    for build in builds:
        for key, d in product_regimes(record(build()).calls).items():
            if key not in covered:
                missing[key] = (d['Hm'], d['Wm'], d['cin'], d['cout'], d['ntaps'])
    assert not missing, missing


def test_grouped_nchw_output_records_group_channel_offsets():
    """A grouped conv with an fp32 NCHW output: group g's channels follow group g - 1's in the slot (out_coff = g * cout)."""
    P = plan_mod.Plan(1, 48, 80)
    x = P.tensor(12, 20, 128, 1)
    ws = [np.zeros((3, 64, 9), np.float32)] * 2
    P.conv_taps([P.sub(x, 0, 64), P.sub(x, 64, 64)], [None, None], ws, [np.zeros(3, np.float32)] * 2,
                [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)], 12, 20, name='g', out_nchw=2)
    (d,) = [a[0] for fn, a in record(P).calls if fn == 'rtm3d_op_conv']
    assert (d['out_tensor'], d['out_nchw_f32'], d['groups'], d['out_coff'][:2]) == (-1, 2, 2, [0, 3])
