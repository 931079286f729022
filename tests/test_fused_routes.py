"""The host mirror of where the fused DLA backbone kernels run a launch (tests/fused_routes.py), checked by hand-worked launches;
the GPU cases of tests/test_gpu_fused.py against it; and a coverage guard: every regime the DLA-34 plans send to these kernels is
one that some GPU case runs."""
import pytest

from rtm3d_amd import plan as plan_mod, weights
from tests import fused_routes as fr
from tests import test_gpu_fused as gpu_cases
from tests.abi_recorder import pin_switches, record


def test_root_instances_and_names():
    assert fr.root_instance(True, False, True) == (1, 0, 1) and fr.root_instance(1, 1, 0) == (1, 1, 0)
    assert fr.root_instance(0, 1, 0) == (0, 1, 0) and fr.root_instance(0, 0, 1) == (0, 0, 1)
    assert sorted(fr.ROOT_INSTANCES) == sorted((p, s, n) for p in (0, 1) for s in (0, 1) for n in (0, 1) if s or n)
    with pytest.raises(ValueError):
        fr.root_instance(1, 0, 0)
    assert fr.root_name(1, 1) == 'conv3x3_c64+root1x1+pool_fused+s2d' and fr.root_name(0, 0) == 'conv3x3_c64+root1x1_fused'


def test_conv64_root_regimes_by_hand():
    # DLA-34 level2 tail: B = 1 runs <1,0,1> on 96 x 320 (12 x 10 items) or 104 x 320 (13 x 10), one item per workgroup
    assert fr.conv64_root(1, 96, 320, 1, 0) == {'total': 120, 'grid': 120, 'single': True, 'first_draw_busy': None, 'mod3': None,
                                               'instance': (1, 0, 1)}
    assert fr.conv64_root(1, 104, 320, 1, 0)['total'] == 130
    # B >= 2 runs <1,1,0>: 2 x 384 fits the CUs, 2 x 416 draws tickets (87 first draws of three, the last one two items short)
    assert fr.conv64_root(2, 96, 320, 1, 1, out=False)['single']
    r = fr.conv64_root(2, 104, 320, 1, 1, out=False)
    assert (r['total'], r['grid'], r['single'], r['first_draw_busy'], r['mod3'], r['instance']) == (260, 256, False, 87, 2, (1, 1, 0))
    r = fr.conv64_root(32, 96, 320, 1, 1, out=False)
    assert (r['total'], r['grid'], r['first_draw_busy'], r['mod3']) == (3840, 256, 256, 0)
    # the ticket boundaries: 256 single, 257 / 258 / 259 tickets
    assert fr.conv64_root(4, 64, 256, 0, 0)['single'] and fr.conv64_root(1, 8, 8224, 0, 1)['mod3'] == 2
    assert fr.conv64_root(2, 8, 4128, 1, 1, out=False)['first_draw_busy'] == 86 and fr.conv64_root(7, 296, 32, 1, 1)['mod3'] == 1
    with pytest.raises(AssertionError):
        fr.conv64_root(1, 12, 32, 1, 0)


def test_conv32s2_stem_and_pool_by_hand():
    # level entry: items on the half-resolution output map (input 192 x 640 per image at 384 x 1280)
    assert fr.conv32s2(1, 96, 320)['total'] == 120 and fr.conv32s2(1, 96, 320)['single']
    r = fr.conv32s2(2, 104, 320)
    assert (r['total'], r['single'], r['mod3'], r['first_draw_busy']) == (260, False, 2, 87)
    assert fr.conv32s2(32, 104, 320)['total'] == 4160 and fr.conv32s2(1, 8, 32)['total'] == 1
    # stem: 16 x 32 full-resolution tiles
    assert fr.stem(1, 384, 1280, 3) == {'layers': 3, 'grid': 960, 'out_scale': 2, 'out_channels': 32}
    assert fr.stem(32, 416, 1280, 3)['grid'] == 32 * 26 * 40 and fr.stem(2, 32, 64, 2)['out_channels'] == 16
    # maxpool_s2d: the DLA-34 bs=32 plan's two launches fill their last block; 5 x 7 x 8 channels leaves 221 lanes idle
    assert fr.maxpool_s2d(32, 24, 80, 128) == {'threads': 983040, 'blocks': 3840, 'idle': 0}
    assert fr.maxpool_s2d(32, 13, 40, 256)['idle'] == 0
    assert fr.maxpool_s2d(1, 5, 7, 8) == {'threads': 35, 'blocks': 1, 'idle': 221}
    with pytest.raises(ValueError):
        fr.regime_key('conv3x3_c64_halo')


def test_gpu_cases_match_the_mirror():
    """Every GPU case's declared regime is what the mirror says (a wrong case table shows up without a GPU), and the table
    covers what the kernels' regimes hinge on."""
    for name, sp in list(gpu_cases.CASES.items()) + list(gpu_cases.CHAIN.items()):
        gpu_cases.check_regime(sp)
    cases = list(gpu_cases.CASES.values())
    roots = [(gpu_cases.mirror(sp), sp) for sp in cases if sp['kind'] == 'conv64_root']
    assert {(r['instance'], r['single']) for r, _ in roots} == {(i, s) for i in fr.ROOT_INSTANCES for s in (True, False)}
    assert any(not sp['conv_relu'] for _, sp in roots) and any(not sp['root_relu'] for _, sp in roots)
    assert any(sp['shared'] == 'pool_first' for _, sp in roots) and any(sp['shared'] == 's2d_first' for _, sp in roots)
    for kind in ('conv64_root', 'conv32s2_fused'):
        totals = {gpu_cases.mirror(sp)['total'] for sp in cases if sp['kind'] == kind}
        assert {1, 256, 257, 258, 259} <= totals and max(totals) >= 768, (kind, totals)
    assert any(sp['shared'] for sp in cases if sp['kind'] == 'conv32s2_fused')
    stems = [sp for sp in cases if sp['kind'] == 'stem_fused']
    assert {sp['layers'] for sp in stems} == {2, 3} and any((sp['H'], sp['W']) == (384, 1280) for sp in stems)
    assert all(sp['o_lo'] and sp['o_hi'] for sp in stems if (sp['H'], sp['W']) == (384, 1280))
    pools = [(gpu_cases.mirror(sp), sp) for sp in cases if sp['kind'] == 'maxpool_s2d']
    assert {sp['C'] for _, sp in pools} >= {8, 128, 256} and any(r['idle'] for r, _ in pools) and any(sp['shared'] for _, sp in pools)
    assert {(sp['C'], sp['in_lo'], sp['o_lo']) for _, sp in pools} >= {(128, 256, 512), (256, 256, 1024)}
    chain = {gpu_cases.regime(sp) for sp in gpu_cases.CHAIN.values()}
    assert {fr.regime_key('conv64_root', single=s, instance=i, conv_relu=True, root_relu=True)
            for i, s in (((1, 1, 0), False), ((1, 0, 1), True))} <= chain
    assert {fr.regime_key('conv32s2_fused', single=s) for s in (True, False)} <= chain


def product_regimes(calls):
    """Regime keys of the fused launches (stem, level entry, level tail, space-to-depth max-pool) of a recorded call log."""
    tensors, keys = [], {}
    for fn, a in calls:
        if fn == 'rtm3d_tensor_create':
            tensors.append(a)                           # [B, H, W, C, pad]
        elif fn == 'rtm3d_op_stem_fused':
            B, H, W = tensors[a[0]][:3]
            keys.setdefault(fr.regime_key('stem_fused', layers=3 if a[7] >= 0 else 2), (B, H, W))
        elif fn == 'rtm3d_op_conv32s2_fused':
            B, H, W = tensors[a[0]][:3]
            keys.setdefault(fr.regime_key('conv32s2_fused', single=fr.conv32s2(B, H // 2, W // 2)['single']), (B, H, W))
        elif fn == 'rtm3d_op_conv64_root':
            B, H, W = tensors[a[0]][:3]
            r = fr.conv64_root(B, H, W, a[12] >= 0, a[14] >= 0, a[9] >= 0)
            keys.setdefault(fr.regime_key('conv64_root', single=r['single'], instance=r['instance'], conv_relu=a[4], root_relu=a[11]),
                            (B, H, W))
        elif fn == 'rtm3d_op_maxpool_s2d':
            B, H, W = tensors[a[2]][:3]
            keys.setdefault(fr.regime_key('maxpool_s2d', channels=a[4], idle=fr.maxpool_s2d(B, H, W, a[4])['idle']), (B, H, W))
    return keys


def test_every_product_regime_has_a_gpu_case(monkeypatch):
    pin_switches(monkeypatch)
    sd = weights.synth_state_dict('DLA-34', 3, 'trained')
    covered = {gpu_cases.regime(sp) for sp in gpu_cases.CASES.values()}
    seen, missing = set(), {}
    for B in (1, 2, 32):
        for H in (384, 416):
            for key, where in product_regimes(record(plan_mod.build_plan(sd, 'DLA-34', B, H, 1280)).calls).items():
                seen.add(key)
                if key not in covered:
                    missing[key] = where
    assert not missing, missing
    # the plans do reach every fused kind, the tail in both of its forms and in both regimes
    assert {k[0] for k in seen} == {'stem_fused', 'conv32s2_fused', 'conv64_root', 'maxpool_s2d'}, seen
    assert {(k[1], k[2]) for k in seen if k[0] == 'conv64_root'} == {((1, 0, 1), True), ((1, 1, 0), True), ((1, 1, 0), False)}, seen
