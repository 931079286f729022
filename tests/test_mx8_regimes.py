"""CPU tests of the MXFP8 regime sweep: the host mirror (tests/mx8_regimes.py) against hand-worked launches, the L1 exactness
bound of every exact case of the GPU suite (tests/test_gpu_mx8_regimes.py), and the coverage guard: every regime value the sweep
names is run by some GPU case, and so is every regime of the head ops of the product's MXFP8 plans."""
import numpy as np
import pytest

from rtm3d_amd import plan, weights
from tests import mx8_ref as ref
from tests import mx8_regimes as mr


# ------------------------------------------------------------------------------ the mirror
def test_conv_mirror_hand_worked_product_shapes():
    # the d6 conv at 96 x 320, B = 1: 30720 pixels = 120 full tiles, 4 channel tiles, 9 taps x 4 chunks
    r = mr.conv(1, 96, 320, 256, 1024, 1, 9)
    assert (r['M'], r['MT'], r['NT'], r['cpt'], r['ksteps']) == (30720, 120, 4, 4, 36)
    assert r['grid'] == (480, 1) and r['last_rows'] == 256 and not r['second_half_dead'] and r['mod8'] == 0
    assert not r['tile_straddles'] and not r['partial_straddles']
    # n = 480, a multiple of 8: XCD x owns items [60 x, 60 x + 60); workgroup b = 8 k + x takes item 60 x + k
    assert r['item'](0) == (0, 0) and r['item'](1) == (15, 0) and r['item'](8) == (0, 1) and r['item'](479) == (119, 3)
    assert r['item'](8 * 7 + 3) == ((180 + 7) // 4, (180 + 7) % 4)
    # the d1 convs: 4 groups of 256 -> 256
    r = mr.conv(1, 96, 320, 256, 256, 4, 9)
    assert (r['MT'], r['NT'], r['ksteps'], r['grid'], r['mod8']) == (120, 1, 36, (120, 4), 0)
    assert r['item'](9) == (16, 0)
    # B = 32
    r = mr.conv(32, 96, 320, 256, 1024, 1, 9)
    assert (r['M'], r['MT'], r['grid']) == (983040, 3840, (15360, 1)) and not r['tile_straddles']
    r = mr.conv(32, 96, 320, 256, 256, 4, 9)
    assert (r['MT'], r['grid'], r['last_rows']) == (3840, (3840, 4), 256)


def test_conv_mirror_tile_boundaries():
    r = mr.conv(1, 15, 17, 64, 256, 1, 1)
    assert (r['M'], r['MT'], r['last_rows'], r['second_half_dead']) == (255, 1, 255, False)
    r = mr.conv(1, 16, 16, 64, 256, 1, 1)
    assert (r['M'], r['MT'], r['last_rows'], r['second_half_dead']) == (256, 1, 256, False)
    r = mr.conv(1, 1, 257, 64, 256, 1, 1)
    assert (r['M'], r['MT'], r['last_rows'], r['second_half_dead']) == (257, 2, 1, True)
    assert mr.conv(1, 8, 16, 64, 256, 1, 1)['second_half_dead']                  # 128 rows: exactly the first half
    assert not mr.conv(1, 3, 43, 64, 256, 1, 1)['second_half_dead']              # 129
    assert mr.conv(1, 1, 1, 64, 256, 1, 1)['grid'] == (1, 1)
    # 3 images of 130 pixels: tile 0 holds images 0 and 1, the 134-row tile 1 images 1 and 2
    r = mr.conv(3, 10, 13, 256, 512, 4, 9)
    assert (r['M'], r['MT'], r['NT'], r['last_rows']) == (390, 2, 2, 134) and r['tile_straddles'] and r['partial_straddles']
    assert r['grid'] == (4, 4) and r['mod8'] == 4
    # n = 4 < 8: q = 0, r = 4: workgroup b takes item b
    assert [r['item'](b) for b in range(4)] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # n = 9: XCD 0 owns items 0 and 1 (workgroups 0 and 8), XCD x > 0 item x + 1
    r = mr.conv(2, 12, 25, 512, 768, 1, 9)
    assert (r['MT'], r['NT'], r['cpt'], r['ksteps'], r['mod8']) == (3, 3, 8, 72, 1)
    assert [mr.xcd_contiguous_index(b, 9) for b in range(9)] == [0, 2, 3, 4, 5, 6, 7, 8, 1]


@pytest.mark.parametrize('n', [1, 2, 4, 7, 8, 9, 12, 16, 23, 480])
def test_xcd_order_is_a_permutation(n):
    assert sorted(mr.xcd_contiguous_index(b, n) for b in range(n)) == list(range(n))


def test_quant_mirror_hand_worked():
    assert mr.quant(1, 5, 7, 64) == {'nblk': 2, 'threads': 70, 'grid': 1, 'last_partial': True}
    assert mr.quant(2, 16, 16, 32) == {'nblk': 1, 'threads': 512, 'grid': 2, 'last_partial': False}
    assert mr.quant(3, 1, 1, 64) == {'nblk': 2, 'threads': 6, 'grid': 1, 'last_partial': True}
    assert mr.quant(1, 96, 320, 256) == {'nblk': 8, 'threads': 245760, 'grid': 960, 'last_partial': False}


# ------------------------------------------------------------------------------ the yardstick
def test_reference_conv_against_a_direct_loop():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 3, 4, 96))
    w = rng.standard_normal((2, 3, 5, 32))
    bias = rng.standard_normal((2, 5))
    taps, in_coff = [(-2, 1), (0, 0), (1, -1)], [64, 0]
    got = ref.conv(x, w, bias, taps, in_coff, True)
    for g in range(2):
        for n in range(2):
            for y in range(3):
                for xx in range(4):
                    acc = bias[g].copy()
                    for t, (dy, dx) in enumerate(taps):
                        if 0 <= y + dy < 3 and 0 <= xx + dx < 4:
                            acc += w[g, t] @ x[n, y + dy, xx + dx, in_coff[g]:in_coff[g] + 32]
                    np.testing.assert_allclose(got[g][n, y, xx], np.maximum(acc, 0), rtol=1e-12, atol=1e-12)


def test_quantum():
    assert ref.quantum(np.array([0.0, 6.0, -0.75, 1024.0])) == 0.25
    assert ref.quantum(np.array([3.0 * 2.0 ** -40, 2.0 ** 30])) == 2.0 ** -40
    assert ref.quantum(np.zeros(3)) == 0.0


@pytest.mark.parametrize('c', mr.CONV_CASES, ids=[c['name'] for c in mr.CONV_CASES])
def test_exact_case_satisfies_the_l1_bound(c):
    x, w, bias = ref.conv_case_data(c)                        # (asserts the bound itself)
    l1, q = ref.l1_exactness(x, w, bias, mr.TAPS[c['taps']], c['in_coff'])
    assert l1 < 2.0 ** 24 * q
    assert q <= 2.0 ** (c['sx'] + c['sw'] - 2 * c['spread']) * 4 and q >= 2.0 ** (c['sx'] + c['sw'] - 2 * c['spread'] - 2)
    # the taps stay inside the input border the case allocates (nothing is launched that the admission would refuse)
    assert mr.reach(mr.TAPS[c['taps']]) <= c['in_P']
    assert all(o % (8 if c['out'] == 'f16' else 32) == 0 for o in c['out_coff']) and all(i % 64 == 0 for i in c['in_coff']) and c['in_C'] % 64 == 0


# ------------------------------------------------------------------------------ coverage
def test_every_listed_conv_regime_is_run():
    run = set().union(*[mr.conv_case_values(c) for c in mr.CONV_CASES])
    missing = [v for v in mr.CONV_REQUIRED if v not in run]
    assert not missing, missing
    # dilations 1, 2 and 6 are what the 3 x 3 tap sets say
    assert mr.TAPS['d2'][0] == (-2, -2) and mr.TAPS['d6'][8] == (6, 6) and len(mr.TAPS['t80']) == 80 == len(set(mr.TAPS['t80']))
    assert all(dy < 0 and dx < 0 for dy, dx in mr.TAPS['neg'])
    # the case that must catch a swapped tap / chunk split
    c = next(c for c in mr.CONV_CASES if c['name'] == 't6_row_m255')
    assert len(mr.TAPS[c['taps']]) == 3 and c['cin'] == 128


def test_every_listed_quant_regime_is_run():
    run = set().union(*[mr.quant_case_values(q) for q in mr.QUANT_CASES])
    missing = [v for v in mr.QUANT_REQUIRED if v not in run]
    assert not missing, missing
    # every value class sits in some case's blocks
    seen = set()
    for name, B, H, W, in_C, in_coff, channels, in_P, out_C, out_coff, out_P, first in mr.QUANT_CASES:
        n = B * H * W * channels // 32
        seen |= {ref.VALUE_CLASSES[(first + i) % len(ref.VALUE_CLASSES)] for i in range(min(n, len(ref.VALUE_CLASSES)))}
    assert seen == set(ref.VALUE_CLASSES)


def test_epilogue_classes_of_the_exact_cases():
    """The output blocks the lane-pair reduction and the saturation need are in the reference of the case that claims them."""
    from rtm3d_amd import mx8
    c = next(c for c in mr.CONV_CASES if c['name'] == 'd6_cpt8_m600')
    x, w, bias = ref.conv_case_data(c)
    y = ref.conv(x, w, bias, mr.TAPS[c['taps']], c['in_coff'], c['relu'])[0].astype(np.float32)
    cls = ref.epilogue_classes(y)
    assert all(cls.values()), cls
    assert (mx8.quantize(y)[1] != 127).all()


@pytest.mark.parametrize('bb,nc,B,H,W', [('DLA-34', 1, 2, 64, 128), ('DLA-34', 2, 2, 64, 128), ('DLA-34', 3, 2, 64, 128), ('RESNET-18', 2, 2, 64, 128),
                                         ('DLA-34', 1, 1, 384, 1280), ('DLA-34', 2, 1, 384, 1280), ('DLA-34', 3, 32, 384, 1280), ('RESNET-18', 2, 1, 384, 1280)])
def test_every_regime_of_the_product_plans_is_run(bb, nc, B, H, W):
    sd = weights.synth_state_dict(bb, 1, 'trained', header_num_conv=nc)
    P = plan.build_plan(sd, bb, B, H, W, header_num_conv=nc, head_precision='mxfp8')
    conv_run = set().union(*[mr.conv_case_values(c) for c in mr.CONV_CASES])
    quant_run = set().union(*[mr.quant_case_values(q) for q in mr.QUANT_CASES])
    convs = [op for op in P.ops if op['op'] == 'conv_mx8']
    quants = [op for op in P.ops if op['op'] == 'quant_mx8']
    assert len(convs) == nc and len(quants) == 1
    for op in convs:
        missing = mr.plan_conv_values(P, op) - conv_run
        assert not missing, (op['name'], missing)
    for op in quants:
        missing = mr.plan_quant_values(P, op) - quant_run
        assert not missing, (op['name'], missing)
