"""The host mirror of the register-direct small-channel conv launches (tests/smallc_routes.py), checked by hand-worked launches
of the product shapes; the GPU cases of tests/test_gpu_smallc.py against it; a coverage guard (every instance and regime the
ResNet and DLA-34 plans send to kernel 3 is one that some GPU case runs); the exactness condition of the bit-for-bit cases,
from the reference operands alone; and the lowering of 16 -> 16 convs whose taps the vertical-walk kernel does not take."""
import numpy as np
import pytest

from rtm3d_amd import _lib, plan as plan_mod, weights
from tests import smallc_routes as sr
from tests import test_gpu_smallc as gpu_cases
from tests.abi_recorder import pin_switches, record

T4_64, T4_16, T16_16, T16_32, T32_64, T32_64P = (gpu_cases.T4_64, gpu_cases.T4_16, gpu_cases.T16_16, gpu_cases.T16_32, gpu_cases.T32_64,
                                                 gpu_cases.T32_64P)
R4_16, R16_16 = gpu_cases.R4_16, gpu_cases.R16_16


def test_instances_and_names():
    assert sr.instance(4, 64, 49, 2) == ('tile', 4, 4, 7, 8) and sr.instance(4, 16, 49, 2) == ('tile', 4, 1, 7, 8)
    assert sr.instance(4, 16, 49) == ('rows', 4, 1, 7, 1, 32) and sr.instance(4, 16, 49, 1, 2) == ('tile', 4, 1, 7, 8)
    assert sr.instance(16, 16, 9, rows_packing=True) == ('rows', 16, 1, 3, 2, 32) and sr.instance(16, 16, 9) == ('tile', 16, 1, 5, 8)
    assert sr.instance(16, 32, 9, 2) == ('tile', 16, 2, 5, 8) and sr.instance(32, 64, 9, 2) == ('tile', 32, 2, 9, 8)
    assert sr.instance(32, 64, 1) == ('tile', 32, 4, 1, 8)
    assert len(sr.INSTANCES) == 8 and len(set(sr.INSTANCES)) == 8
    assert [sr.ksteps(i) for i in (T4_64, R4_16, R16_16, T16_16, T32_64, T32_64P)] == [7, 7, 6, 5, 9, 1]
    assert sr.op_name(4) == 'stem7x7_regmfma' and sr.op_name(16) == sr.op_name(32) == 'conv_smallc_regmfma'
    for bad in ((16, 64, 9), (32, 32, 9), (4, 32, 49), (8, 16, 9), (32, 64, 25)):
        with pytest.raises(ValueError):
            sr.instance(*bad)
    with pytest.raises(ValueError):
        sr.instance(16, 16, 9, 2, rows_packing=True)


def test_product_launches_by_hand():
    # ResNet conv1 (7x7 stride 2, 4 -> 64): 192 x 640 or 208 x 640 output pixels per image, 512 to a block, nothing ragged
    for B, H, grid_x in ((1, 384, 240), (32, 384, 7680), (1, 416, 260), (32, 416, 8320)):
        r = sr.launch(B, H, 1280, 4, 64, 49, 2)
        assert (r['instance'], r['op'], r['grid'], r['M']) == (T4_64, 'stem7x7_regmfma', (grid_x, 1), B * (H // 2) * 640), r
        assert (r['m_mod16'], r['ntiles_mod8'], r['idle_waves'], r['row_straddles'], r['image_straddles'], r['store_bytes']) == (0, 0, 0, 0, 0, 16)
    # the unfused DLA stem: base_layer and level0 walk 80 column strips x 12 (13) row strips per image; level1 is conv1's grid
    for B, H, strips in ((1, 384, 12), (2, 416, 13)):
        for cin, inst, rp in ((4, R4_16, False), (16, R16_16, True)):
            r = sr.launch(B, H, 1280, cin, 16, 49 if cin == 4 else 9, rows_packing=rp)
            assert (r['instance'], r['tiles_x'], r['strips_y'], r['nwaves'], r['grid']) == (inst, 80, strips, B * strips * 80, (B * strips * 20, 1)), r
            assert (r['w_mod16'], r['h_mod32'], r['last_rows'], r['nwaves_mod4'], r['store_bytes']) == (0, 0, 32, 0, 8)
    r = sr.launch(1, 384, 1280, 16, 32, 9, 2)
    assert (r['instance'], r['grid'], r['op'], r['store_bytes']) == (T16_32, (240, 1), 'conv_smallc_regmfma', 16)
    # the unfused level-2 entry on the 192 x 640 map: the 3x3 stride-2 conv (two channel halves on grid.y) and the 1x1 on the pooled map
    r = sr.launch(1, 192, 640, 32, 64, 9, 2)
    assert (r['instance'], r['M'], r['ntiles'], r['grid'], r['idle_waves']) == (T32_64, 30720, 1920, (60, 2), 0)
    r = sr.launch(1, 96, 320, 32, 64, 1)
    assert (r['instance'], r['grid'], r['ksteps']) == (T32_64P, (60, 1), 1)
    # edges: a last tile of 14 pixels, a run that ends after 7 tiles, tiles over row ends and an image boundary
    r = sr.launch(1, 37, 51, 4, 64, 49, 2)
    assert (r['Hm'], r['Wm'], r['M'], r['m_mod16'], r['ntiles'], r['ntiles_mod8'], r['idle_waves']) == (19, 26, 494, 14, 31, 7, 0)
    r = sr.launch(3, 5, 6, 32, 64, 1)
    assert (r['M'], r['ntiles'], r['idle_waves'], r['image_straddles']) == (90, 6, 3, 2) and r['row_straddles'] == 6
    r = sr.launch(1, 33, 40, 4, 16, 49)
    assert (r['tiles_x'], r['w_mod16'], r['strips_y'], r['h_mod32'], r['last_rows'], r['nwaves_mod4']) == (3, 8, 2, 1, 1, 2)
    assert sr.nchw_to_nhwc4(32, 384, 1280) == {'threads': 15728640, 'blocks': 61440, 'idle': 0}
    assert sr.nchw_to_nhwc4(3, 5, 7) == {'threads': 105, 'blocks': 1, 'idle': 151}


def test_gpu_cases_match_the_mirror():
    """Every GPU case's declared instance and regime is what the mirror says, and the table reaches the edges of every
    instance."""
    cases = list(gpu_cases.CASES.items())
    for name, sp in cases + list(gpu_cases.CHAIN.items()):
        assert 'instance' in sp['expect'], name
        gpu_cases.check_regime(sp)
    by = {}
    for name, sp in cases:
        by.setdefault(gpu_cases.mirror(sp)['instance'], []).append((sp, gpu_cases.mirror(sp)))
    assert set(by) == set(sr.INSTANCES)
    for inst, lst in by.items():
        assert {sp['mode'] for sp, _ in lst} == {'exact', 'random'}, inst
        assert {sp['relu'] for sp, _ in lst if sp['mode'] == 'exact'} == {True, False}, inst
        assert {sp['out_P'] for sp, _ in lst} >= ({0, 1, 2} if inst not in (T4_16, T16_16) else {0, 1}), inst
        assert any(sp['in_P'] > max(max(abs(dy), abs(dx)) for dy, dx in sp['taps']) and (sp['cin'] != 4 or sp['in_P'] > 4) for sp, _ in lst), inst
        if inst[1] != 4:
            assert any(sp['in_lo'] for sp, _ in lst) and any(sp['in_hi'] for sp, _ in lst), inst
        if inst[0] == 'rows':
            assert {r['nwaves_mod4'] for _, r in lst} >= {0, 1, 2, 3}, inst
            assert {r['last_rows'] for _, r in lst} >= {1, 6, 20, 32} and {r['w_mod16'] for _, r in lst} >= {0, 1, 8}, inst
            assert any(sp['B'] > 1 for sp, _ in lst) and any(r['strips_y'] == 3 for _, r in lst), inst
            assert any(sp['ramp'] and r['strips_y'] > 1 for sp, r in lst), inst
        else:
            assert any(r['m_mod16'] for _, r in lst) and any(r['ntiles_mod8'] for _, r in lst) and any(r['row_straddles'] for _, r in lst), inst
            assert any(r['image_straddles'] for _, r in lst), inst
            if lst[0][1]['store_bytes'] == 16:
                # a 16-byte store at channel offset 8 of a tensor whose channel count is 8 mod 16
                assert any(sp['out_lo'] % 16 == 8 and (sp['out_lo'] + sp['cout'] + sp['out_hi']) % 16 == 8 for sp, _ in lst), inst
    for inst in (T4_64, T32_64, T32_64P):
        assert any(r['idle_waves'] == 3 for _, r in by[inst]), inst
    # taps off the 3x3 grid on the per-tile instances that index every tap
    for inst in (T16_16, T16_32, T32_64):
        assert any(sp['dil'] == 2 or sp['explicit'] for sp, _ in by[inst] if sp['mode'] == 'exact'), inst


def test_exact_cases_are_exact_in_fp32():
    """In units of (input quantum) x (weight quantum), sum |w x| + |bias| of every output of every exact case is below 2^24:
    whatever order the kernel sums in, every partial sum is an fp32 number and the result is rounded to fp16 once."""
    n = 0
    for name, sp in list(gpu_cases.CASES.items()) + list(gpu_cases.CHAIN.items()):
        if sp['mode'] != 'exact':
            continue
        ops = gpu_cases.operands(sp, gpu_cases.case_seed(name))
        lo = sp['in_lo']
        x = ops['x'][..., lo:lo + sp['cin']].astype(np.float64)
        units = (ops['w'].astype(np.float64) / gpu_cases.WQ, ops['b'].astype(np.float64) / gpu_cases.WQ)
        assert np.array_equal(x, np.round(x)) and all(np.array_equal(u, np.round(u)) for u in units), name
        assert gpu_cases.exactness_units(sp, ops) < 2 ** 24, (name, gpu_cases.exactness_units(sp, ops))
        # operands that cannot cancel: weights differ along every axis, inputs from pixel to pixel
        w = ops['w'] if sp['cin'] != 4 else ops['w'][:, :, :3]
        assert all((np.diff(w, axis=a) != 0).all() for a in range(3) if w.shape[a] > 1), name
        ref = gpu_cases.reference(sp, ops)
        assert np.abs(ref).max() < 65504 and (ref < 0).mean() > 0.2 and (ref > 0).mean() > 0.2, name
        n += 1
    assert n >= 30


def _rows_packing(d, blobs):
    return d['cin'] == 16 and d['cout'] == 16 and blobs[d['w_blob']][0] == 6 * 64 * 8 * 2


def product_regimes(calls):
    """Regime keys of the rtm3d_op_conv launches of a recorded call log that run on kernel 3."""
    tensors, blobs, keys = [], [], {}
    for fn, args in calls:
        if fn == 'rtm3d_tensor_create':
            tensors.append(args)
        if fn == 'rtm3d_blob_create':
            blobs.append(args)
        if fn != 'rtm3d_op_conv' or args[0]['kernel'] != _lib.CONV_SMALLC:
            continue
        d = args[0]
        s, B = d['in_stride'], tensors[d['in_tensor']][0]
        r = sr.launch(B, (d['Hm'] - 1) * s + 1, (d['Wm'] - 1) * s + 1, d['cin'], d['cout'], d['ntaps'], s, d['out_scale'], _rows_packing(d, blobs))
        keys.setdefault(sr.regime_key(r, d['relu']), (B, d['Hm'], d['Wm'], d['cin'], d['cout'], d['ntaps']))
    return keys


def test_every_product_regime_has_a_gpu_case(monkeypatch):
    sds = {bb: weights.synth_state_dict(bb, 3, 'trained') for bb in ('DLA-34', 'RESNET-18', 'RESNET-34')}
    # (build, switches): the ResNet stems; the DLA stem and level-2 entry with their fusions off, and on a map the level entry's
    # fused kernel does not admit (W % 128 != 0)
    off = {'FUSE_STEM': False, 'FUSE_LEVEL_ENTRY': False}
    plans = [('RESNET-18', 1, 384, 1280, {}), ('RESNET-18', 32, 416, 1280, {}), ('RESNET-34', 8, 384, 1280, {}),
             ('DLA-34', 1, 384, 1280, off), ('DLA-34', 2, 416, 1280, off), ('DLA-34', 32, 384, 1280, off), ('DLA-34', 1, 384, 1312, {})]
    covered = {gpu_cases.regime(sp) for sp in gpu_cases.CASES.values()}
    seen, missing = set(), {}
    for bb, B, H, W, switches in plans:
        pin_switches(monkeypatch, **switches)
        for key, where in product_regimes(record(plan_mod.build_plan(sds[bb], bb, B, H, W)).calls).items():
            seen.add(key)
            if key not in covered:
                missing[key] = (bb,) + where
    assert not missing, missing
    # the plans reach every instance but the two no product layer has (4 -> 16 and 16 -> 16 off the vertical walk)
    assert {k[0] for k in seen} == set(sr.INSTANCES) - {T4_16, T16_16}, {k[0] for k in seen}


def _record(P):
    """(rtm3d_op_conv descriptors, blob entries) of a plan's recorded call log."""
    calls = record(P).calls
    return [a[0] for fn, a in calls if fn == 'rtm3d_op_conv'], [a for fn, a in calls if fn == 'rtm3d_blob_create']


@pytest.mark.parametrize('dil,stride,rows', [(1, 1, True), (2, 1, False), (1, 2, False)])
def test_only_the_plain_3x3_takes_the_row_packing(dil, stride, rows):
    """A 16 -> 16 conv is packed by filter rows (6 K-steps, the vertical-walk kernel) only with the plain dilation-1 taps at
    stride 1: a dilated one keeps the per-tap packing of the per-tile kernel, which indexes every tap."""
    P = plan_mod.Plan(1, 32, 32)
    x, y = P.tensor(32, 32, 16, 2), P.tensor(32 // stride, 32 // stride, 16, 1)
    P.conv(x, y, np.ones((16, 16, 3, 3), np.float32), np.zeros(16, np.float32), stride=stride, dil=dil, name='c')
    (d,), blobs = _record(P)
    assert d['kernel'] == _lib.CONV_SMALLC and _rows_packing(d, blobs) == rows
    assert blobs[d['w_blob']][0] == (6 if rows else 5) * 64 * 8 * 2
    assert (d['tap_dy'][0][0], d['tap_dx'][0][8]) == (-dil, dil)


def test_gpu_cases_record_the_instance_the_mirror_names():
    """Each GPU case, recorded without a device: one kernel-3 descriptor per op, with the weight packing (5 or 6 K-steps for
    16 -> 16) that makes launch_conv_smallc pick the instance the case declares; likewise the every-pair chain as one plan."""
    def matches(d, blobs, sp):
        inst = gpu_cases.mirror(sp)['instance']
        assert d['kernel'] == _lib.CONV_SMALLC and (d['cin'], d['cout'], d['ntaps'], d['in_stride'], d['out_scale']) == (
            sp['cin'], sp['cout'], len(sp['taps']), sp['stride'], 1)
        assert blobs[d['w_blob']][0] == (sp['cout'] // 16) * sr.ksteps(inst) * 64 * 8 * 2 and _rows_packing(d, blobs) == (inst == R16_16)
        assert (d['in_coff'][0], d['out_coff'][0], bool(d['relu'])) == (sp['in_lo'], sp['out_lo'], sp['relu'])
        assert [(d['tap_dy'][0][t], d['tap_dx'][0][t]) for t in range(d['ntaps'])] == sp['taps']

    for name, sp in gpu_cases.CASES.items():
        P = plan_mod.Plan(sp['B'], sp['H'], sp['W'])
        gpu_cases.SmallC(P, sp, gpu_cases.case_seed(name))
        (d,), blobs = _record(P)
        matches(d, blobs, sp)
    keys = list(gpu_cases.CHAIN)
    order = gpu_cases.every_pair_order(len(keys))
    P = plan_mod.Plan(2, 64, 64)
    for i in order:
        gpu_cases.SmallC(P, gpu_cases.CHAIN[keys[i]], gpu_cases.case_seed(keys[i]))
    ds, blobs = _record(P)
    assert len(ds) == len(order) == 57
    for d, i in zip(ds, order):
        matches(d, blobs, gpu_cases.CHAIN[keys[i]])
