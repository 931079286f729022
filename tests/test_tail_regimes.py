"""The host mirror of the launch decisions of the forward path's tail (tests/tail_regimes.py: softmax fusion, logit convs,
k x k max-pool, peak patches), checked by hand-worked launches; the GPU cases of tests/test_gpu_tail.py against it; and a coverage
guard: every regime the product plans send to these kernels is one that some GPU case runs."""
import pytest

from rtm3d_amd import plan as plan_mod, weights
from tests import conv256_tiles as ct
from tests import tail_regimes as tr
from tests import test_gpu_tail as gpu_cases
from tests.abi_recorder import pin_switches, record


def test_softmax_fuse_by_hand():
    # 384 x 1280, B = 1: 96 x 320 map.  small: 1 * 48 < 512, one row per chunk, 96 chunks.  xsplit: 320 / 2 = 160 >= 64 -> 2,
    # 320 / 4 = 80 >= 64 -> 4; then 1 * 96 * 4 = 384 < 512 and 320 / 8 = 40 >= 32 -> 8.  seg_w = 40, 768 workgroups.
    r = tr.softmax_fuse(1, 96, 320, 3)
    assert (r['small'], r['rows_per_chunk'], r['chunks'], r['xsplit'], r['seg_w'], r['apply_chunks']) == (True, 1, 96, 8, 40, 768)
    assert r['reduce_grid'] == (96, 1, 3) and r['combine_grid'] == (1, 3, 4) and r['apply_grid'] == (768, 1, 1)
    assert r['seg_widths'] == [40] * 8 and r['parts_busy'] == 16 and not r['reduce_tail'] and r['apply_tail']
    # B = 2 is still small (96 < 512) but 2 * 96 * 4 = 768 >= 512: four segments of 80; B = 32: 32 * 48 = 1536 >= 512: two rows
    # per chunk, 48 chunks (52 at 416 rows)
    r = tr.softmax_fuse(2, 96, 320, 3)
    assert (r['rows_per_chunk'], r['xsplit'], r['seg_w'], r['apply_tail']) == (1, 4, 80, False) and tr.softmax_fuse(2, 104, 320, 3)['chunks'] == 104
    r = tr.softmax_fuse(32, 96, 320, 3)
    assert (r['small'], r['rows_per_chunk'], r['chunks'], r['xsplit'], r['reduce_grid']) == (False, 2, 48, 4, (48, 32, 3))
    assert tr.softmax_fuse(32, 104, 320, 3)['chunks'] == 52 and tr.softmax_fuse(32, 104, 320, 3)['apply_grid'] == (416, 32, 1)
    # the producers of the 96 x 320 map are transposed convs of the 48 x 160 map: 4 phases x 6 x 5 tiles x 2 runs = 240 per image
    assert tr.stat_chunks(4, 48, 160) == 240 and tr.stat_chunks(1, 8, 32) == 2
    r = tr.softmax_fuse(32, 96, 320, 3, partial_chunks=240)
    assert (r['reduce_runs'], r['reduce_grid'], r['combine_chunks'], r['parts_busy']) == (False, None, 240, 16)
    with pytest.raises(AssertionError):
        tr.stat_chunks(4, 52, 160)                  # 416 rows: 52 % 8 != 0, no halo route, no partials
    # the boundary of `small`: B * ceil(H / 2) against 512; an odd H leaves a one-row last chunk
    assert tr.softmax_fuse(51, 19, 40, 1)['small'] and not tr.softmax_fuse(52, 19, 40, 1)['small']
    assert tr.softmax_fuse(52, 19, 40, 1)['last_chunk_rows'] == 1 and tr.softmax_fuse(52, 20, 40, 1)['last_chunk_rows'] == 2
    # column segments: 258 pixels in 8 segments of ceil(33 / 8) * 8 = 40: six full, one of 18, one empty
    r = tr.softmax_fuse(1, 9, 258, 1)
    assert (r['xsplit'], r['seg_w'], r['seg_widths']) == (8, 40, [40] * 6 + [18, 0]) and r['apply_tail'] and r['reduce_tail']
    assert tr.softmax_fuse(2, 12, 20, 1)['seg_w'] == 24 and tr.softmax_fuse(1, 16, 72, 2)['seg_widths'] == [40, 32]


def test_headout_by_hand():
    # 96 x 320 map, four heads: B = 1: 1 * 6 * 10 * 4 = 240 < 1024: 8-row tiles, 12 x 10 of them; B = 32: 7680: 16-row tiles
    r = tr.headout(1, 96, 320, 4)
    assert (r['switch_count'], r['tile_rows'], r['tiles_y'], r['tiles_x'], r['grid'], r['last_rows'], r['last_cols']) == (240, 8, 12, 10, (120, 4), 8, 32)
    assert (r['halo_rows_past'], r['halo_cols_past']) == (0, 0)
    r = tr.headout(32, 96, 320, 4)
    assert (r['tile_rows'], r['tiles_y'], r['grid'], r['last_rows']) == (16, 6, (1920, 4), 16)
    # 104 rows: 7 tile rows of 16, the last one with 8 rows: its halo rows 95 .. 112, of which 105 .. 112 lie past row H + in_P - 1 = 104
    r = tr.headout(32, 104, 320, 4)
    assert (r['tile_rows'], r['tiles_y'], r['last_rows'], r['halo_rows_past'], r['grid']) == (16, 7, 8, 8, (2240, 4))
    # the sparse-heads plan records the heat map head alone: B = 32: 32 * 6 * 10 = 1920 >= 1024; B = 2: 120: 8-row tiles
    assert tr.headout(32, 96, 320, 1)['tile_rows'] == 16 and tr.headout(2, 96, 320, 1)['grid'] == (240, 1)
    # the switch sits at 4 * CUs = 1024 exactly
    assert tr.headout(64, 17, 33, 4)['switch_count'] == 1024 and tr.headout(64, 17, 33, 4)['tile_rows'] == 16
    assert tr.headout(85, 33, 5, 4)['switch_count'] == 1020 and tr.headout(85, 33, 5, 4)['tile_rows'] == 8
    # 17 x 33 in 16-row tiles: the second tile row holds one row, halo rows 15 .. 32, 18 .. 32 past row 17; same for columns
    r = tr.headout(64, 17, 33, 4)
    assert (r['last_rows'], r['last_cols'], r['halo_rows_past'], r['halo_cols_past']) == (1, 1, 15, 31)
    assert tr.headout(1, 13, 32, 2, in_P=1)['halo_rows_past'] == 3 and tr.headout(1, 13, 32, 2, in_P=6)['halo_rows_past'] == 0


def test_xcd_contiguous_index_is_a_permutation():
    for n in range(1, 4097):
        seen = bytearray(n)
        for b in range(n):
            t = tr.xcd_contiguous_index(b, n)
            assert 0 <= t < n and not seen[t], (n, b, t)
            seen[t] = 1
    # n = 10: XCDs 0 and 1 take two items, the others one: workgroups 0 .. 9 -> items 0, 2, 4, 5, 6, 7, 8, 9, 1, 3
    assert [tr.xcd_contiguous_index(b, 10) for b in range(10)] == [0, 2, 4, 5, 6, 7, 8, 9, 1, 3]


def test_maxpool_and_patches_by_hand():
    # DLA-34 level3 -> level4 pool at B = 1: 24 x 80 x 128 channels = 30720 threads = 120 full blocks
    assert tr.maxpool(1, 24, 80, 128) == {'threads': 30720, 'blocks': 120, 'idle': 0}
    assert tr.maxpool(1, 96, 320, 64)['idle'] == 0 and tr.maxpool(1, 5, 7, 8) == {'threads': 35, 'blocks': 1, 'idle': 221}
    # patch pixel (5 a + i, 5 b + j) holds z(py + i - 2 + 6 (a - 1), px + j - 2 + 6 (b - 1))
    assert tr.patch_cell(0, 0) == (-8, -8) and tr.patch_cell(7, 7) == (0, 0) and tr.patch_cell(14, 14) == (8, 8)
    assert tr.patch_cell(4, 5) == (-4, -2) and tr.patch_cell(10, 9) == (4, 2)
    assert sorted({tr.patch_cell(r, 0)[0] for r in range(15)}) == [-8, -7, -6, -5, -4, -2, -1, 0, 1, 2, 4, 5, 6, 7, 8]
    # a corner peak: the 5 x 5 window (origin 2) loses two rows and two columns: 25 - 9 = 16 positions; the 3 x 3 one 9 - 4 = 5
    assert len(tr.mask_zeroed(0, 0, 5, 2, 96, 320)) == 16 and len(tr.mask_zeroed(95, 319, 3, 1, 96, 320)) == 5
    assert tr.mask_zeroed(0, 0, 3, 1, 96, 320) == {(0, 0), (0, 1), (0, 2), (1, 0), (2, 0)}
    assert tr.mask_zeroed(1, 5, 5, 2, 96, 320) == {(0, j) for j in range(5)} and tr.mask_zeroed(2, 2, 5, 2, 96, 320) == set()
    assert tr.mask_zeroed(-1, -1, 5, 2, 96, 320) == set()
    with pytest.raises(ValueError):
        tr.regime_key('conv64_root')


def test_gpu_cases_match_the_mirror():
    """Every GPU case's declared regime is what the mirror says, and the table covers what the regimes hinge on."""
    for name, sp in list(gpu_cases.CASES.items()) + list(gpu_cases.CHAIN.items()):
        gpu_cases.check_regime(sp)
    cases = list(gpu_cases.CASES.values())
    fus = [(gpu_cases.mirror(sp), sp) for sp in cases if sp['kind'] == 'softmax_fuse']
    assert {(sp['n_u'], r['reduce_runs']) for r, sp in fus} == {(n, w) for n in (1, 2, 3) for w in (True, False)}
    own = [(r, sp) for r, sp in fus if r['reduce_runs']]
    assert any(r['rows_per_chunk'] == 1 and sp['H'] % 2 for r, sp in own) and any(r['rows_per_chunk'] == 2 and r['last_chunk_rows'] == 1 for r, sp in own)
    for rs in (own, [(r, sp) for r, sp in fus if not r['reduce_runs']]):
        n = {r['combine_chunks'] for r, _ in rs}
        assert any(c < 16 for c in n) and 16 in n and any(c > 16 and c % 16 for c in n) and any(c > 16 and c % 16 == 0 for c in n), n
    assert {48, 104, 240} & {r['combine_chunks'] for r, _ in fus} >= {104, 240}
    assert {r['xsplit'] for r, _ in fus} == {1, 2, 4, 8}
    assert any(r['last_seg_w'] == 0 for r, _ in fus) and any(0 < r['last_seg_w'] < r['seg_w'] for r, _ in fus)
    assert any(sp['W'] % 8 for _, sp in fus) and any(sp['W'] % 16 in range(1, 9) for _, sp in fus) and any(sp['W'] < 32 for _, sp in fus)
    assert any(r['reduce_tail'] for r, _ in own) and any(r['apply_tail'] for r, _ in fus)
    assert any(len(set(sp['u_pads'])) > 1 for _, sp in fus) and {(sp['zi_pad'], sp['zo_pad']) for _, sp in fus} >= {(0, 6), (6, 0), (1, 2)}
    prods = [sp for _, sp in fus if sp['producer']]
    assert {(gpu_cases.producer_domain(sp)[3], gpu_cases.producer_tiles(sp)['one_list']) for sp in prods} == {(t, o) for t in (4, 9) for o in (True, False)}
    assert any(sp['B'] > 1 and not gpu_cases.producer_tiles(sp)['one_list'] for sp in prods) and any(sp['replay'] for sp in prods)
    heads = [(gpu_cases.mirror(sp), sp) for sp in cases if sp['kind'] == 'headout']
    exact = [(r, sp) for r, sp in heads if sp['exact']]
    assert {(r['tile_rows'], sp['nheads']) for r, sp in exact} == {(t, n) for t in (8, 16) for n in (1, 2, 3, 4)}
    assert {r['grid'][0] % 8 for r, _ in exact} == set(range(8))
    for pos in range(4):
        assert {sp['couts'][pos] for _, sp in exact if sp['nheads'] > pos} >= {1, 16}, pos
    assert {r['switch_count'] for r, _ in exact} >= {1024} and any(1020 <= r['switch_count'] < 1024 for r, _ in exact)
    assert any(r['tile_rows'] == 16 and r['halo_rows_past'] >= 2 for r, _ in exact) and any(r['tile_rows'] == 16 and r['halo_cols_past'] >= 2 for r, _ in exact)
    assert any(r['tile_rows'] == 8 and r['halo_rows_past'] for r, _ in exact) and {sp['in_P'] for _, sp in exact} >= {1, 2, 6}
    assert {r['tile_rows'] for r, sp in heads if not sp['exact']} == {8, 16}
    pools = [(gpu_cases.mirror(sp), sp) for sp in cases if sp['kind'] == 'maxpool']
    assert {(sp['k'], sp['stride'], sp['pad'], bool(r['idle'])) for r, sp in pools} == {(2, 2, 0, False), (2, 2, 0, True), (3, 2, 1, False), (3, 2, 1, True)}
    assert any(sp['negative'] and sp['pad'] for _, sp in pools) and any(sp['in_lo'] and sp['in_hi'] and sp['o_lo'] and sp['o_hi'] for _, sp in pools)
    chain = {k for sp in gpu_cases.CHAIN.values() for k in gpu_cases.regimes(sp)}
    assert {k[:3] for k in chain if k[0] == 'softmax_fuse'} >= {('softmax_fuse', 2, 'reduce'), ('softmax_fuse', 1, 'partials'), ('softmax_fuse', 2, 'partials')}
    assert {k[0] for k in chain} == {'softmax_fuse', 'stat_producer', 'headout', 'maxpool'}


def product_regimes(calls, cus=256):
    """Regime keys of the tail launches of a recorded call log."""
    tensors, keys, stat = [], {}, {}
    for fn, a in calls:
        if fn == 'rtm3d_tensor_create':
            tensors.append(a)                           # [B, H, W, C, pad]
        elif fn == 'rtm3d_op_conv' and a[0]['softmax_stat_slot'] >= 0:
            d = a[0]
            B = tensors[d['in_tensor']][0]
            stat[d['out_tensor']] = tr.stat_chunks(d['groups'], d['Hm'], d['Wm'])
            one = ct.tiles('halo', B * d['Hm'] * d['Wm'], d['cout'], groups=d['groups'], cin=d['cin'], cus=cus)['one_list']
            keys.setdefault(tr.regime_key('stat_producer', ntaps=d['ntaps'], one_list=one), (B, d['Hm'], d['Wm']))
        elif fn == 'rtm3d_op_softmax_fuse':
            B, H, W = tensors[a[0]][:3]
            us = list(a[3])[:a[2]]
            chunks = {stat.pop(u, 0) for u in us}
            assert len(chunks) == 1, 'the operands of one fusion all have producers with partials, or none has'
            keys.setdefault(tr.regime_key('softmax_fuse', B=B, H=H, W=W, n_u=a[2], partial_chunks=chunks.pop(), cus=cus), (B, H, W))
        elif fn == 'rtm3d_op_headout':
            B, H, W, _, P = tensors[a[0]]
            keys.setdefault(tr.regime_key('headout', B=B, H=H, W=W, nheads=a[3], couts=list(a[4])[:a[3]], in_P=P, cus=cus), (B, H, W))
        elif fn == 'rtm3d_op_maxpool':
            B, Ho, Wo = tensors[a[2]][:3]
            keys.setdefault(tr.regime_key('maxpool', k=a[5], stride=a[6], pad=a[7], B=B, Ho=Ho, Wo=Wo, C=a[4]), (B, Ho, Wo))
        elif fn == 'rtm3d_op_patch_mask':
            keys.setdefault(tr.regime_key('patch_mask', S=tensors[a[0]][1], origin=a[4]), tuple(tensors[a[0]]))
    return keys


# what the GPU file runs besides CASES: the mask op of the two window sizes (test_peak_patch_mask)
MASK_CASES = {tr.regime_key('patch_mask', S=5, origin=2), tr.regime_key('patch_mask', S=3, origin=1)}


def test_every_product_regime_has_a_gpu_case(monkeypatch):
    pin_switches(monkeypatch)
    covered = {k for sp in gpu_cases.CASES.values() for k in gpu_cases.regimes(sp)} | MASK_CASES
    seen, missing, by_plan = set(), {}, {}
    for bb in ('DLA-34', 'RESNET-18'):
        sd = weights.synth_state_dict(bb, 3, 'trained')
        plans = [((bb, B, H, dh), (lambda B=B, H=H, dh=dh: plan_mod.build_plan(sd, bb, B, H, 1280, dense_heads=dh)))
                 for B in (1, 2, 32) for H in (384, 416) for dh in (None, 1)]
        if bb == 'DLA-34':
            plans += [((bb, 'peaks', B), (lambda B=B: plan_mod.build_peak_plan(sd, B * 100, (96, 320)))) for B in (1, 32)]
        for tag, build in plans:
            by_plan[tag] = product_regimes(record(build()).calls)
            for key, where in by_plan[tag].items():
                seen.add(key)
                if key not in covered:
                    missing[key] = (tag, where)
    assert not missing, missing
    # what the plans are known to reach: a change of routing shows here
    assert {k[0] for k in seen} == {'softmax_fuse', 'stat_producer', 'headout', 'maxpool', 'patch_mask'}, seen
    for (bb, B, H, dh), keys in ((t, k) for t, k in by_plan.items() if t[1] != 'peaks'):
        fus = [k for k in keys if k[0] == 'softmax_fuse']
        assert len(fus) == 1 and fus[0][1] == 3 and fus[0][6:] == (8 if B == 1 else 4, 'full', False), (bb, B, H, fus)
        # 384 rows: the transposed convs of the 48 x 160 map take the halo route and write the partials (from B = 2 on: at B = 1
        # they are too small for the 256 x 256 kernels); 416 rows: 52 % 8 != 0, the fusion reduces for itself
        assert fus[0][2] == ('partials' if H == 384 and B >= 2 else 'reduce'), (bb, B, H, fus)
        assert fus[0][3] == (None if fus[0][2] == 'partials' else 2 if B == 32 else 1), (bb, B, H, fus)
        assert [k[1:] for k in keys if k[0] == 'stat_producer'] == ([(4, B == 2)] if fus[0][2] == 'partials' else []), (bb, B, H, keys)
        ho = [k for k in keys if k[0] == 'headout']
        assert len(ho) == 1 and ho[0][1:4] == (16 if B == 32 else 8, 1 if dh else 4, (3,) if dh else (3, 16, 2, 2)), (bb, B, H, dh, ho)
        assert ho[0][4:] == (B == 32 and H == 416, False), (bb, B, H, ho)
    assert {k[1:4] for k in seen if k[0] == 'maxpool'} == {(2, 2, 0), (3, 2, 1)} and not any(k[4] for k in seen if k[0] == 'maxpool')
    assert {k for k in seen if k[0] == 'patch_mask'} == MASK_CASES
