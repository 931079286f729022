"""Host mirror of what the launch code decides for the MXFP8 head ops (rtm3d_op_conv_mx8 / rtm3d_op_quant_mx8 in runtime.hip,
launch_conv_mx8 / launch_quant_mx8 and the kernels' index arithmetic in conv_mx8.hip), and the case table of the GPU suite
(tests/test_gpu_mx8_regimes.py), so that tests/test_mx8_regimes.py can read it without a GPU.

conv_mx8: one workgroup per (256-pixel tile, 256-channel tile) of a group, grid (MT * NT, groups); workgroup b takes item
xcd_contiguous_index(b, MT * NT), pixel tile item / NT, channel tile item % NT.  A K-step is (tap, 64-channel chunk): k = tap * cpt
+ chunk.  The rows of a partial last pixel tile past M re-read pixel M - 1 and store nothing; its second pixel half (waves with
wp == 1, rows 128-255) is dead altogether when it holds at most 128 pixels.
quant_mx8: one thread per (pixel, 32-channel block), 256 threads a workgroup."""
TILE = 256


def cdiv(a, b):
    return -(-a // b)


def xcd_contiguous_index(b, n):
    q, r, xcd, k = n >> 3, n & 7, b & 7, b >> 3
    return xcd * q + (xcd if xcd < r else r) + k


def conv(B, H, W, cin, cout, groups, ntaps):
    assert cin % 64 == 0 and cout % 256 == 0 and 1 <= groups <= 4 and 1 <= ntaps <= 80
    M, HW = B * H * W, H * W
    MT, NT, cpt = cdiv(M, TILE), cout // 256, cin // 64
    last_rows = M - (MT - 1) * TILE
    spans = [(t * TILE // HW, (min(M, (t + 1) * TILE) - 1) // HW) for t in range(MT)]
    n = MT * NT

    def item(b):
        i = xcd_contiguous_index(b, n)
        return i // NT, i % NT                          # (pixel tile, channel tile)
    return {'M': M, 'MT': MT, 'NT': NT, 'cpt': cpt, 'ksteps': ntaps * cpt, 'grid': (n, groups), 'last_rows': last_rows,
            'second_half_dead': last_rows <= 128, 'tile_straddles': any(a != b for a, b in spans),
            'partial_straddles': last_rows < TILE and spans[-1][0] != spans[-1][1], 'mod8': n % 8, 'item': item}


def quant(B, H, W, channels):
    assert channels % 32 == 0 and channels > 0
    nblk = channels // 32
    threads = B * H * W * nblk
    return {'nblk': nblk, 'threads': threads, 'grid': cdiv(threads, 256), 'last_partial': threads % 256 != 0}


# ------------------------------------------------------------------------------ tap sets
def taps3x3(dil):
    return [(ky * dil - dil, kx * dil - dil) for ky in range(3) for kx in range(3)]


TAPS = {
    'one': [(0, 0)],
    'two': [(0, 0), (1, 1)],
    'd1': taps3x3(1), 'd2': taps3x3(2), 'd6': taps3x3(6),
    'row': [(0, -1), (0, 0), (0, 1)],                               # 1 x 3
    'col': [(-1, 0), (0, 0), (1, 0)],                               # 3 x 1
    'neg': [(-1, -1), (-2, -1), (-1, -3)],                          # negative offsets only
    'corner': [(-5, 5), (0, 0), (1, 0)],                            # the border's corner, far beyond what the others need
    't80': [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5)][:80],   # the table's limit
}


def reach(taps):
    return max(max(abs(dy), abs(dx)) for dy, dx in taps)


# ------------------------------------------------------------------------------ GPU cases
# Exact data (tests/mx8_ref.py): spread / density chosen so that the L1 bound holds (tests/test_mx8_regimes.py checks it on the
# host); sx / sw shift the whole input / weight tensor by a power of two, the output scale bytes move by sx + sw.
def _c(name, B, H, W, cin, cout, taps, in_P, out, out_P, relu, in_coff=(0,), out_coff=(0,), in_C=None, out_C=None, spread=2,
       density=1.0, sx=0, sw=0, zero_block=False):
    G = len(in_coff)
    assert len(out_coff) == G
    return {'name': name, 'B': B, 'H': H, 'W': W, 'cin': cin, 'cout': cout, 'groups': G, 'taps': taps, 'in_P': in_P, 'out': out,
            'out_P': out_P, 'relu': relu, 'in_coff': list(in_coff), 'out_coff': list(out_coff),
            'in_C': in_C if in_C is not None else max(in_coff) + cin, 'out_C': out_C if out_C is not None else max(out_coff) + cout,
            'spread': spread, 'density': density, 'sx': sx, 'sw': sw, 'zero_block': zero_block}


CONV_CASES = [
    # T = 1 (no prefetch), M = 1, H = W = 1, one workgroup, no border on either side
    _c('t1_m1', 1, 1, 1, 64, 256, 'one', 0, 'mx8', 0, False),
    # T = 2 from one tap x two chunks; W = 1, M < 128: the second pixel half is dead; output border 3
    _c('t2_cpt2_m100', 1, 100, 1, 128, 256, 'one', 0, 'f16', 3, True, in_coff=(0, 128), out_coff=(0, 256), sx=-4),
    # T = 2 from two taps x one chunk
    _c('t2_two_taps', 1, 3, 5, 64, 256, 'two', 1, 'mx8', 1, True),
    # 3 taps x 2 chunks (ntaps != cpt: the tap / chunk split), M = 255, NT = 2, an MX8 slice at 32 of 576 channels
    _c('t6_row_m255', 1, 15, 17, 128, 512, 'row', 1, 'mx8', 1, True, out_coff=(32,), out_C=576),
    # odd T = 3, M = 256 exactly, 3 groups, fp16 slices from channel 8 (a multiple of 8, not of 32) of 812 (a pixel stride that is
    # a multiple of 8 bytes only: what the epilogue's 8-byte stores need and no more)
    _c('t3_col_m256', 1, 16, 16, 64, 256, 'col', 1, 'f16', 1, False, in_coff=(0, 64, 128), out_coff=(8, 264, 520), out_C=812, sx=-4),
    # odd T = 9, dilation 2, H = 1, M = 257: one live row in the last tile; NT = 4, 8 workgroups
    _c('t9_d2_m257', 1, 1, 257, 64, 1024, 'd2', 2, 'mx8', 1, False),
    # B = 3 with 130-pixel images: the full tile and the partial one (134 rows) each cross an image boundary; cpt = 4, 4 groups in
    # descending order, two of them on the same slice of a 384-channel input; 4 workgroups per group
    _c('b3_straddle_g4', 3, 10, 13, 256, 512, 'd1', 1, 'f16', 1, True, in_coff=(128, 128, 64, 0), out_coff=(1536, 1024, 512, 0),
       in_C=384, sx=-6),
    # cpt = 8, dilation 6, 3 pixel tiles x 3 channel tiles = 9 workgroups; enough blocks for every epilogue class
    _c('d6_cpt8_m600', 2, 12, 25, 512, 768, 'd6', 6, 'mx8', 1, True, spread=1),
    # 80 taps; the whole tensors shifted up: output scale bytes around 127 + 60
    _c('t80_scale_hi', 1, 6, 7, 64, 256, 't80', 4, 'mx8', 1, False, spread=1, sx=25, sw=26),
    # the border's corner through a border of 5; 2 groups
    _c('corner_p5', 2, 5, 9, 64, 256, 'corner', 5, 'f16', 0, False, in_coff=(64, 0), out_coff=(0, 256), sx=-2),
    # negative offsets only; the whole tensors shifted down: output scale bytes around 127 - 60
    _c('neg_scale_lo', 2, 8, 5, 128, 256, 'neg', 3, 'mx8', 3, True, sx=-34, sw=-35),
    # a border of 7 around taps that reach 1; an output block that ReLU zeroes
    _c('d1_p7_zero_block', 1, 8, 8, 256, 256, 'd1', 7, 'mx8', 1, True, zero_block=True),
]

QUANT_CASES = [
    # name, B, H, W, in_C, in_coff, channels, in_P, out_C, out_coff, out_P, first value class
    ('c8_of_72', 1, 5, 7, 72, 8, 64, 0, 96, 32, 0, 0),                # in_C a multiple of 8 only; 70 threads
    ('c24_nblk1', 2, 16, 16, 96, 24, 32, 2, 32, 0, 6, 0),             # nblk = 1; 512 threads, no partial workgroup
    ('c40_b3_1x1', 3, 1, 1, 104, 40, 64, 2, 64, 0, 0, 11),            # B = 3, H = W = 1: 6 threads (the NaN classes first)
    ('c0_aligned', 1, 4, 8, 64, 0, 64, 1, 128, 64, 6, 6),             # block-aligned, the product's form
]


def conv_case_values(c):
    """Every regime value a conv case runs, as (dimension, value) pairs."""
    r = conv(c['B'], c['H'], c['W'], c['cin'], c['cout'], c['groups'], len(TAPS[c['taps']]))
    T = r['ksteps']
    vals = {('T', T if T in (1, 2, 80) else 'odd' if T % 2 else 'even'), ('cpt', r['cpt']), ('taps', c['taps']),
            ('split', 'ntaps>1,cpt>1,ntaps!=cpt' if len(TAPS[c['taps']]) > 1 and r['cpt'] > 1 and len(TAPS[c['taps']]) != r['cpt'] else 'plain'),
            ('border', 'reach' if c['in_P'] == reach(TAPS[c['taps']]) else 'larger'),
            ('M', r['M'] if r['M'] in (1, 255, 256, 257) else '<128' if r['M'] < 128 else 'other'),
            ('last_tile', 'full' if r['last_rows'] == TILE else 'half_dead' if r['second_half_dead'] else 'both_halves'),
            ('straddle', r['tile_straddles']), ('partial_straddle', r['partial_straddles']),
            ('W1', c['W'] == 1), ('H1', c['H'] == 1),
            ('grid', 1 if r['grid'][0] == 1 else '%8==0' if r['mod8'] == 0 else ('<8' if r['grid'][0] < 8 else '>8') + ',%%8==%d' % r['mod8']),
            ('NT', r['NT']), ('groups', c['groups']),
            ('in_slice', 'whole' if c['in_C'] == c['groups'] * c['cin'] and sorted(c['in_coff']) == [g * c['cin'] for g in range(c['groups'])]
             else 'offset_in_wider'),
            ('in_shared', len(set(c['in_coff'])) < c['groups']),
            ('descending', c['groups'] > 1 and all(a > b for a, b in zip(c['out_coff'], c['out_coff'][1:]))),
            ('out_slice', 'whole' if c['out_C'] == c['groups'] * c['cout'] else 'offset_in_wider' if min(c['out_coff']) else 'wider'),
            ('out_align', (c['out'], 'odd' if min(c['out_coff']) % (32 if c['out'] == 'f16' else 256) else 'aligned')),
            ('out_P', c['out_P']), ('epilogue', (c['out'], c['relu'])),
            ('shift', 'hi' if c['sx'] + c['sw'] >= 45 else 'lo' if c['sx'] + c['sw'] <= -45 else 'mid'),
            ('zero_block', c['zero_block'])}
    return vals


# what the issue lists: every (dimension, value) here must be run by some conv case
CONV_REQUIRED = (
    [('T', v) for v in (1, 2, 'odd', 80)] + [('cpt', v) for v in (1, 2, 4, 8)] + [('split', 'ntaps>1,cpt>1,ntaps!=cpt')]
    + [('taps', v) for v in ('one', 'd1', 'd2', 'd6', 'row', 'col', 'neg', 'corner')] + [('border', 'larger')]
    + [('M', v) for v in (1, '<128', 255, 256, 257)] + [('last_tile', 'half_dead'), ('last_tile', 'full'), ('straddle', True), ('partial_straddle', True), ('W1', True), ('H1', True)]
    + [('grid', 1), ('grid', '<8,%8==2'), ('grid', '<8,%8==4'), ('grid', '>8,%8==1'), ('grid', '%8==0')]
    + [('NT', v) for v in (1, 2, 4)] + [('groups', v) for v in (1, 2, 3, 4)]
    + [('in_slice', 'offset_in_wider'), ('in_shared', True), ('descending', True), ('out_slice', 'offset_in_wider'),
       ('out_align', ('f16', 'odd')), ('out_align', ('mx8', 'odd'))]
    + [('out_P', v) for v in (0, 1, 3)] + [('epilogue', (o, r)) for o in ('f16', 'mx8') for r in (False, True)]
    + [('shift', 'hi'), ('shift', 'lo'), ('zero_block', True)])


def quant_case_values(q):
    name, B, H, W, in_C, in_coff, channels, in_P, out_C, out_coff, out_P, _ = q
    r = quant(B, H, W, channels)
    return {('in_coff', in_coff), ('in_coff%32', in_coff % 32), ('in_C%32', in_C % 32 != 0), ('nblk1', r['nblk'] == 1),
            ('last_partial', r['last_partial']), ('b3_1x1', (B, H, W) == (3, 1, 1)), ('in_P', in_P), ('out_P', out_P),
            ('in_border', in_P > 0), ('out_slice', 'whole' if channels == out_C else 'offset' if out_coff else 'wider')}


QUANT_REQUIRED = ([('in_coff', v) for v in (8, 24, 40)] + [('in_C%32', True), ('nblk1', True), ('last_partial', True), ('last_partial', False),
                                                             ('b3_1x1', True), ('in_P', 0), ('in_P', 2), ('out_P', 0), ('out_P', 6)])


# ------------------------------------------------------------------------------ the product plans' ops
# The dimensions a head op of build_plan(head_precision='mxfp8') is placed in; the M-dependent ones by class, since the kernel
# treats every full tile alike.
PLAN_CONV_DIMS = ('cpt', 'taps', 'border', 'last_tile', 'NT', 'groups', 'in_slice', 'in_shared', 'out_slice', 'epilogue')
PLAN_QUANT_DIMS = ('in_coff%32', 'in_C%32', 'nblk1', 'in_border', 'out_P')


def plan_conv_values(P, op):
    """The (dimension, value) pairs of a conv_mx8 op of plan P, over PLAN_CONV_DIMS."""
    names = {tuple(v): k for k, v in TAPS.items()}
    tin, tout = P.tensors[op['inp'][0].tid], P.tensors[op['out'][0].tid]
    c = _c(op['name'], P.B, op['Hm'], op['Wm'], op['cin'], op['cout'], names[tuple(op['taps'])], tin['pad'],
           'f16' if op['out_fp16'] else 'mx8', tout['pad'], bool(op['relu']), in_coff=[s.coff for s in op['inp']],
           out_coff=[s.coff for s in op['out']], in_C=tin['C'], out_C=tout['C'])
    return {(d, v) for d, v in conv_case_values(c) if d in PLAN_CONV_DIMS}


def plan_quant_values(P, op):
    tin, tout = P.tensors[op['inp'].tid], P.tensors[op['out'].tid]
    q = (op['name'], P.B, tin['H'], tin['W'], tin['C'], op['inp'].coff, op['inp'].C, tin['pad'], tout['C'], op['out'].coff, tout['pad'], 0)
    return {(d, v) for d, v in quant_case_values(q) if d in PLAN_QUANT_DIMS}
