"""CPU: the host helpers of "drawing tracks" (the font, the label text) against the numpy yardstick tests/draw_tracks_ref.py,
the yardstick against closed forms, and the conditions of the case tables (tests/draw_tracks_cases.py) that make the device
comparison of tests/test_gpu_draw_tracks.py a comparison of bytes.  No GPU: rtm3d_draw_font_rows, rtm3d_draw_label_text and
rtm3d_draw_tracks_default_params are host functions."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import draw_ref
from tests import draw_cases as dc
from tests import draw_tracks_ref as ref
from tests import draw_tracks_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def c_params(lib, names=tc.NAMES, fields=15, ncls=3):
    q = _lib.DrawTracksParamsC()
    assert lib.rtm3d_draw_tracks_default_params(ctypes.byref(q)) == 0
    q.label_fields, q.base.ncls = fields, ncls
    for i in range(16):
        q.names[i].value = names[i][:7] if i < len(names) else b''
    return q


# ---------------------------------------------------------------- the font

def test_font_rows_equal_the_art_for_every_character(lib):
    for ch in ref.CHARS:
        rows = (ctypes.c_uint8 * 7)()
        assert lib.rtm3d_draw_font_rows(ord(ch), ctypes.byref(rows)) == 0, ch
        assert list(rows) == ref.font_rows(ch), ch


def test_font_refuses_every_byte_outside_the_set(lib):
    for byte in range(-2, 258):
        if 0 <= byte < 256 and chr(byte) in ref.CHARS:
            continue
        rows = (ctypes.c_uint8 * 7)(*[0xEE] * 7)
        assert lib.rtm3d_draw_font_rows(byte, ctypes.byref(rows)) != 0, byte
        assert list(rows) == [0xEE] * 7


def test_glyphs_are_distinct_non_empty_and_fit_5_by_7():
    assert len(ref.CHARS) == 44 and len(set(ref.CHARS)) == 44
    seen = {}
    for ch in ref.CHARS:
        rows = ref.font_rows(ch)
        assert len(rows) == 7 and all(0 <= r < 32 for r in rows), ch
        assert any(rows) == (ch != ' '), ch
        assert tuple(rows) not in seen, (ch, seen.get(tuple(rows)))
        seen[tuple(rows)] = ch


def test_default_params_and_struct_size(lib):
    q = _lib.DrawTracksParamsC()
    assert lib.rtm3d_draw_tracks_default_params(ctypes.byref(q)) == 0
    assert (q.base.layers, q.npal, q.label_fields, q.font_scale, q.bev_fade, q.vel_horizon) == (15, 32, 3, 1, 256, 1.0)
    assert [q.names[i].value for i in (0, 9, 10, 15)] == [b'C0', b'C9', b'C10', b'C15']
    assert len({tuple(q.palette[i]) for i in range(32)}) == 32
    assert lib.rtm3d_draw_tracks_default_params(None) != 0
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s/include/rtm3d_hip.h"\nint main(void){printf("%%zu %%zu %%zu", '
           'sizeof(rtm3d_draw_tracks_params), offsetof(rtm3d_draw_tracks_params, names), offsetof(rtm3d_draw_tracks_params, vel_horizon));return 0;}' % REPO)
    os.makedirs(os.path.join(REPO, 'tests', '_build'), exist_ok=True)
    exe = os.path.join(REPO, 'tests', '_build', 'sizeof_draw_tracks')
    subprocess.run(['gcc', '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    P = _lib.DrawTracksParamsC
    assert [int(v) for v in subprocess.check_output([exe]).split()] == [ctypes.sizeof(P), P.names.offset, P.vel_horizon.offset]


# ---------------------------------------------------------------- the label text

IDS = (0, 1, 42, 9999999, 10000000, 10000001, -1, -7654321, -20000005, 2 ** 31 - 1, -2 ** 31)
SCORES = (0.0, 0.05, 0.5, 0.999999, 1.0, 7.0, -0.3, float('nan'))
ZS = (-3.0, 0.0, 0.04, 0.1, 9.96, 45.67, 999.94, 1234.5, float('nan'), float('inf'))


def test_label_text_equals_the_yardstick(lib):
    n = 0
    for fields in range(16):
        q = c_params(lib, fields=fields)
        for tid, cls, (score, z) in itertools.product(IDS, range(3), zip(SCORES + SCORES[:2], ZS)):
            out = (ctypes.c_char * 32)()
            assert lib.rtm3d_draw_label_text(ctypes.byref(q), tid, cls, score, z, out) == 0
            want = ref.label_text(fields, tid, tc.NAMES[cls], score, z)
            assert out.value.decode('latin-1') == want, (fields, tid, cls, score, z)
            assert len(want) <= 27 and all(c in ref.CHARS for c in want)
            n += 1
    assert n == 16 * len(IDS) * 3 * len(ZS)


def test_label_text_spot_values(lib):
    q = c_params(lib)
    out = (ctypes.c_char * 32)()

    def text(fields, tid, cls, score, z):
        q.label_fields = fields
        assert lib.rtm3d_draw_label_text(ctypes.byref(q), tid, cls, score, z, out) == 0
        return out.value.decode()

    assert text(15, 9999999, 1, 0.999999, 1234.5) == '#9999999 PEDESTR 99% 999.9M'           # the longest: 27 characters
    assert text(15, 10000000, 0, 1.0, 0.04) == '#0 CAR 99% 0.0M'
    assert text(15, -12, 2, 0.0, -1.0) == '?12 CY?L-ST 00% 0.0M'
    assert text(14, 5, 0, 0.5, 45.67) == 'CAR 50% 45.6M' and text(1, 0, 0, 0.5, 1.0) == '' and text(9, 0, 0, 0.5, 7.25) == '7.2M'
    assert text(0, 5, 0, 0.5, 1.0) == ''
    assert ref.label_text(15, 3, b'Car', 0.5, 7.25, kept=False) == '#3 CAR 50%'                   # no distance without a 3D box
    q.label_fields = 16
    assert lib.rtm3d_draw_label_text(ctypes.byref(q), 1, 0, 0.5, 1.0, out) != 0 and b'label_fields' in lib.rtm3d_last_error()
    q.label_fields = 15
    assert lib.rtm3d_draw_label_text(ctypes.byref(q), 1, 3, 0.5, 1.0, out) != 0 and b'class' in lib.rtm3d_last_error()
    assert lib.rtm3d_draw_label_text(None, 1, 0, 0.5, 1.0, out) != 0


# ---------------------------------------------------------------- the yardstick against closed forms

def test_a_scale_2_glyph_on_a_blank_image():
    img = np.zeros((20, 16, 3), np.uint8)
    n = ref.paint_glyph(img, '1', 3, 2, 2, (9, 8, 7))
    art = ['..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.']
    want = np.zeros((20, 16), bool)
    for r, row in enumerate(art):
        for c, bit in enumerate(row):
            if bit == '#':
                want[2 + 2 * r:4 + 2 * r, 3 + 2 * c:5 + 2 * c] = True
    assert n == 4 * 10 and np.array_equal(img.any(2), want) and (img[want] == (9, 8, 7)).all()


def test_ink_is_black_from_128000_on():
    assert 299 * 128 + 587 * 128 + 114 * 128 == 128000
    assert ref.ink((128, 128, 128)) == (0, 0, 0) and ref.ink((128, 128, 127)) == (255, 255, 255)        # 128000 and 127886
    assert ref.ink((255, 87, 6)) == (255, 255, 255) and ref.ink((255, 87, 7)) == (0, 0, 0)              # 127998 and 128112
    img = np.zeros((12, 12, 3), np.uint8)
    ref.paint_label(img, '1', 0, 0, 1, (128, 128, 127))
    assert tuple(img[1, 3]) == (255, 255, 255) and tuple(img[0, 0]) == (128, 128, 127)                    # glyph pixel, background pixel


def test_label_above_the_box_or_inside_it():
    s, n = 2, 3
    hl = 9 * s
    assert ref.label_box(5, 0, n, s) == (5, 0, 5 + (6 * n + 1) * s - 1, hl - 1)                   # y1 = 0: inside
    assert ref.label_box(5, hl - 1, n, s) == (5, hl - 1, 5 + (6 * n + 1) * s - 1, 2 * hl - 2)     # one row short: inside
    assert ref.label_box(5, hl, n, s) == (5, 0, 5 + (6 * n + 1) * s - 1, hl - 1)                  # y1 = label height: above, top row 0
    assert ref.label_box(5, -4, n, s)[1] == -4
    img = np.zeros((40, 50, 3), np.uint8)
    bg, gl = ref.paint_label(img, 'A1', 4, hl, s, (200, 0, 0))
    assert bg == 13 * s * hl and (img[:hl, 4:4 + 13 * s].any(2)).all() and not img[hl:].any() and not img[:, :4].any()
    assert gl == s * s * (sum(r.count('#') for r in ref.ART['A']) + sum(r.count('#') for r in ref.ART['1']))
    assert tuple(img[s, 4 + s + s]) == (255, 255, 255)                                            # 'A' row 0 column 1, white on dark red


@pytest.mark.parametrize('edge,x1,y1,s', [('left', -7, 20, 2), ('right', 40, 20, 2), ('top', 10, -5, 2), ('bottom', 10, 20, 3)])
def test_a_label_clipped_by_each_frame_edge(edge, x1, y1, s):
    text = '#12'                                             # (bottom: 27 rows do not fit above row 20, so inside: rows 20 .. 46 of 37)
    big = np.zeros((37 + 80, 53 + 80, 3), np.uint8)
    small = np.zeros((37, 53, 3), np.uint8)
    # the same label on a canvas with 40 pixels of room all round: the frame is its window
    # (placement is decided by y1 alone, so it is repeated by hand on the big canvas)
    bx0, by0, bx1, by1 = ref.label_box(x1, y1, len(text), s)
    ref.paint_rect(big, bx0 + 40, by0 + 40, bx1 + 40, by1 + 40, (10, 20, 200))
    ref.paint_text(big, text, bx0 + s + 40, by0 + s + 40, s, ref.ink((10, 20, 200)))
    bg, gl = ref.paint_label(small, text, x1, y1, s, (10, 20, 200))
    assert np.array_equal(small, big[40:77, 40:93])
    full = (6 * len(text) + 1) * s * 9 * s
    assert 0 < bg < full and gl > 0, (edge, bg, full)


def test_bad_extents_remove_one_primitive_only():
    img = np.zeros((10, 10, 3), np.uint8)
    assert ref.paint_rect(img, 0, 0, 8193, 5, (1, 1, 1)) == 0 and not img.any()
    wide = np.zeros((8, 8192, 3), np.uint8)
    assert ref.paint_glyph(wide, '8', 8188, 0, 1, (1, 1, 1)) == 17 - 4          # columns 8188 .. 8192: legal, the last one (4 pixels) off the frame
    assert ref.paint_glyph(wide, '8', 8189, 0, 1, (1, 1, 1)) == 0              # .. 8193: not drawn at all
    assert ref.paint_glyph(img, '8', 0, 0, 1, (1, 1, 1)) == 17


def test_id_colours():
    pal = tc.PALETTE3
    assert tuple(ref.id_colour(pal, 1, False)) == pal[0] and tuple(ref.id_colour(pal, 4, False)) == pal[0] and tuple(ref.id_colour(pal, 6, False)) == pal[2]
    assert tuple(ref.id_colour(pal, -2, True)) == (5, 10, 100) and tuple(ref.id_colour([(255, 1, 0)], -9, True)) == (128, 1, 0)


# ---------------------------------------------------------------- the case tables

CASES = tc.cases()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_case_conditions(case):
    p = case['params']
    if p['layers'] & ref.TRACK_BEV:
        # every fp64 coordinate that passes through device sin / cos lies at least MARGIN from an integer
        n = 0
        for table in case['state']:
            for sl in table[ref.HEADER:].reshape(-1, ref.SLOT):
                if ref.live(sl):
                    assert tc.track_margins_ok(sl, p['bev_hw'], p['bev_m_per_px'], p['vel_horizon']), case['name']
                    n += 1
        assert n >= 5
    if p['layers'] & ref.BEV:
        for b in range(case['rec'].shape[0]):
            for r in case['rec'][b]:
                if r[31] == 2:
                    assert dc.margins_ok(r, case['K'][b], p['bev_hw'], p['bev_m_per_px'])
    imgs, bev = tc.backgrounds(case)
    stats = ref.draw(imgs, case['rec'], case['ids'], case['K'], bev, case['state'], **p)
    for key in case['expect']:                           # nothing passes because it was skipped
        assert stats[key] > 0, (case['name'], key, stats)
    for key in set(stats) - set(case['expect']):
        assert stats[key] == 0, (case['name'], key, stats)


def test_case_specials():
    by = {c['name']: c for c in CASES}
    # two_rounds: slot 1 is the ninth painted slot of ten and its label has 26 characters: items 232 .. 260 hold it
    c = by['two_rounds']
    text = ref.label_text(15, c['ids'][0, 1], tc.NAMES[1], c['rec'][0, 1, 1], c['rec'][0, 1, 29])
    assert text == '#1234567 PEDESTR 54% 11.0M' and c['rec'].shape[1] == 10
    first = (10 - 1 - 1) * 29
    assert first + 1 <= 256 < first + 1 + len(text) - 1                 # glyph items on both sides of item 256
    img = np.zeros((101, 223, 3), np.uint8)
    assert ref.paint_label(img, text, 27, 21, 1, (1, 1, 1)) == ((6 * 26 + 1) * 9, sum(r.count('#') for ch in text for r in ref.ART[ch]))   # all inside
    # scale3_cross: the label of slot 0 has pixels on both sides of row 16 and of column 64
    c = by['scale3_cross']
    box = ref.label_box(40, 30, len(ref.label_text(3, 12, tc.NAMES[1], 0.9, 0.0)), 3)
    assert box[1] < 16 <= box[3] and box[0] < 64 <= box[2]
    # clipped: one label per edge, and a negative anchor in each direction
    c = by['clipped']
    boxes = [ref.label_box(int(r[20]), int(r[21]), len(ref.label_text(1, i, b'', 0, 0)), 4) for r, i in zip(c['rec'][0], c['ids'][0])]
    assert boxes[0][0] < 0 and boxes[0][3] > 36 and boxes[1][2] > 52 and boxes[2][1] < 0
    # ids_mix: ids beyond the palette, negative ids, id 0 beside tracked slots
    c = by['ids_mix']
    assert (np.abs(c['ids']) > len(tc.PALETTE3)).any() and (c['ids'] < 0).any() and ((c['ids'] == 0) & (c['rec'][..., 31] >= 1)).any()
    # track panel: a free slot between live ones, a coasting slot no record matches, a NaN velocity, a 7-digit id
    c = by['track_panel']
    t0 = c['state'][0][ref.HEADER:].reshape(5, ref.SLOT)
    assert [ref.live(s) for s in t0] == [True, True, False, True, True]
    assert t0[1, 4] > 0 and t0[1, 3] == 0 and t0[1, 6] == -1 and 17 not in np.abs(c['ids'])
    assert np.isnan(t0[3, 14]) and np.isfinite(t0[3, 7:14]).all()
    # the NaN velocity removes exactly that slot's mark: with the velocity repaired, more is painted and nothing else changes
    fixed = c['state'].copy()
    fixed[0][ref.HEADER + 3 * ref.SLOT + 14] = 0.5
    a, b = tc.backgrounds(c)[1], tc.backgrounds(c)[1]
    sa = ref.draw(tc.backgrounds(c)[0], c['rec'], c['ids'], None, a, c['state'], **c['params'])
    sb = ref.draw(tc.backgrounds(c)[0], c['rec'], c['ids'], None, b, fixed, **c['params'])
    assert sb['track_vel'] > sa['track_vel'] and sb['track_box'] == sa['track_box']
    # the fade case starts from a panel without a zero and has tiles that nothing touches
    c = by['track_fade']
    _, bev = tc.backgrounds(c)
    before = bev.copy()
    ref.draw(tc.backgrounds(c)[0], c['rec'], c['ids'], None, bev, c['state'], **c['params'])
    faded = ((before.astype(np.int64) * 200 + 128) >> 8).astype(np.uint8)
    same = (bev == faded).all(3)
    assert before.min() >= 1 and same[:, :16, :64].all() and not same.all() and (bev != before).any(3).mean() > 0.5


BASE_CASES = dc.cases()


@pytest.mark.parametrize('case', BASE_CASES, ids=[c['name'] for c in BASE_CASES])
def test_all_ids_zero_and_no_new_layer_is_draw_ref(case):
    imgs, bev = dc.backgrounds(case)
    want, want_bev = [i.copy() for i in imgs], None if bev is None else bev.copy()
    draw_ref.draw(want, case['rec'], case['K'], want_bev, **case['params'])
    ids = np.zeros(case['rec'].shape[:2], np.int32)
    stats = ref.draw(imgs, case['rec'], ids, case['K'], bev, None, palette=tc.PALETTE3, names=tc.NAMES, **case['params'])
    assert all(np.array_equal(a, b) for a, b in zip(imgs, want)) and (bev is None or np.array_equal(bev, want_bev))
    assert not any(stats[k] for k in stats if isinstance(k, str))
