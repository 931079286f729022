"""Host side of the raw sensor frames (include/rtm3d_hip.h, "raw sensor frames"; no device): the numpy restatement
tests/raw_ref.py on what can be said about it without a second implementation (a mosaic of one colour comes back as that
colour; pack / unpack; a frame written out by hand), the plane layouts, the launch schedule against the case table, every
refusal, the tone tables, the parameters of raw.RawSource, and the header against the binding."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import raw_cases as cases
from tests import raw_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _err(lib):
    return lib.rtm3d_last_error().decode()


def src_array(specs, base=0x10000):
    """[(layout, bits, h, w)] -> ctypes array of RawSrc with made-up, well-formed plane addresses, RGGB, unit parameters."""
    arr = (_lib.RawSrc * len(specs))()
    for i, (layout, bits, h, w) in enumerate(specs):
        s = arr[i]
        s.plane, s.pitch, s.h, s.w = base + 0x1000000 * i, ref.row_bytes(layout, w), h, w
        s.layout, s.bits, s.pattern = ref.LAYOUT_ID[layout], bits, 0
        for k in range(4):
            s.gain[k] = 1024
        s.ccm[0] = s.ccm[4] = s.ccm[8] = 1024
    return arr


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('method', cases.METHODS)
@pytest.mark.parametrize('pattern', cases.PATTERNS)
def test_constant_colour_comes_back(pattern, method):
    """The filters of every case sum to 16 and the fold keeps CFA colours: a mosaic sampled from ANY constant colour is that
    colour at every pixel, borders included - every layout, every size from 2 x 2 to 7 x 7."""
    rng = np.random.Generator(np.random.PCG64(3))
    for layout, bits in cases.LAYOUT_BITS:
        M = (1 << bits) - 1
        for h in range(2, 8):
            for w in range(2, 8):
                colour = rng.integers(0, M + 1, 3)
                img = np.broadcast_to(colour, (h, w, 3))
                src = ref.make_source(ref.bayer_of(img, pattern), layout, bits, pattern, pitch=ref.row_bytes(layout, w) + (h + w) % 3 * 2, rng=rng)
                got = ref.demosaic(src, method)
                t = colour >> (bits - 12) if bits >= 12 else colour << (12 - bits)
                assert np.array_equal(got, np.broadcast_to((t >> 4).astype(np.uint8), (h, w, 3))), (layout, bits, h, w, colour)
                assert np.array_equal(ref.demosaic(src, method, 'bgr'), got[:, :, ::-1])


def test_filters_sum_to_sixteen_and_reach_both_clamps():
    """Random 16-bit data at 9 x 11 drives the MHC filters below 0 and above M (the clamps are live code), and the checkerboard
    of the GPU table does so at every bit depth."""
    rng = np.random.Generator(np.random.PCG64(4))
    s = rng.integers(0, 65536, (9, 11))
    m = s
    at = lambda dy, dx: np.take(np.take(m, ref.fold(np.arange(9) + dy, 9), 0), ref.fold(np.arange(11) + dx, 11), 1)
    ax1, ay1, ax2, ay2 = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0), at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
    d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    unclamped = np.stack([8 * m + 4 * (ax1 + ay1) - 2 * (ax2 + ay2), 12 * m + 4 * d - 3 * (ax2 + ay2), 10 * m + 8 * ax1 - 2 * d - 2 * ax2 + ay2,
                          10 * m + 8 * ay1 - 2 * d - 2 * ay2 + ax2])
    unclamped = (unclamped + 8) >> 4
    assert unclamped.min() < 0 and unclamped.max() > 65535
    for taps in ((8, 4, 4, -2, -2, 0), (12, 0, 0, -3, -3, 4), (10, 8, 0, -2, 1, -2), (10, 0, 8, 1, -2, -2)):   # C, ax1, ay1, ax2, ay2, d
        assert taps[0] + 2 * sum(taps[1:5]) + 4 * taps[5] == 16
    for layout, bits in cases.ONE_PER_LAYOUT:
        M = (1 << bits) - 1
        src = cases.value_source('checker', layout, bits, 'rggb', 9, 11, rng)
        out = ref.demosaic(src, 'mhc')
        assert out.min() == 0 and out.max() == 255 and np.array_equal(ref.mosaic(src), np.where(np.add.outer(np.arange(9), np.arange(11)) & 1, M, 0))


def test_fold():
    assert ref.fold(np.arange(-4, 7), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert ref.fold(np.arange(-3, 8), 4).tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    for n in range(2, 9):                                                       # the folded position keeps the parity
        i = np.arange(-20, 30)
        assert np.array_equal(ref.fold(i, n) & 1, i & 1) and ref.fold(i, n).min() == 0 and ref.fold(i, n).max() == n - 1


def test_a_frame_written_out_by_hand():
    """3 x 3 RGGB, bilinear, unit parameters - small enough to follow with a pencil.  R sits at the four corners, B in the middle."""
    m = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]])
    src = ref.make_source(m * 16, 'u16', 12, 'rggb')
    got = ref.demosaic(src, 'bilinear').astype(int)
    # centre (1, 1) is B = 50: G = (40 + 60 + 20 + 80 + 2) >> 2 = 50, R = (10 + 30 + 70 + 90 + 2) >> 2 = 50
    assert got[1, 1].tolist() == [50, 50, 50]
    # corner (0, 0) is R = 10: the folded neighbours are (0, 1) twice and (1, 0) twice, the diagonals all (1, 1)
    assert got[0, 0].tolist() == [10, (20 + 20 + 40 + 40 + 2) >> 2, 50]
    # (0, 1) is G = 20 on a red row: H = (10 + 30 + 1) >> 1 = R, V = (50 + 50 + 1) >> 1 = B
    assert got[0, 1].tolist() == [20, 20, 50]
    # (1, 0) is G = 40 on a blue row: H = (50 + 50 + 1) >> 1 = B, V = (10 + 70 + 1) >> 1 = R
    assert got[1, 0].tolist() == [40, 40, 50]
    # the same values in the other three patterns: the mosaic moves, the colours follow
    assert ref.demosaic(ref.make_source(m * 16, 'u16', 12, 'bggr'), 'bilinear').astype(int)[0, 1].tolist() == [50, 20, 20]
    assert ref.demosaic(ref.make_source(m * 16, 'u16', 12, 'grbg'), 'bilinear').astype(int)[0, 0].tolist() == [20, 10, 40]
    assert ref.demosaic(ref.make_source(m * 16, 'u16', 12, 'gbrg'), 'bilinear').astype(int)[0, 0].tolist() == [40, 10, 20]
    # black level, gain with its rounding, colour matrix and tone on one pixel of a constant frame
    src = ref.make_source(np.full((2, 2), 1000), 'u16', 12, 'rggb', black=[100, 0, 0, 100], gain=[1536, 1024, 1024, 2047])
    assert ref.mosaic(src).tolist() == [[1350, 1000], [1000, (900 * 2047 + 512) >> 10]]
    src['ccm'] = [2048, -1024, 0, 0, 1024, 0, -8192, 0, 8192]
    tone = (255 - (np.arange(4096) >> 4)).astype(np.uint8)
    src['tone'] = tone
    r, g, b = 1350, 1000, (900 * 2047 + 512) >> 10
    want = [np.clip((2048 * r - 1024 * g + 512) >> 10, 0, 4095), g, np.clip((-8192 * r + 8192 * b + 512) >> 10, 0, 4095)]
    assert ref.demosaic(src, 'bilinear')[0, 0].tolist() == [int(tone[v]) for v in want]


@pytest.mark.parametrize('layout,bits', cases.LAYOUT_BITS)
def test_pack_unpack_round_trip(layout, bits):
    rng = np.random.Generator(np.random.PCG64(5))
    for h, w in ((2, 2), (3, 5), (4, 7), (5, 8), (2, 9), (3, 13)):                 # widths that do and do not fill a MIPI group
        rb = ref.row_bytes(layout, w)
        for pitch in (rb, rb + 6):
            s = rng.integers(0, 1 << bits, (h, w))
            plane = ref.pack(s, layout, bits, pitch, rng=rng)
            assert plane.dtype == np.uint8 and plane.size == (h - 1) * pitch + rb
            assert np.array_equal(ref.unpack(plane, layout, bits, h, w, pitch), s), (layout, bits, h, w, pitch)
    # the bytes of one MIPI group, by the CSI-2 text: four (two) high bytes, then the low bits, sample 0 in the lowest
    if layout == 'mipi10':
        assert ref.pack(np.array([[0x3FF, 0x001, 0x2AA, 0x154]] * 2), layout, 10)[:5].tolist() == [0xFF, 0x00, 0xAA, 0x55, 0b00100111]
    if layout == 'mipi12':
        assert ref.pack(np.array([[0xABC, 0x123]] * 2), layout, 12)[:3].tolist() == [0xAB, 0x12, 0x3C]
    if layout == 'u16':                                                               # a sample above the range is clipped, not wrapped
        assert ref.unpack(np.array([0xFF, 0xFF, 0x00, 0x04], np.uint8), layout, 10, 1, 2, 4).tolist() == [[1023, 1023]]
    if layout == 'u16_msb':
        assert ref.unpack(np.array([0xFF, 0xFF, 0x7F, 0x00], np.uint8), layout, 10, 1, 2, 4).tolist() == [[1023, 1]]


# ---------------------------------------------------------------------------------------------------- layout and plan
@pytest.mark.parametrize('layout,bits', cases.LAYOUT_BITS)
def test_raw_src_layout(lib, layout, bits):
    from rtm3d_amd import raw
    for h, w in ((2, 2), (3, 5), (5, 7), (16384, 16384)):
        assert raw.layout(layout, bits, h, w) == (ref.row_bytes(layout, w), h)
    by_hand = {'u8': 5, 'u16': 10, 'u16_msb': 10, 'mipi10': 10, 'mipi12': 9}[layout]
    assert raw.layout(layout, bits, 3, 5) == (by_hand, 3)
    with pytest.raises(RuntimeError, match='2..16384'):
        raw.layout(layout, bits, 1, 5)
    with pytest.raises(RuntimeError, match='2..16384'):
        raw.layout(layout, bits, 4, 16385)
    with pytest.raises(RuntimeError, match='does not take 9 bits'):
        raw.layout(layout, 9, 4, 4)
    p, r = ctypes.c_int(), ctypes.c_int()
    assert lib.rtm3d_raw_src_layout(5, 8, 4, 4, ctypes.byref(p), ctypes.byref(r)) != 0 and 'unknown layout 5' in _err(lib)
    assert lib.rtm3d_raw_src_layout(0, 8, 4, 4, None, ctypes.byref(r)) != 0 and 'null' in _err(lib)


def test_plan_and_the_case_table(lib):
    """The schedule of the launcher, and the table against it: every regime the kernel's code distinguishes exists among the
    sizes of the GPU test for the tile the plan reports."""
    from rtm3d_amd import raw
    TW, TH, halo, threads = cases.tile()
    assert TW % 8 == 0 and TH % 2 == 0 and threads == (TW // 8) * (TH // 2) and halo == 2
    sizes = cases.sizes(TW, TH)
    assert len(sizes) == 11 and len(set(sizes)) == 11 and all(h >= 2 and w >= 2 for h, w in sizes)
    seen = set()
    for h, w in sizes:
        r = cases.regimes(h, w, TW, TH, halo)
        assert r <= cases.ALL_REGIMES
        seen |= r
    assert seen == cases.ALL_REGIMES, cases.ALL_REGIMES - seen
    # one entry per chunk of 32; tiles = the largest frame's, whatever its place in the chunk
    specs = [('u8', 8, h, w) for h, w in sizes] * 6 + [('mipi10', 10, 3 * TH + 1, 2 * TW + 1)]
    arr = src_array(specs)
    for method in (0, 1):
        p = raw.plan(arr, method)
        assert len(p) == 3 and [(e.first, e.count) for e in p] == [(0, 32), (32, 32), (64, 3)]
        for e in p:
            want = max(-(-w // TW) * -(-h // TH) for _, _, h, w in specs[e.first:e.first + e.count])
            assert (e.tile_w, e.tile_h, e.halo, e.threads) == (TW, TH, halo, threads)
            assert e.tiles == want and e.grid_x == want and e.grid_y == e.count
        assert p[2].tiles == 4 * 3
    out = (_lib.DemosaicPlan * 1)()
    assert lib.rtm3d_frames_demosaic_plan(1, src_array([('u8', 8, 16384, 16384)]), 0, out) == 0
    assert out[0].tiles == (16384 // TW) * (16384 // TH) < 65536 * 2
    assert lib.rtm3d_frames_demosaic_plan(1, arr, 0, None) != 0 and lib.rtm3d_frames_demosaic_plan(0, arr, 0, out) != 0
    assert lib.rtm3d_frames_demosaic_plan(1, arr, 2, out) != 0 and 'method 2' in _err(lib)


# ---------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_names_its_frame(lib):
    specs = [('u8', 8, 4, 6), ('u16', 12, 5, 7), ('mipi10', 10, 6, 9), ('mipi12', 12, 3, 5), ('u16_msb', 16, 2, 2)]
    dst = (ctypes.c_void_p * 5)(*[0x9000000 + 0x10000 * i for i in range(5)])

    def refused(change, word, method=0, order=0, d=dst, n=5):
        arr = src_array(specs)
        change(arr)
        assert lib.rtm3d_frames_demosaic_check(n, arr, d, method, order) != 0, word
        assert word in _err(lib), (_err(lib), word)

    assert lib.rtm3d_frames_demosaic_check(5, src_array(specs), dst, 0, 0) == 0
    assert lib.rtm3d_frames_demosaic_check(5, src_array(specs), dst, 1, 1) == 0

    def setter(i, field, value, index=None):
        def f(arr):
            if index is None:
                setattr(arr[i], field, value)
            else:
                getattr(arr[i], field)[index] = value
        return f

    refused(setter(4, 'layout', 5), 'frame 4 has the unknown layout 5')
    refused(setter(4, 'layout', -1), 'frame 4 has the unknown layout -1')
    refused(setter(3, 'pattern', 4), 'frame 3 has the unknown pattern 4')
    refused(lambda a: None, 'method 2', method=2)
    refused(lambda a: None, 'method -1', method=-1)
    refused(lambda a: None, 'dst_order 2', order=2)
    refused(setter(0, 'bits', 10), 'frame 0: layout 0 does not take 10 bits')
    refused(setter(1, 'bits', 8), 'frame 1: layout 1 does not take 8 bits')
    refused(setter(1, 'bits', 11), 'frame 1: layout 1 does not take 11 bits')
    refused(setter(2, 'bits', 12), 'frame 2: layout 3 does not take 12 bits')
    refused(setter(3, 'bits', 10), 'frame 3: layout 4 does not take 10 bits')
    refused(setter(4, 'bits', 18), 'frame 4: layout 2 does not take 18 bits')
    refused(setter(2, 'reserved', 7), 'frame 2: reserved = 7')
    refused(setter(2, 'pad', 1), 'frame 2: pad = 1')
    refused(setter(3, 'plane', None), 'frame 3: the plane is a NULL')
    refused(lambda a: None, 'frame 4: the destination is a NULL', d=(ctypes.c_void_p * 5)(dst[0], dst[1], dst[2], dst[3], None))
    refused(setter(2, 'h', 1), 'frame 2 is 1 x 9')
    refused(setter(2, 'w', 1), 'frame 2 is 6 x 1')
    refused(setter(4, 'h', 16385), 'frame 4 is 16385 x 2')
    refused(setter(0, 'w', 16385), 'frame 0 is 4 x 16385')
    refused(setter(0, 'pitch', 5), 'frame 0: pitch 5 is below the row\'s 6 bytes')
    refused(setter(2, 'pitch', 14), 'frame 2: pitch 14 is below the row\'s 15 bytes')       # 9 samples: three groups of 5 bytes
    refused(setter(3, 'pitch', 8), 'frame 3: pitch 8 is below the row\'s 9 bytes')
    refused(setter(1, 'pitch', 15), 'frame 1: a uint16 plane has an odd')
    refused(setter(4, 'plane', 0x10001), 'frame 4: a uint16 plane has an odd')
    refused(setter(0, 'black', 256, 3), 'frame 0: black[3] = 256 is above 255')
    refused(setter(2, 'black', 1024, 0), 'frame 2: black[0] = 1024 is above 1023')
    refused(setter(1, 'gain', 16385, 2), 'frame 1: gain[2] = 16385 is above 16384')
    refused(setter(3, 'ccm', 8193, 5), 'frame 3: ccm[5] = 8193 is outside')
    refused(setter(3, 'ccm', -8193, 8), 'frame 3: ccm[8] = -8193 is outside')
    refused(lambda a: None, 'B = 0', n=0)
    assert lib.rtm3d_frames_demosaic_check(5, None, dst, 0, 0) != 0 and lib.rtm3d_frames_demosaic_check(5, src_array(specs), None, 0, 0) != 0
    # the bounds themselves are legal, and so are odd addresses and pitches of the byte layouts
    arr = src_array(specs)
    arr[0].black[0], arr[0].gain[0], arr[0].ccm[1], arr[0].ccm[2], arr[0].plane, arr[0].pitch = 255, 16384, 8192, -8192, 0x10003, 7
    arr[2].plane, arr[2].pitch, arr[3].plane, arr[3].pitch = 0x2000001, 17, 0x3000003, 11
    assert lib.rtm3d_frames_demosaic_check(5, arr, dst, 0, 0) == 0, _err(lib)
    # the launcher refuses through the same code before it touches a device: nothing is launched, on a machine with none too
    bad = src_array(specs)
    bad[4].reserved = 1
    assert lib.rtm3d_frames_demosaic(None, 5, bad, dst, 0, 0) != 0 and 'frame 4: reserved = 1' in _err(lib)


# ---------------------------------------------------------------------------------------------------- the Python module
def test_tone_tables():
    from rtm3d_amd import raw
    lin = raw.tone_table('linear').numpy()
    assert lin.dtype == np.uint8 and lin.shape == (4096,) and np.array_equal(lin, np.arange(4096) >> 4)
    for kind in ('linear', 'srgb', 2.2, 1.0, 0.5):
        t = raw.tone_table(kind).numpy().astype(int)
        assert t.shape == (4096,) and t[0] == 0 and t[-1] == 255 and (np.diff(t) >= 0).all(), kind
    srgb = raw.tone_table('srgb').numpy().astype(int)
    assert (srgb >= lin.astype(int)).all() and srgb[4095 // 5] > 118                  # 18 % grey lands near 118 / 255 (0.46)
    u = 0.5
    assert srgb[2048] == int(np.floor((1.055 * u ** (1 / 2.4) - 0.055) * 255 + 0.5)) or abs(srgb[2048] - 188) <= 1
    assert np.abs(raw.tone_table(1.0).numpy().astype(int) - np.floor(np.arange(4096) / 4095 * 255 + 0.5)).max() == 0
    with pytest.raises(ValueError, match='tone_table'):
        raw.tone_table('rec709')
    with pytest.raises(ValueError, match='positive'):
        raw.tone_table(0.0)


def test_cell_parameters_of_a_source():
    """Floats to Q10 with round-half-up, scalars to the four cells, (r, g, b) gains through the pattern."""
    from rtm3d_amd import raw
    assert raw.q10(1.0) == 1024 and raw.q10(0.00048828125) == 1 and raw.q10(0.000488) == 0 and raw.q10(-0.00048828125) == 0
    assert raw.q10(1.5) == 1536 and raw.q10(-1.5) == -1536 and raw.q10(2.0 - 1 / 2048) == 2048
    assert raw.cell_params('rggb', 10) == ([0] * 4, [1024] * 4, ref.IDENTITY)
    for name, cells in ref.CELLS.items():
        assert raw.PATTERN_CELLS[name] == cells and raw.PATTERNS[name] == ref.PATTERN_ID[name]
        black, gain, ccm = raw.cell_params(name, 12, 64, (2.0, 1.0, 1.5))
        assert black == [64] * 4 and gain == [(2048, 1024, 1536)[c] for c in cells]
    assert raw.cell_params(2, 12, [1, 2, 3, 4095], [1, 1.25, 16, 0])[:2] == ([1, 2, 3, 4095], [1024, 1280, 16384, 0])
    c = raw.cell_params('bggr', 8, ccm=[[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [-8, 0, 8]])[2]
    assert c == [1843, -614, -205, -307, 1638, -307, -8192, 0, 8192]
    for kw, word in (({'black': 4096}, 'black'), ({'black': -1}, 'black'), ({'black': [1, 2]}, 'black'), ({'gains': 16.001}, 'gains'),
                     ({'gains': -0.1}, 'gains'), ({'gains': [1, 2]}, 'gains'), ({'ccm': [1, 2, 3]}, 'ccm'), ({'ccm': np.eye(3) * 8.01}, 'ccm')):
        with pytest.raises(ValueError, match=word):
            raw.cell_params('rggb', 12, **kw)
    with pytest.raises(ValueError, match='unknown pattern'):
        raw.cell_params('rgbg', 12)


def test_raw_source_validation():
    """What RawSource refuses before it looks at the device: names, bits, and a plane that is no CUDA tensor."""
    import torch
    from rtm3d_amd import raw
    plane = torch.zeros(4, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match='unknown layout'):
        raw.RawSource(plane, 'mipi14', 'rggb')
    with pytest.raises(ValueError, match='unknown layout'):
        raw.RawSource(plane, 5, 'rggb')
    with pytest.raises(ValueError, match='unknown pattern'):
        raw.RawSource(plane, 'u8', 'rgbw')
    with pytest.raises(ValueError, match='takes 8 bits'):
        raw.RawSource(plane, 'u8', 'rggb', bits=10)
    with pytest.raises(ValueError, match='takes 16 / 14 / 12 / 10 bits'):
        raw.RawSource(plane, 'u16', 'rggb', bits=8)
    with pytest.raises(ValueError, match='gains'):
        raw.RawSource(plane, 'u8', 'rggb', gains=17)
    with pytest.raises(ValueError, match='CUDA tensor'):
        raw.RawSource(plane, 'u8', 'rggb')
    with pytest.raises(ValueError, match='non-empty list of RawSource'):
        raw.c_sources([])
    with pytest.raises(ValueError, match='unknown method'):
        raw.plan(src_array([('u8', 8, 4, 4)]), 'ahd')
    assert raw.layout_id('raw10') == raw.LAYOUTS['mipi10'] and raw.layout_id('RAW12') == 4 and raw.layout_id(2) == 2
    assert raw.LAYOUTS == ref.LAYOUT_ID and raw.METHODS == ref.METHOD_ID
    assert sorted((n, b) for n, bs in raw.LAYOUT_BITS.items() for b in bs) == sorted(ref.LAYOUT_BITS)


# ---------------------------------------------------------------------------------------------------- header and binding
def test_header_binding_and_facade_agree(lib):
    from rtm3d_amd import engine, raw
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert '#define RTM3D_ABI_VERSION 9' in hdr and _lib.ABI_VERSION == 9
    names = ('rtm3d_raw_src_layout', 'rtm3d_frames_demosaic_plan', 'rtm3d_frames_demosaic_check', 'rtm3d_frames_demosaic',
             'rtm3d_engine_detect_frames_raw')
    for name in names:
        m = re.search(r'int %s\(([^;]*)\);' % name, hdr)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    for table, prefix in ((raw.LAYOUTS, 'RTM3D_RAW_'), (raw.PATTERNS, 'RTM3D_CFA_'), (raw.METHODS, 'RTM3D_DEMOSAIC_')):
        for name, v in table.items():
            assert re.search(r'#define %s%s %d\b' % (prefix, name.upper(), v), hdr), name
        assert len(re.findall(r'#define %s\w+ \d+' % prefix, hdr)) == len(table)
    # the mirrored structs have the C sizes and field offsets (through a tiny C program)
    import subprocess
    src = ('#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu", '
           'sizeof(rtm3d_raw_src), offsetof(rtm3d_raw_src, pitch), offsetof(rtm3d_raw_src, black), offsetof(rtm3d_raw_src, ccm), '
           'offsetof(rtm3d_raw_src, pad), sizeof(rtm3d_demosaic_plan));return 0;}' % REPO)
    os.makedirs(os.path.join(REPO, 'tests', '_build'), exist_ok=True)
    exe = os.path.join(REPO, 'tests', '_build', 'sizeof_raw_src')
    subprocess.run(['gcc', '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    R = _lib.RawSrc
    assert got == [ctypes.sizeof(R), R.pitch.offset, R.black.offset, R.ccm.offset, R.pad.offset, ctypes.sizeof(_lib.DemosaicPlan)] and got[0] == 80
    # the facade: detect_frames_raw is the twin of detect_frames_src with `method` in front of `order`
    a = list(inspect.signature(engine.Engine.detect_frames_raw).parameters)
    b = list(inspect.signature(engine.Engine.detect_frames_src).parameters)
    assert a == b[:3] + ['method'] + b[3:] and a[-1] == 'nms3d'
    assert list(inspect.signature(raw.demosaic).parameters) == ['sources', 'method', 'order', 'out']
    assert list(inspect.signature(raw.RawSource.__init__).parameters)[1:] == ['plane', 'layout', 'pattern', 'bits', 'size', 'pitch', 'black',
                                                                               'gains', 'ccm', 'tone']
    # one listing per kernel source, the example among the examples, and no word of the raw stage inside the pixel formats
    mk = open(os.path.join(REPO, 'rtm3d_amd', 'csrc', 'Makefile')).read()
    assert ' demosaic.hip ' in mk and 'EXAMPLES += engine_detect_raw' in mk and os.path.exists(os.path.join(REPO, 'examples', 'engine_detect_raw.c'))
    from rtm3d_amd import pixfmt
    assert len(pixfmt.FORMATS) == 11
