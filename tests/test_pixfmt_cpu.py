"""Host side of the pixel formats (include/rtm3d_hip.h, "pixel formats"; no device): the plane layouts, the launch schedule
against the case table, every refusal, the library's coefficient tables against the ones derived from (Kr, Kb), and the
integer rule of tests/pixfmt_ref.py against the float64 matrix."""
import ctypes
import os
import re

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import pixfmt_cases as cases
from tests import pixfmt_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _err(lib):
    return lib.rtm3d_last_error().decode()


def src_array(specs, base=0x10000):
    """[(format name, h, w) or dict of overrides] -> ctypes array of FrameSrc with made-up, well-formed plane addresses."""
    arr = (_lib.FrameSrc * len(specs))()
    for i, sp in enumerate(specs):
        fmt, h, w = sp[:3]
        s = arr[i]
        for p, (row_bytes, rows) in enumerate(ref.layout(fmt, h, w)):
            s.plane[p], s.pitch[p] = base + 0x1000000 * p, row_bytes
        s.h, s.w, s.format = h, w, ref.FORMAT_ID[fmt]
    return arr


# ---------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize('fmt', ref.FORMATS)
def test_frame_src_layout(lib, fmt):
    for h, w in ((1, 1), (2, 2), (3, 5), (5, 3)):
        n = ctypes.c_int()
        pitch, rows = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
        assert lib.rtm3d_frame_src_layout(ref.FORMAT_ID[fmt], h, w, ctypes.byref(n), pitch, rows) == 0
        want = ref.layout(fmt, h, w)
        assert n.value == len(want) and [(pitch[i], rows[i]) for i in range(n.value)] == want, (fmt, h, w)
        assert all(pitch[i] == 0 and rows[i] == 0 for i in range(n.value, 3))
    # written out once, independent of the reference's table: a 3 x 5 frame, cw = 3, ch = 2
    n = ctypes.c_int()
    pitch, rows = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    assert lib.rtm3d_frame_src_layout(ref.FORMAT_ID[fmt], 3, 5, ctypes.byref(n), pitch, rows) == 0
    by_hand = {'rgb24': [(15, 3)], 'bgr24': [(15, 3)], 'rgba32': [(20, 3)], 'bgra32': [(20, 3)], 'gray8': [(5, 3)],
               'nv12': [(5, 3), (6, 2)], 'nv21': [(5, 3), (6, 2)], 'i420': [(5, 3), (3, 2), (3, 2)], 'yuyv': [(12, 3)], 'uyvy': [(12, 3)],
               'p010': [(10, 3), (12, 2)]}[fmt]
    assert [(pitch[i], rows[i]) for i in range(n.value)] == by_hand


def test_frame_src_layout_refusals(lib):
    n = ctypes.c_int()
    pitch, rows = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    assert lib.rtm3d_frame_src_layout(11, 4, 4, ctypes.byref(n), pitch, rows) != 0 and 'unknown format 11' in _err(lib)
    assert lib.rtm3d_frame_src_layout(-1, 4, 4, ctypes.byref(n), pitch, rows) != 0
    assert lib.rtm3d_frame_src_layout(5, 0, 4, ctypes.byref(n), pitch, rows) != 0 and '1..16384' in _err(lib)
    assert lib.rtm3d_frame_src_layout(5, 4, 16385, ctypes.byref(n), pitch, rows) != 0
    assert lib.rtm3d_frame_src_layout(5, 16384, 16384, ctypes.byref(n), pitch, rows) == 0


# ---------------------------------------------------------------------------------------------------- the schedule
def test_convert_plan_against_the_case_table(lib):
    """Every boundary of the mapping - pixels per thread, rows per thread, runs per workgroup, frames per launch - has a case
    on either side of it, and the plan says so."""
    one = (_lib.ConvertPlan * 1)()
    seen = set()
    for h, w in cases.SIZES + cases.WIDE:
        for fmt in ('nv12', 'bgra32'):
            assert lib.rtm3d_frames_convert_plan(1, src_array([(fmt, h, w)]), one) == 0, _err(lib)
            p = one[0]
            assert (p.first, p.count, p.px_per_thread, p.rows_per_thread, p.threads) == (0, 1, cases.G, cases.R, cases.T)
            runs = cases.expected_runs(h, w)
            assert p.runs == runs and p.grid_x == (runs + cases.T - 1) // cases.T and p.grid_y == 1, (h, w)
        seen.add((np.sign(w - cases.G), np.sign(h - cases.R), np.sign(runs - cases.T)))
    # widths below / at / above one run, heights below / at / above one row group, run counts below / at / above one workgroup
    assert {s[0] for s in seen} == {-1, 0, 1} and {s[1] for s in seen} == {-1, 0, 1} and {s[2] for s in seen} == {-1, 0, 1}
    # ... and a partial last run / row group next to whole ones
    assert any(w % cases.G == 0 for _, w in cases.SIZES) and any(w % cases.G for _, w in cases.SIZES)
    assert any(h % cases.R == 0 for h, _ in cases.SIZES) and any(h % cases.R for h, _ in cases.SIZES)
    runs = sorted(cases.expected_runs(h, w) for h, w in cases.BLOCK_EDGES)
    assert runs == [cases.T - 1, cases.T - 1, cases.T, cases.T, cases.T + 1, cases.T + 1]
    # chunks: 2 x 32 + 6 frames of mixed sizes; each chunk's grid is its own largest frame's
    sizes = [cases.SIZES[i % len(cases.SIZES)] for i in range(2 * cases.CHUNK + 6)]
    specs = [(ref.FORMATS[i % len(ref.FORMATS)], h, w) for i, (h, w) in enumerate(sizes)]
    out = (_lib.ConvertPlan * 3)()
    assert lib.rtm3d_frames_convert_plan(len(specs), src_array(specs), out) == 0, _err(lib)
    for k, p in enumerate(out):
        chunk = sizes[k * cases.CHUNK:(k + 1) * cases.CHUNK]
        big = max(cases.expected_runs(h, w) for h, w in chunk)
        assert (p.first, p.count, p.grid_y) == (k * cases.CHUNK, len(chunk), len(chunk))
        assert p.runs == big and p.grid_x == (big + cases.T - 1) // cases.T
    assert [p.count for p in out] == [32, 32, 6]
    # the largest legal frame stays inside the grid limits
    assert lib.rtm3d_frames_convert_plan(1, src_array([('gray8', 16384, 16384)]), one) == 0
    assert one[0].runs == 2048 * 8192 and one[0].grid_x == 65536


# ---------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_without_a_device(lib):
    """rtm3d_frames_convert_check is the launcher's own validation (the launcher calls it first); the plan validates the
    sources the same way."""
    dst = (ctypes.c_void_p * 3)(0x7000000, 0x7100000, 0x7200000)
    good = [('nv12', 6, 10), ('p010', 5, 7), ('bgra32', 3, 3)]
    plan = (_lib.ConvertPlan * 1)()

    def refused(arr, pattern, dst=dst, order=0, B=3, plan_too=True):
        assert lib.rtm3d_frames_convert_check(B, arr, dst, order) != 0, pattern
        assert re.search(pattern, _err(lib)), (_err(lib), pattern)
        if plan_too:
            assert lib.rtm3d_frames_convert_plan(B, arr, plan) != 0 and re.search(pattern, _err(lib)), (_err(lib), pattern)

    assert lib.rtm3d_frames_convert_check(3, src_array(good), dst, 0) == 0, _err(lib)
    assert lib.rtm3d_frames_convert_check(3, src_array(good), dst, 1) == 0, _err(lib)
    a = src_array(good); a[1].format = 11
    refused(a, r'frame 1 has the unknown format 11')
    a = src_array(good); a[2].format = -1
    refused(a, r'frame 2 has the unknown format -1')
    a = src_array(good); a[0].matrix = 2
    refused(a, r'frame 0: unknown matrix 2')
    a = src_array(good); a[1].range = -1
    refused(a, r'frame 1: unknown matrix 0 or range -1')
    a = src_array(good); a[2].matrix, a[2].range = 7, 7                     # ignored for RGB
    assert lib.rtm3d_frames_convert_check(3, a, dst, 0) == 0, _err(lib)
    a = src_array(good); a[2].reserved = 1
    refused(a, r'frame 2: reserved = 1')
    a = src_array(good); a[0].plane[1] = None
    refused(a, r'frame 0: plane 1 is a NULL')
    a = src_array(good); a[2].plane[0] = None
    refused(a, r'frame 2: plane 0 is a NULL')
    a = src_array([('i420', 4, 4)] + good[1:]); a[0].plane[2] = None
    refused(a, r'frame 0: plane 2 is a NULL')
    a = src_array(good)                                                   # planes the format does not use may be NULL (they are)
    assert a[2].plane[1] is None and a[0].plane[2] is None
    d = (ctypes.c_void_p * 3)(0x7000000, None, 0x7200000)
    refused(src_array(good), r'frame 1: the destination is a NULL', dst=d, plan_too=False)
    for field, v in (('h', 0), ('w', 0), ('h', -3), ('w', 16385), ('h', 16385)):
        a = src_array(good); setattr(a[1], field, v)
        refused(a, r'frame 1 is -?\d+ x -?\d+; a side must lie in 1\.\.16384')
    a = src_array(good); a[0].pitch[0] = 9
    refused(a, r'frame 0: pitch 9 of plane 0 is below the row\'s 10 bytes')
    a = src_array(good); a[0].pitch[1] = 9
    refused(a, r'frame 0: pitch 9 of plane 1')
    a = src_array(good); a[1].pitch[0] = 15                                # P010, 7 wide: 14 bytes of luma; 15 is enough but odd
    refused(a, r'frame 1: plane 0 of a P010 surface has an odd address or pitch')
    a = src_array(good); a[1].plane[1] = a[1].plane[1] + 1
    refused(a, r'frame 1: plane 1 of a P010 surface has an odd')
    a = src_array(good); a[0].plane[0] = a[0].plane[0] + 1; a[0].pitch[0] = 11; a[2].plane[0] = a[2].plane[0] + 3   # legal elsewhere
    assert lib.rtm3d_frames_convert_check(3, a, dst, 0) == 0, _err(lib)
    refused(src_array(good), r'dst_order 2', order=2, plan_too=False)
    refused(src_array(good), r'B = 0', B=0)
    assert lib.rtm3d_frames_convert_check(3, None, dst, 0) != 0 and lib.rtm3d_frames_convert_check(3, src_array(good), None, 0) != 0
    # the launcher itself refuses before it touches a device (there is none here): the same message
    a = src_array(good); a[1].format = 11
    assert lib.rtm3d_frames_convert(None, 3, a, dst, 0) != 0 and 'frame 1 has the unknown format 11' in _err(lib)
    # the engine entry refuses a context that is no engine before anything else
    ctx = ctypes.c_void_p()
    assert lib.rtm3d_engine_detect_frames_src(ctx, None, src_array(good), dst, 0, None, None, None, None) != 0


# ---------------------------------------------------------------------------------------------------- tables and the rule
HEADER_TABLES = {   # as printed in the header
    ('bt601', 'limited', 8): [76309, 104597, -25675, -53279, 132201], ('bt601', 'limited', 10): [76309, 104597, -25675, -53279, 132201],
    ('bt709', 'limited', 8): [76309, 117489, -13975, -34925, 138438], ('bt709', 'limited', 10): [76309, 117489, -13975, -34925, 138438],
    ('bt601', 'full', 8): [65536, 91881, -22553, -46802, 116130], ('bt709', 'full', 8): [65536, 103206, -12276, -30679, 121609],
    ('bt601', 'full', 10): [65344, 91612, -22487, -46664, 115789], ('bt709', 'full', 10): [65344, 102903, -12240, -30589, 121252]}


def test_library_tables_equal_the_derived_ones(lib):
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    for (m, r, bits), want in HEADER_TABLES.items():
        tab, yo, co, S = ref.table(m, r, bits)
        assert tab == want, (m, r, bits, tab)
        assert ', '.join('%d' % v for v in want) in re.sub(r' +', ' ', hdr), 'the header prints %s' % (want,)
        for fmt in (('p010',) if bits == 10 else ('nv12', 'nv21', 'i420', 'yuyv', 'uyvy')):
            out = (ctypes.c_int * 8)()
            assert lib.rtm3d_yuv_coefficients(ref.FORMAT_ID[fmt], ('bt601', 'bt709').index(m), ('limited', 'full').index(r), out) == 0
            assert list(out) == want + [yo, co, S], (fmt, m, r, list(out))
    out = (ctypes.c_int * 8)()
    assert lib.rtm3d_yuv_coefficients(ref.FORMAT_ID['rgb24'], 0, 0, out) != 0 and lib.rtm3d_yuv_coefficients(5, 2, 0, out) != 0
    # int32 suffices: the largest intermediate of any table at any sample value
    for (m, r, bits), (cy, crv, cgu, cgv, cbu) in HEADER_TABLES.items():
        top, c = (255, 128) if bits == 8 else (1023, 512)
        worst = abs(cy) * top + max(abs(crv), abs(cgu) + abs(cgv), abs(cbu)) * c + (1 << 17)
        assert worst < 1.5e8, (m, r, bits, worst)


@pytest.mark.parametrize('matrix,rng', cases.MATRIX_RANGE)
def test_integer_rule_against_the_float64_matrix(matrix, rng):
    """A stride-3 grid over the 2^24 triples plus the extremes: the integer rule is within 1 of the float64 matrix with
    round-half-up and clamp (exhaustively it differs in fewer than 0.03 % of the values, never by more than 1)."""
    axis = np.unique(np.concatenate([np.arange(0, 256, 3), [0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255]]))
    Y, U, V = np.meshgrid(axis, axis, axis, indexing='ij')
    got = ref.yuv_to_rgb(Y, U, V, matrix, rng).astype(np.int32)
    want = ref.yuv_to_rgb_real(Y, U, V, matrix, rng).astype(np.int32)
    d = np.abs(got - want)
    print('%s %s: max diff %d, %.4f %% of %d values differ' % (matrix, rng, d.max(), 100.0 * (d > 0).mean(), d.size))
    assert d.max() <= 1


@pytest.mark.parametrize('matrix,rng', cases.MATRIX_RANGE)
def test_ten_bit_rule_against_the_float64_matrix(matrix, rng):
    axis = np.unique(np.concatenate([np.arange(0, 1024, 13), [0, 63, 64, 65, 511, 512, 513, 939, 940, 941, 959, 960, 961, 1022, 1023]]))
    Y, U, V = np.meshgrid(axis, axis, axis, indexing='ij')
    d = np.abs(ref.yuv_to_rgb(Y, U, V, matrix, rng, 10).astype(np.int32) - ref.yuv_to_rgb_real(Y, U, V, matrix, rng, 10).astype(np.int32))
    assert d.max() <= 1


def test_anchors():
    g = np.arange(256)
    mid = np.full(256, 128)
    for m in ('bt601', 'bt709'):
        assert ref.yuv_to_rgb(16, 128, 128, m, 'limited').tolist() == [0, 0, 0]
        assert ref.yuv_to_rgb(235, 128, 128, m, 'limited').tolist() == [255, 255, 255]
        assert ref.yuv_to_rgb(64, 512, 512, m, 'limited', 10).tolist() == [0, 0, 0]
        assert ref.yuv_to_rgb(940, 512, 512, m, 'limited', 10).tolist() == [255, 255, 255]
        assert np.array_equal(ref.yuv_to_rgb(g, mid, mid, m, 'full'), np.repeat(g[:, None], 3, 1))      # full-range grey passes through
        assert ref.yuv_to_rgb(1023, 512, 512, m, 'full', 10).tolist() == [255, 255, 255]
        # below black and above white clamp
        assert ref.yuv_to_rgb(0, 128, 128, m, 'limited').tolist() == [0, 0, 0] and ref.yuv_to_rgb(255, 128, 128, m, 'limited').tolist() == [255] * 3


def test_reference_layouts_and_orders():
    """The numpy restatement on a frame small enough to write out: a 2 x 3 NV12 / NV21 / I420 / YUYV / UYVY frame of one grey
    level and one saturated chroma sample lands where the formats say; the padding is never read."""
    Y = np.array([[50, 60, 70], [80, 90, 100]], np.uint8)
    cb, cr = np.array([[100, 200]], np.uint8), np.array([[30, 140]], np.uint8)          # cw = 2, ch = 1
    want = ref.yuv_to_rgb(Y, np.array([[100, 100, 200]] * 2), np.array([[30, 30, 140]] * 2), 'bt601', 'limited')
    pad = 0xEE

    def pitched(rows, pitch):
        out = np.full((len(rows) - 1) * pitch + len(rows[-1]), pad, np.uint8)
        for i, r in enumerate(rows):
            out[i * pitch:i * pitch + len(r)] = r
        return out

    uv = np.stack([cb, cr], -1).reshape(1, 4)
    src = {'format': 'nv12', 'h': 2, 'w': 3, 'planes': [pitched(Y, 5), pitched(uv, 4)], 'pitches': [5, 4]}
    assert np.array_equal(ref.convert(src), want)
    assert np.array_equal(ref.convert(src, 'bgr'), want[:, :, ::-1])
    src = {'format': 'nv21', 'h': 2, 'w': 3, 'planes': [pitched(Y, 3), pitched(uv[:, [1, 0, 3, 2]], 9)], 'pitches': [3, 9]}
    assert np.array_equal(ref.convert(src), want)
    src = {'format': 'i420', 'h': 2, 'w': 3, 'planes': [pitched(Y, 4), pitched(cb, 2), pitched(cr, 7)], 'pitches': [4, 2, 7]}
    assert np.array_equal(ref.convert(src), want)
    # 4:2:2 carries chroma per row: give both rows the same
    row = lambda y: [y[0], 100, y[1], 30, y[2], 200, pad, 140]
    src = {'format': 'yuyv', 'h': 2, 'w': 3, 'planes': [pitched([row(Y[0]), row(Y[1])], 11)], 'pitches': [11]}
    assert np.array_equal(ref.convert(src), want)
    swap = lambda r: [r[1], r[0], r[3], r[2], r[5], r[4], r[7], r[6]]
    src = {'format': 'uyvy', 'h': 2, 'w': 3, 'planes': [pitched([swap(row(Y[0])), swap(row(Y[1]))], 8)], 'pitches': [8]}
    assert np.array_equal(ref.convert(src), want)
    # P010: the same samples scaled to 10 bits, junk in the six low bits
    p16 = lambda a: ((np.asarray(a, np.uint16) << 2 << 6) | 0x2A).astype('<u2').view(np.uint8)
    src = {'format': 'p010', 'h': 2, 'w': 3, 'planes': [pitched([p16(Y[0]), p16(Y[1])], 8), pitched([p16(uv[0])], 8)], 'pitches': [8, 8]}
    want10 = ref.yuv_to_rgb(Y.astype(np.int32) * 4, np.array([[400, 400, 800]] * 2), np.array([[120, 120, 560]] * 2), 'bt601', 'limited', 10)
    assert np.array_equal(ref.convert(src), want10) and np.abs(want10.astype(int) - want.astype(int)).max() <= 1
    # packed RGB
    px = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    src = {'format': 'bgra32', 'h': 2, 'w': 3, 'planes': [pitched(px.reshape(2, 12), 13)], 'pitches': [13]}
    assert np.array_equal(ref.convert(src), px[:, :, [2, 1, 0]]) and np.array_equal(ref.convert(src, 'bgr'), px[:, :, :3])
    src = {'format': 'gray8', 'h': 2, 'w': 3, 'planes': [pitched(Y, 3)], 'pitches': [3]}
    assert np.array_equal(ref.convert(src), np.repeat(Y[:, :, None], 3, 2))


def test_python_module_host_side(lib):
    """pixfmt.layout / yuv_coefficients / format names without a device."""
    from rtm3d_amd import pixfmt
    assert pixfmt.layout('nv12', 3, 5) == [(5, 3), (6, 2)] and pixfmt.layout('bgra', 2, 2) == [(8, 2)]
    assert pixfmt.yuv_coefficients('p010', 'bt709', 'full') == ([65344, 102903, -12240, -30589, 121252], 0, 512, 18)
    assert pixfmt.FORMATS == ref.FORMAT_ID
    with pytest.raises(ValueError, match='unknown pixel format'):
        pixfmt.layout('nv16', 2, 2)
    with pytest.raises(RuntimeError, match='1..16384'):
        pixfmt.layout('nv12', 0, 2)
    p = pixfmt.plan(src_array([('yuyv', 9, 17)]))
    assert len(p) == 1 and p[0].runs == 3 * 5
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    for name, v in pixfmt.FORMATS.items():
        assert re.search(r'#define RTM3D_PIX_%s %d\b' % (name.upper(), v), hdr), name
