"""Host side of the lens undistortion (include/rtm3d_hip.h, "lens undistortion"; no device): anchors that pin the numpy
restatement tests/lens_ref.py independently of the kernels, every refusal through the _check entry and the launchers' own
validation, the launch schedule against the case table, and the header, the library and the binding against each other."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import lens_cases as cases
from tests import lens_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _err(lib):
    return lib.rtm3d_last_error().decode()


# ---------------------------------------------------------------------------------------------------- the builder's rule
def test_zero_distortion_is_the_identity_map():
    m = ref.build_map('brown', cases.K_LENS, [0] * 8, cases.K_LENS, cases.EYE, 40, 56)
    v, u = np.meshgrid(np.arange(40), np.arange(56), indexing='ij')
    assert np.array_equal(m[..., 0], 32 * u) and np.array_equal(m[..., 1], 32 * v)
    m = ref.build_map('brown', cases.K_LENS, [0] * 8, cases.K_LENS, cases.EYE, 48, 64)       # a map larger than the lens: the same
    assert m[47, 63].tolist() == [32 * 63, 32 * 47]


def test_pure_k1_against_the_closed_form():
    """x_d = x (1 + k1 r^2) in plain Python floats, at pixels written out here."""
    fx, _, cx, _, fy, cy = cases.K_LENS[:6]
    k1 = -0.21
    m = ref.build_map('brown', cases.K_LENS, [k1], cases.K_LENS, cases.EYE, 48, 64)
    for u, v in ((0, 0), (63, 47), (27, 19), (28, 20), (5, 40), (60, 3)):
        x, y = (u - cx) / fx, (v - cy) / fy
        c = 1 + k1 * (x * x + y * y)
        want = [math.floor((fx * (x * c) + cx) * 32 + 0.5), math.floor((fy * (y * c) + cy) * 32 + 0.5)]
        assert m[v, u].tolist() == want, (u, v)
    # barrel distortion pulls the corner towards the centre: by hand, pixel (0, 0): x = -27.25 / 41.5, y = -19.5 / 43
    x, y = -27.25 / 41.5, -19.5 / 43.0
    r2 = x * x + y * y
    assert abs(r2 - 0.636811) < 1e-6 and m[0, 0, 0] == math.floor((41.5 * x * (1 - 0.21 * r2) + 27.25) * 32 + 0.5) == 117


def test_fisheye_axis_pixel_takes_the_small_r_branch():
    Kr = [30.0, 0, 31.0, 0, 30.0, 23.0, 0, 0, 1]
    U, V, outside = ref.build_uv('fisheye', cases.K_LENS, [0.1, 0.2, 0.3, 0.4], Kr, cases.EYE, 48, 64)
    assert not outside[23, 31] and U[23, 31] == cases.K_LENS[2] and V[23, 31] == cases.K_LENS[5]      # s = 1, not 0 / 0
    m = ref.build_map('fisheye', cases.K_LENS, [0.1, 0.2, 0.3, 0.4], Kr, cases.EYE, 48, 64)
    assert m[23, 31].tolist() == [32 * 27 + 8, 32 * 19 + 16]                                             # 27.25, 19.5
    # equidistant, no coefficients: theta / r at a pixel one focal length off the axis: r = 1, theta = pi / 4
    m = ref.build_map('fisheye', cases.K_LENS, [0, 0, 0, 0], Kr, cases.EYE, 48, 64)
    assert m[23, 61, 0] == math.floor((41.5 * (math.pi / 4) + 27.25) * 32 + 0.5) and m[23, 61, 1] == 32 * 19 + 16


def test_rays_behind_the_camera_are_outside():
    name, kind, K, dist, Kr, R, (ho, wo) = cases.BROWN_CASES[-1]
    assert name == 'tilted'
    m = ref.build_map(kind, K, dist, Kr, R, ho, wo)
    v, u = np.meshgrid(np.arange(ho), np.arange(wo), indexing='ij')
    Wz = R[6] * ((u - Kr[2]) / Kr[0]) + R[7] * ((v - Kr[5]) / Kr[4]) + R[8]
    behind = ~(Wz > 0)
    assert 0.05 < behind.mean() < 0.95
    assert (m[behind] == ref.OUTSIDE).all() and (m[..., 0] != ref.OUTSIDE).any()
    # and a position beyond 2^20 is outside although its ray is not behind
    assert ((m[..., 0] == ref.OUTSIDE) & ~behind).any()
    # Wz == 0 exactly: a rectified camera turned by 90 degrees looks along the physical x axis; its centre column has a = 0
    m = ref.build_map('brown', cases.K_LENS, [0] * 8, [10.0, 0, 3.0, 0, 10.0, 2.0, 0, 0, 1], [0, 0, 1, 0, 1, 0, -1, 0, 0], 5, 7)
    assert (m[:, 3:, 0] == ref.OUTSIDE).all() and (m[:, :3, 0] != ref.OUTSIDE).all()


@pytest.mark.parametrize('case', cases.FISHEYE_CASES, ids=[c[0] for c in cases.FISHEYE_CASES])
def test_fisheye_entries_near_a_rounding_boundary_are_rare(case):
    """The GPU test excuses (by at most 1) the entries whose U*32 + 0.5 lies within 1e-6 of an integer: at most 0.1 % of a case."""
    _, kind, K, dist, Kr, R, (ho, wo) = case
    near = ref.near_half(kind, K, dist, Kr, R, ho, wo)
    m = cases.reference_map(case)
    print('%s: %d of %d entries near a boundary, %d outside' % (case[0], near.sum(), near.size, (m[..., 0] == ref.OUTSIDE).sum()))
    assert near.mean() <= 0.001
    assert (m[..., 0] != ref.OUTSIDE).mean() > 0.3                       # the case maps something


# ---------------------------------------------------------------------------------------------------- the remap's rule
def test_identity_map_is_a_copy():
    rng = np.random.Generator(np.random.PCG64(1))
    src = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    v, u = np.meshgrid(np.arange(5), np.arange(7), indexing='ij')
    m = np.stack([32 * u, 32 * v], -1)
    assert np.array_equal(ref.remap(src, m, (9, 9, 9)), src)
    # a pixel's worth further: the last column and row come from the fill
    out = ref.remap(src, m + 32, (9, 8, 7))
    assert np.array_equal(out[:-1, :-1], src[1:, 1:]) and (out[-1] == (9, 8, 7)).all() and (out[:, -1] == (9, 8, 7)).all()


def test_half_pixel_shift_is_the_rounded_mean_of_two_neighbours():
    rng = np.random.Generator(np.random.PCG64(2))
    src = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    dx, dy = 2, 1
    v, u = np.meshgrid(np.arange(4), np.arange(5), indexing='ij')
    m = np.stack([32 * u + 32 * dx + 16, 32 * v + 32 * dy], -1)
    a, b = src[dy:dy + 4, dx:dx + 5].astype(int), src[dy:dy + 4, dx + 1:dx + 6].astype(int)
    assert np.array_equal(ref.remap(src, m), (a + b + 1) >> 1)
    m = np.stack([32 * u + 32 * dx, 32 * v + 32 * dy + 16], -1)
    a, b = src[dy:dy + 4, dx:dx + 5].astype(int), src[dy + 1:dy + 5, dx:dx + 5].astype(int)
    assert np.array_equal(ref.remap(src, m), (a + b + 1) >> 1)


def test_weights_sum_to_1024_and_outside_and_negative_positions():
    ax, ay = np.meshgrid(np.arange(32), np.arange(32))
    assert ((32 - ax) * (32 - ay) + ax * (32 - ay) + (32 - ax) * ay + ax * ay == 1024).all()
    src = np.full((2, 2, 3), 200, np.uint8)
    # a constant frame stays constant at every fraction inside it
    m = np.stack([ax, ay], -1)
    assert (ref.remap(src, m) == 200).all()
    # arithmetic shifts: -1 is pixel -1 at fraction 31 / 32, -33 pixel -2: one 32nd / nothing of pixel 0 against the fill
    m = np.array([[[-1, 0], [-32, 0], [-33, 0], [ref.OUTSIDE, 5], [2 ** 31 - 1, 0], [ref.OUTSIDE + 1, 0], [0, ref.OUTSIDE]]])
    out = ref.remap(src, m, (8, 8, 8))[0, :, 0].tolist()
    assert out == [(1 * 32 * 8 + 31 * 32 * 200 + 512) >> 10, 8, 8, 8, 8, 8, 8]
    # column -1 lies outside, column 0 inside, on both rows: samples (ix + 1, iy) and (ix + 1, iy + 1), bits 1 and 3
    assert ref.sample_pattern(m, 2, 2)[0].tolist() == [10, 10, 0, -1, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------- refusals
def remap_args(good, base=0x10000):
    """[(h, w, ho, wo)] -> (src pointers, hw, maps, dst pointers) with made-up, well-formed addresses."""
    n = len(good)
    src = (ctypes.c_void_p * n)(*[base + 0x1000000 * i for i in range(n)])
    dst = (ctypes.c_void_p * n)(*[base + 0x1000000 * i + 0x800000 for i in range(n)])
    hw = (ctypes.c_int * (2 * n))(*[v for g in good for v in g[:2]])
    maps = (_lib.LensMapC * n)()
    for i, g in enumerate(good):
        maps[i] = _lib.LensMapC(0x40000000 + 0x1000000 * i, g[2], g[3], 0)
    return src, hw, maps, dst


def test_every_remap_refusal_without_a_device(lib):
    good = [(6, 10, 4, 4), (5, 7, 8, 3), (3, 3, 3, 3)]
    fill = (ctypes.c_uint8 * 3)(1, 2, 3)
    plan = (_lib.RemapPlan * 1)()

    def refused(args, pattern, plan_too=False, B=3, fill=fill):
        src, hw, maps, dst = args
        assert lib.rtm3d_frames_remap_check(B, src, hw, maps, dst, fill) != 0, pattern
        assert re.search(pattern, _err(lib)), (_err(lib), pattern)
        # the launcher refuses before it touches a device (there is none here): the same message
        assert lib.rtm3d_frames_remap(None, B, src, hw, maps, dst, fill) != 0 and re.search(pattern, _err(lib)), (_err(lib), pattern)
        if plan_too:
            assert lib.rtm3d_frames_remap_plan(B, maps, plan) != 0 and re.search(pattern, _err(lib)), (_err(lib), pattern)

    assert lib.rtm3d_frames_remap_check(3, *remap_args(good), fill) == 0, _err(lib)
    a = remap_args(good); a[0][1] = None
    refused(a, r'frame 1: the source is a NULL')
    a = remap_args(good); a[3][2] = None
    refused(a, r'frame 2: the destination is a NULL')
    a = remap_args(good); a[2][0].d_map = None
    refused(a, r'frame 0: the map is a NULL', plan_too=True)
    for field, v in (('ho', 0), ('wo', 0), ('ho', -3), ('wo', 16385), ('ho', 16385)):
        a = remap_args(good); setattr(a[2][1], field, v)
        refused(a, r'frame 1: a map of -?\d+ x -?\d+; a side must lie in 1\.\.16384', plan_too=True)
    for k, v in ((0, 0), (1, 0), (0, -1), (1, 16385), (0, 16385)):
        a = remap_args(good); a[1][2 * 2 + k] = v
        refused(a, r'frame 2 is -?\d+ x -?\d+; a side must lie in 1\.\.16384')
    for off in (1, 2, 3):
        a = remap_args(good); a[2][2].d_map = a[2][2].d_map + off
        refused(a, r'frame 2: the map\'s address is no multiple of 4', plan_too=True)
    a = remap_args(good); a[2][1].reserved = 7
    refused(a, r'frame 1: reserved = 7', plan_too=True)
    # overlap: the destination begins inside its source, ends inside it, covers it, or is it
    h, w, ho, wo = good[1]
    for d in (0, h * w * 3 - 1, -(ho * wo * 3) + 1, -5):
        a = remap_args(good); a[3][1] = a[0][1] + d
        refused(a, r'frame 1: the destination overlaps its source')
    for d in (h * w * 3, -(ho * wo * 3)):                                  # touching is not overlapping
        a = remap_args(good); a[3][1] = a[0][1] + d
        assert lib.rtm3d_frames_remap_check(3, *a, fill) == 0, _err(lib)
    a = remap_args(good); a[3][1] = a[0][2]                                # another frame's source is not this frame's
    assert lib.rtm3d_frames_remap_check(3, *a, fill) == 0, _err(lib)
    a = remap_args(good); a[0][0] = a[0][0] + 3; a[3][2] = a[3][2] + 1     # any byte address is legal for frames
    assert lib.rtm3d_frames_remap_check(3, *a, fill) == 0, _err(lib)
    a = remap_args(good); a[2][1].d_map = a[2][0].d_map                    # frames may share a map
    a[2][1].ho, a[2][1].wo = a[2][0].ho, a[2][0].wo
    assert lib.rtm3d_frames_remap_check(3, *a, fill) == 0, _err(lib)
    refused(remap_args(good), r'B = 0', B=0, plan_too=True)
    refused(remap_args(good), r'null pointer', fill=None)
    src, hw, maps, dst = remap_args(good)
    assert lib.rtm3d_frames_remap_check(3, None, hw, maps, dst, fill) != 0 and lib.rtm3d_frames_remap_check(3, src, None, maps, dst, fill) != 0
    assert lib.rtm3d_frames_remap_check(3, src, hw, None, dst, fill) != 0 and lib.rtm3d_frames_remap_check(3, src, hw, maps, None, fill) != 0
    assert lib.rtm3d_frames_remap_plan(3, maps, None) != 0
    # the engine entry refuses a context that is no engine before anything else
    ctx = ctypes.c_void_p()
    assert lib.rtm3d_engine_detect_frames_lens(ctx, None, None, src, hw, 0, maps, dst, fill, None, None, None, None) != 0
    assert 'not made by rtm3d_engine_load' in _err(lib)


def build_args(n=2):
    m, r = (_lib.LensModelC * n)(), (_lib.LensRectC * n)()
    for i in range(n):
        m[i] = _lib.LensModelC(i % 2, 40, 56, (ctypes.c_double * 9)(*cases.K_LENS), (ctypes.c_double * 8)(0.1, 0.01, 0, 0))
        r[i] = _lib.LensRectC(48, 64, (ctypes.c_double * 9)(*cases.K_LENS), (ctypes.c_double * 9)(*cases.EYE))
    return m, r, (ctypes.c_void_p * n)(*[0x40000000 + 0x1000000 * i for i in range(n)])


def test_every_builder_refusal_without_a_device(lib):
    def refused(args, pattern, n=2):
        assert lib.rtm3d_lens_map_build(None, n, *args) != 0, pattern
        assert re.search(pattern, _err(lib)), (_err(lib), pattern)

    a = build_args(); a[0][1].kind = 2
    refused(a, r'map 1: unknown lens kind 2')
    a = build_args(); a[0][0].kind = -1
    refused(a, r'map 0: unknown lens kind -1')
    for i, pattern in ((1, r'map 1: K has an entry \[1\] or \[3\]'), (3, r'K has an entry \[1\] or \[3\]'), (6, r'K has a bottom row'),
                       (7, r'K has a bottom row')):
        a = build_args(); a[0][1].K[i] = 0.5
        refused(a, pattern)
        a = build_args(); a[1][1].K[i] = 0.5
        refused(a, pattern.replace('K has', 'the rectified K has'))
    a = build_args(); a[0][0].K[8] = 2.0
    refused(a, r'map 0: K has a bottom row that is not 0 0 1')
    for i in (0, 4):
        for v in (0.0, -3.0, float('nan')):
            a = build_args(); a[0][1].K[i] = v
            refused(a, r'map 1: K has fx or fy that is not > 0')
            a = build_args(); a[1][0].K[i] = v
            refused(a, r'map 0: the rectified K has fx or fy')
    for field, v in (('h', 0), ('w', 16385)):
        a = build_args(); setattr(a[0][1], field, v)
        refused(a, r'map 1: a lens of -?\d+ x -?\d+; a side must lie in 1\.\.16384')
    for field, v in (('ho', 0), ('wo', -1), ('ho', 16385)):
        a = build_args(); setattr(a[1][0], field, v)
        refused(a, r'map 0: a map of -?\d+ x -?\d+; a side must lie in 1\.\.16384')
    for i in (4, 5, 6, 7):
        a = build_args(); a[0][1].dist[i] = 1e-3                            # map 1 is the fisheye one
        refused(a, r'map 1: a fisheye lens has four coefficients')
    a = build_args(); a[2][1] = None
    refused(a, r'map 1: the map is a NULL')
    a = build_args(); a[2][0] = a[2][0] + 2
    refused(a, r'map 0: the map\'s address is no multiple of 4')
    refused(build_args(), r'n = 0', n=0)
    m, r, p = build_args()
    assert lib.rtm3d_lens_map_build(None, 2, None, r, p) != 0 and lib.rtm3d_lens_map_build(None, 2, m, None, p) != 0
    assert lib.rtm3d_lens_map_build(None, 2, m, r, None) != 0


# ---------------------------------------------------------------------------------------------------- the schedule
def test_remap_plan_against_the_case_table(lib):
    """Every boundary of the mapping - pixels per thread, the workgroup's span of a row, runs per workgroup, frames per launch -
    has a destination size on either side of it, and the plan says so."""
    one = (_lib.RemapPlan * 1)()
    seen = set()
    for ho, wo in cases.DST_SIZES:
        maps = (_lib.LensMapC * 1)(_lib.LensMapC(0x1000, ho, wo, 0))
        assert lib.rtm3d_frames_remap_plan(1, maps, one) == 0, _err(lib)
        p = one[0]
        assert (p.first, p.count, p.px_per_thread, p.threads) == (0, 1, cases.PX, cases.T)
        runs = cases.expected_runs(ho, wo)
        assert p.runs == runs and p.grid_x == (runs + cases.T - 1) // cases.T and p.grid_y == 1, (ho, wo)
        seen.add((np.sign(wo - cases.PX), np.sign(wo - cases.SPAN), np.sign(runs - cases.T)))
    assert {s[0] for s in seen} == {-1, 0, 1} and {s[1] for s in seen} == {-1, 0, 1} and {s[2] for s in seen} == {-1, 0, 1}
    widths = {wo for _, wo in cases.DST_SIZES}
    for k in (cases.PX, 2 * cases.PX, cases.SPAN):                         # one below, at and above a multiple of the run and of the span
        assert {k - 1, k, k + 1} <= widths, k
    assert sorted(cases.expected_runs(ho, wo) for ho, wo in cases.DST_BLOCK_EDGES) == [cases.T - 1, cases.T, cases.T + 1]
    assert max(ho * wo for ho, wo in cases.DST_SIZES) == 48 * 64 and max(h * w for h, w in cases.SRC_SIZES) == 37 * 53
    # chunks: 33 frames make two launches; each chunk's grid is its own largest destination's
    sizes = [cases.DST_SIZES[i % len(cases.DST_SIZES)] for i in range(cases.CHUNK + 1)]
    maps = (_lib.LensMapC * len(sizes))(*[_lib.LensMapC(0x1000, ho, wo, 0) for ho, wo in sizes])
    out = (_lib.RemapPlan * 2)()
    assert lib.rtm3d_frames_remap_plan(len(sizes), maps, out) == 0, _err(lib)
    for k, p in enumerate(out):
        chunk = sizes[k * cases.CHUNK:(k + 1) * cases.CHUNK]
        big = max(cases.expected_runs(ho, wo) for ho, wo in chunk)
        assert (p.first, p.count, p.grid_y) == (k * cases.CHUNK, len(chunk), len(chunk))
        assert p.runs == big and p.grid_x == (big + cases.T - 1) // cases.T
    assert [p.count for p in out] == [32, 1]
    # the largest legal map stays inside the grid limits
    maps = (_lib.LensMapC * 1)(_lib.LensMapC(0x1000, 16384, 16384, 0))
    assert lib.rtm3d_frames_remap_plan(1, maps, one) == 0
    assert one[0].runs == 4096 * 16384 and one[0].grid_x == 4096 * 16384 // 256


# ---------------------------------------------------------------------------------------------------- header, library, binding
def test_header_library_and_binding_agree(lib):
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    names = ['rtm3d_frames_remap_plan', 'rtm3d_frames_remap_check', 'rtm3d_frames_remap', 'rtm3d_lens_map_build',
             'rtm3d_engine_detect_frames_lens']
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        proto = re.search(r'int %s\(([^;]*)\);' % name, hdr).group(1)
        assert len(proto.split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
    assert '#define RTM3D_ABI_VERSION 9' in hdr and lib.rtm3d_abi_version() == 9
    assert re.search(r'#define RTM3D_LENS_OUTSIDE INT32_MIN\b', hdr) and re.search(r'#define RTM3D_LENS_BROWN 0\b', hdr)
    assert re.search(r'#define RTM3D_LENS_FISHEYE 1\b', hdr)
    structs = [('rtm3d_lens_map', _lib.LensMapC), ('rtm3d_lens_model', _lib.LensModelC), ('rtm3d_lens_rect', _lib.LensRectC),
               ('rtm3d_remap_plan', _lib.RemapPlan)]
    # sizes and the offset of the last field, through a tiny C program
    last = {'rtm3d_lens_map': 'reserved', 'rtm3d_lens_model': 'dist', 'rtm3d_lens_rect': 'R', 'rtm3d_remap_plan': 'grid_y'}
    body = ''.join('printf("%%zu %%zu ", sizeof(%s), offsetof(%s, %s));' % (s, s, last[s]) for s, _ in structs)
    src = '#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s return 0;}' % (REPO, body)
    os.makedirs(os.path.join(REPO, 'tests', '_build'), exist_ok=True)
    exe = os.path.join(REPO, 'tests', '_build', 'sizeof_lens')
    subprocess.run(['gcc', '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [v for s, c in structs for v in (ctypes.sizeof(c), getattr(c, last[s]).offset)]
    assert got == want, (got, want)
    assert ctypes.sizeof(_lib.LensMapC) == 24 and ctypes.sizeof(_lib.LensModelC) == 152 and ctypes.sizeof(_lib.LensRectC) == 152
    # the fields of the binding are the fields of the header, in order
    for s, c in structs:
        text = re.search(r'typedef struct %s \{(.*?)\} %s;' % (s, s), hdr, re.S).group(1)
        text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
        fields = [re.sub(r'\[\d+\]', '', f.strip().split()[-1].lstrip('*')) for decl in text.split(';') if decl.strip()
                  for f in decl.split(',')]
        assert fields == [f[0] for f in c._fields_], (s, fields)


def test_python_module_host_side(lib):
    from rtm3d_amd import lens
    m = lens.LensModel.brown(np.array(cases.K_LENS).reshape(3, 3), [-0.2, 0.05, 0, 0, 0.01], (40, 56))
    c = m.c_struct()
    assert (c.kind, c.h, c.w) == (0, 40, 56) and list(c.K) == cases.K_LENS and list(c.dist) == [-0.2, 0.05, 0, 0, 0.01, 0, 0, 0]
    assert lens.LensModel.fisheye(cases.K_LENS, [0.1, 0.2, 0.3, 0.4], (4, 5)).c_struct().kind == 1
    assert lens.KINDS == ref.KIND_ID and lens.OUTSIDE == ref.OUTSIDE and lens.CHUNK == cases.CHUNK
    with pytest.raises(ValueError, match='at most 4'):
        lens.LensModel.fisheye(cases.K_LENS, [0.1] * 5, (4, 5))
    with pytest.raises(ValueError, match='at most 8'):
        lens.LensModel.brown(cases.K_LENS, [0.1] * 9, (4, 5))
    with pytest.raises(ValueError, match='3 x 3'):
        lens.LensModel.brown([1, 2, 3], [], (4, 5))
    with pytest.raises(ValueError, match='unknown lens kind'):
        lens.LensModel('division', cases.K_LENS, [], (4, 5))
    with pytest.raises(ValueError, match='three bytes'):
        lens.c_fill((0, 256, 0))
    p = lens.plan((_lib.LensMapC * 1)(_lib.LensMapC(0x1000, 9, 17, 0)))
    assert len(p) == 1 and p[0].runs == 9 * 5
    with pytest.raises(RuntimeError, match='reserved = 1'):
        lens.plan((_lib.LensMapC * 1)(_lib.LensMapC(0x1000, 9, 17, 1)))
