"""CPU: the regime table of the uint8 input path (tests/preprocess_cases.py) against the launcher's own statement of its schedule
(rtm3d_preprocess_batch_plan, a host function: the launcher calls the same code) - every case runs in the regime it is named
after - and the oracle (oracle/preprocess_ref.py) at the table's shapes against float64 bilinear interpolation.  The kernels
themselves: tests/test_gpu_preprocess.py."""
import ctypes

import numpy as np
import pytest

from oracle import preprocess_ref
from rtm3d_amd import _lib
from tests import preprocess_cases as pc


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def plan_of(lib, shapes, canvas):
    """([plan tuple per sub-batch], None) or (None, error message)."""
    a = np.array(shapes, np.int32).reshape(-1, 4)
    hw, rhw = np.ascontiguousarray(a[:, :2]), np.ascontiguousarray(a[:, 2:])
    out = (_lib.PreprocessPlan * ((len(a) + 63) // 64))()
    rc = lib.rtm3d_preprocess_batch_plan(len(a), hw.ctypes.data_as(ctypes.c_void_p), rhw.ctypes.data_as(ctypes.c_void_p),
                                         canvas[0], canvas[1], out)
    if rc != 0:
        assert rc == 1
        return None, lib.rtm3d_last_error().decode()
    return [tuple(getattr(p, f) for f in pc.PLAN_FIELDS) for p in out], None


def test_the_table_holds_every_named_regime():
    assert list(pc.CASES) == ['multiband_up2', 'unstaged_wide', 'widest_table', 'table_refused', 'subbatches_70', 'anisotropic',
                              'misaligned', 'odd_pads', 'mean_edges', 'full_canvas_all', 'replay']


@pytest.mark.parametrize('name', list(pc.CASES))
def test_case_runs_in_the_regime_it_names(lib, name):
    case = pc.CASES[name]
    exp = case['expect']
    H, W = case['canvas']
    plans, err = plan_of(lib, case['images'], case['canvas'])
    if 'refused' in exp:
        assert plans is None and exp['refused'] in err, err
        return
    assert err is None, err
    assert plans == exp['plan']
    if 'second' in case:
        assert plan_of(lib, case['second'], case['canvas'])[0] == exp['plan_second']
    # per image: staged / unstaged / misaligned / short bands, from the plan's numbers and the oracle's row coefficients
    got = {}
    for i, (shape, off) in enumerate(zip(case['images'], pc.offsets(case))):
        p = dict(zip(pc.PLAN_FIELDS, plans[i // 64]))
        assert p['first'] <= i < p['first'] + p['count']
        k = pc.band_stats(shape, off, p['band_rows'], p['stage_bytes'])
        assert k[0] + k[1] == -(-shape[2] // p['band_rows'])
        got[k] = got.get(k, 0) + 1
    assert got == exp['bands']
    # what else the case is there for, counted from its shapes
    shapes = case['images']
    assert sum((rh > h) + (rw > w) for h, w, rh, rw in shapes) == exp.get('upscale', 0)
    assert sum((rh < h) + (rw < w) for h, w, rh, rw in shapes) == exp.get('downscale', 0)
    assert sum((rh, rw) == (H, W) for _, _, rh, rw in shapes) == exp.get('full_canvas_images', 0)
    assert sum(bool((H - rh) % 2 or (W - rw) % 2) for _, _, rh, rw in shapes) >= exp.get('odd_pad_images', 0)
    p0 = dict(zip(pc.PLAN_FIELDS, plans[0]))
    assert (p0['bands'] > p0['grid_x']) == exp.get('multiband', False)
    assert (p0['border_grid_x'] == 0) == (exp.get('full_canvas_images', 0) == len(shapes))
    assert p0['col_bytes'] + p0['stage_bytes'] + 4608 <= 65536              # dynamic + static LDS of pre_interior_kernel


def test_the_named_regimes_in_detail(lib):
    C = pc.CASES
    # multiband_up2: workgroups 0 and 1 take two bands, the other thirty one; both the x2 up-scale and the identity do
    p = dict(zip(pc.PLAN_FIELDS, plan_of(lib, C['multiband_up2']['images'], C['multiband_up2']['canvas'])[0][0]))
    assert (p['band_rows'], p['bands'], p['grid_x']) == (16, 34, 32)
    assert [len(range(x, p['bands'], p['grid_x'])) for x in range(p['grid_x'])] == [2, 2] + [1] * 30
    assert {s[2] for s in C['multiband_up2']['images']} == {530}
    # unstaged_wide: one row per band; all 50 bands of image 0 gather, all 50 of image 1 are staged
    p = dict(zip(pc.PLAN_FIELDS, plan_of(lib, C['unstaged_wide']['images'], C['unstaged_wide']['canvas'])[0][0]))
    assert p['band_rows'] == 1
    assert pc.band_stats(C['unstaged_wide']['images'][0], 0, 1, p['stage_bytes'])[:2] == (0, 50)
    assert pc.band_stats(C['unstaged_wide']['images'][1], 0, 1, p['stage_bytes'])[:2] == (50, 0)
    # widest_table: the widest accepted row leaves no stage; one pixel wider is refused, whatever else is in the batch
    p = dict(zip(pc.PLAN_FIELDS, plan_of(lib, C['widest_table']['images'], C['widest_table']['canvas'])[0][0]))
    assert (p['col_bytes'], p['stage_bytes']) == (60000, 0)
    plans, err = plan_of(lib, [(2, 2, 2, 2)] * 64 + [(1, 7501, 1, 7501)], (2, 7504))
    assert plans is None and 'resized width 7501 exceeds' in err
    # subbatches_70: 64 + 6
    plans = plan_of(lib, C['subbatches_70']['images'], C['subbatches_70']['canvas'])[0]
    assert [(q[0], q[1]) for q in plans] == [(0, 64), (64, 6)]
    # misaligned: every image starts off a 16-byte boundary, at the six offsets, with a pitch that is no multiple of 16 (or a
    # single row); three spans are shorter than a chunk
    m = C['misaligned']
    assert m['offsets'] == [1, 3, 7, 8, 13, 15]
    assert all(h == 1 or (w * 3) % 16 for h, w, _, _ in m['images'])
    assert [h * w * 3 for h, w, _, _ in m['images']][:3] == [3, 12, 15] and {(1, 1), (2, 2), (1, 5)} <= {s[:2] for s in m['images']}
    assert {(s[:2] == s[2:]) for s in m['images']} == {True, False}
    # odd_pads: both pads odd; full height with a side border; full width with rows above and below
    H, W = C['odd_pads']['canvas']
    s = C['odd_pads']['images']
    assert any((H - rh) % 2 and (W - rw) % 2 for _, _, rh, rw in s)
    assert any(rh == H and rw < W for _, _, rh, rw in s) and any(rw == W and rh < H for _, _, rh, rw in s)
    # anisotropic: up in one axis and down in the other, both ways round, next to an image that fills the canvas
    s = C['anisotropic']['images']
    assert s[0][2] > s[0][0] and s[0][3] < s[0][1] and s[1][2] < s[1][0] and s[1][3] > s[1][1] and s[2][2:] == C['anisotropic']['canvas']


def test_mean_edges_content_has_the_sums_it_is_about():
    case = pc.CASES['mean_edges']
    imgs = pc.make_images(case)
    n = imgs[0].shape[0] * imgs[0].shape[1]
    sums = [im.reshape(-1, 3).astype(np.int64).sum(0) for im in imgs]
    k = np.array([7, 100, 200])
    assert (imgs[0] == 255).all() and (imgs[1][..., 1] == 0).all()
    np.testing.assert_array_equal(sums[2], k * n)
    np.testing.assert_array_equal(sums[3], (k + 1) * n - 1)
    for (canvas, s), colour in zip(pc.oracle_canvases(case, imgs), case['expect']['border_colours']):
        np.testing.assert_array_equal(s // n, colour)
        np.testing.assert_array_equal(canvas[0, 0], colour)                  # the oracle's border is that colour
        np.testing.assert_array_equal(canvas[-1, -1], colour)


def test_replay_calls_differ_where_a_stale_sum_would_show():
    case = pc.CASES['replay']
    a = [c[0, 0].astype(int) for c, _ in pc.oracle_canvases(case, pc.make_images(case, 0), 0)]
    b = [c[0, 0].astype(int) for c, _ in pc.oracle_canvases(case, pc.make_images(case, 1), 1)]
    assert all((x >= 200).all() for x in a) and all((x <= 55).all() for x in b)


def test_refusals_of_the_plan_entry(lib):
    out = (_lib.PreprocessPlan * 2)()
    ok = np.array([4, 4], np.int32)

    def call(B, hw, rhw, H, W, o=out):
        hw = None if hw is None else np.ascontiguousarray(hw, np.int32)
        rhw = None if rhw is None else np.ascontiguousarray(rhw, np.int32)
        rc = lib.rtm3d_preprocess_batch_plan(B, None if hw is None else hw.ctypes.data_as(ctypes.c_void_p),
                                             None if rhw is None else rhw.ctypes.data_as(ctypes.c_void_p), H, W, o)
        return rc, lib.rtm3d_last_error().decode()

    assert call(1, ok, None, 8, 8)[0] == 0 and (out[0].first, out[0].count) == (0, 1)        # NULL resized sizes: no resize
    for B, hw, o in ((0, ok, out), (-1, ok, out), (1, None, out), (1, ok, None)):
        rc, err = call(B, hw, None, 8, 8, o)
        assert rc == 1 and 'bad arguments' in err
    for hw, rhw, what in (([4, 4], [9, 4], '4x4 -> 9x4'), ([4, 4], [4, 9], '4x4 -> 4x9'), ([0, 4], None, '0x4 -> 0x4'),
                          ([4, -1], None, '4x-1'), ([4, 4], [0, 4], '-> 0x4'), ([4, 4], [4, 0], '-> 4x0')):
        rc, err = call(1, hw, rhw, 8, 8)
        assert rc == 1 and 'image 0 ' in err and what in err and 'does not fit the 8x8 canvas' in err, err
    # a bad image in the second sub-batch is named by its index in the whole batch
    hw = np.tile(ok, (70, 1))
    hw[66] = (9, 4)
    rc, err = call(70, hw, None, 8, 8)
    assert rc == 1 and 'image 66 (9x4' in err


def test_plan_struct_has_the_c_layout(lib, tmp_path):
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s/include/rtm3d_hip.h"\nint main(void){printf("%%zu", sizeof(rtm3d_preprocess_plan));'
           % repo + ''.join('printf(" %%zu", offsetof(rtm3d_preprocess_plan, %s));' % f for f in pc.PLAN_FIELDS) + 'return 0;}')
    c, exe = str(tmp_path / 'l.c'), str(tmp_path / 'l')
    open(c, 'w').write(src)
    subprocess.run(['gcc', '-std=c99', '-Werror', '-o', exe, c], check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(_lib.PreprocessPlan)] + [getattr(_lib.PreprocessPlan, f).offset for f in pc.PLAN_FIELDS]


def _float_bilinear(img, nh, nw):
    """float64 bilinear interpolation at OpenCV's sample positions (the check of test_oracle_resize_properties)."""
    h, w = img.shape[:2]
    ys = np.clip((np.arange(nh) + 0.5) * h / nh - 0.5, 0, h - 1)
    xs = np.clip((np.arange(nw) + 0.5) * w / nw - 0.5, 0, w - 1)
    y0 = np.floor(ys).astype(int); x0 = np.floor(xs).astype(int)
    y1 = np.minimum(y0 + 1, h - 1); x1 = np.minimum(x0 + 1, w - 1)
    fy = (ys - y0)[:, None, None]; fx = (xs - x0)[None, :, None]
    f = img.astype(np.float64)
    return (f[y0][:, x0] * (1 - fx) + f[y0][:, x1] * fx) * (1 - fy) + (f[y1][:, x0] * (1 - fx) + f[y1][:, x1] * fx) * fy


@pytest.mark.parametrize('name', ['multiband_up2', 'anisotropic', 'misaligned', 'full_canvas_all', 'replay'])
def test_oracle_resize_within_one_lsb_of_float_bilinear(name):
    """Guards the oracle at the new shapes: on the up-scaling and anisotropic cases the fixed-point resize stays within 1 LSB of
    float64 bilinear interpolation."""
    case = pc.CASES[name]
    seen = 0
    for img, (h, w, rh, rw) in list(zip(pc.make_images(case), case['images']))[:6]:
        if rh > h or rw > w:
            got = preprocess_ref.resize_bilinear_u8(img, (rh, rw)).astype(np.float64)
            assert got.shape == (rh, rw, 3)
            assert np.abs(got - _float_bilinear(img, rh, rw)).max() <= 1.0
            seen += 1
    assert seen >= 1
