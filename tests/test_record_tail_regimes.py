"""CPU: the yardstick of the record tail (tests/record_tail_ref.py) against the project's host forms - tests/util.pack_records_reference,
kitti_results.calc_proj_corners / kitti_label_values, preprocess.resize_K / adjust_K, rtm3d_frame_geometry - and against the
vectors made by running the reference (tests/golden/project_cases.npz); and every condition the cases of
tests/record_tail_regimes.py must meet, on the yardstick alone: the sizes reach the block / wave / chunk boundaries they are
named for, every Ry is clear of an fp32 rounding midpoint, every snap-window case is clear of the 1e-3 threshold and every
sub-threshold case shows a missing snap, the depth cases have the finite / infinite / NaN pattern they claim, kept and not-kept
slots meet inside one wave in both orders, the alpha cases wrap, the clip cases clip and no coordinate sits on a clip limit, the
NMS case does suppress a slot, and the old kept rule of the KITTI rows (flag >= 1) would write other rows.  No device is used."""
import math

import numpy as np
import pytest
import torch

from rtm3d_amd import kitti_results as kr
from rtm3d_amd import preprocess
from rtm3d_amd.model_utils import Boxes3D, FUN_ACCEPT
from tests import box_overlap_ref
from tests import record_tail_ref as ref
from tests import record_tail_regimes as rg
from tests.util import load_golden, pack_records_reference

RTOL, ATOL = 1e-9, 1e-7          # the bar of test_project_boxes_device_vs_reference_vectors


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def close(got, want):
    return abs(got - want) <= RTOL * abs(want) + ATOL


# ------------------------------------------------------------------------------------------------ 1. pack_records
def test_pack_cases_reach_the_regimes_of_the_kernel():
    shapes = {(c['B'], c['topk']) for c in map(rg.pack_case, rg.PACK_NAMES)}
    assert shapes == {(1, 1), (1, 7), (1, 8), (3, 3), (5, 13)}
    assert 1 * 1 * 32 == 32 and 1 * 7 * 32 < 256 == 1 * 8 * 32 and 5 * 13 * 32 > 8 * 256
    per_shape = {}
    for name in rg.PACK_NAMES:
        c = rg.pack_case(name)
        per_shape.setdefault('rel', set()).update(int(v) - c['topk'] if v > 0 else int(v) for v in c['n'])
        assert c['x'].shape == (c['B'] * c['topk'], 8) and c['cls'].dtype == np.int64 and c['status'].dtype == np.int32
        assert set(c['status'].tolist()) <= {-1, 0, 1, 2, 3} and c['fun_accept'] == FUN_ACCEPT == rg.FUN_ACCEPT
    assert per_shape['rel'] >= {0, -2, 5}                                 # n = 0 and topk (both 0 here), -2, topk + 5
    assert any(0 in c['n'].tolist() for c in map(rg.pack_case, rg.PACK_NAMES))
    assert any(0 < v < c['topk'] for c in map(rg.pack_case, rg.PACK_NAMES) for v in c['n'])


def yard_pack(c, solved=True):
    s = (c['x'], c['fun'], c['status']) if solved else (None, None, None)
    return ref.pack_records(c['n'], c['cls'], c['score'], c['mproj'], c['verts'], c['bbox'], c['topk'], *s, fun_accept=c['fun_accept'])


@pytest.mark.parametrize('name', rg.PACK_NAMES + ['kept_edge_0', 'fields'])
def test_pack_yardstick_equals_the_torch_definition(name):
    c = rg.pack_case(name)
    bx = Boxes3D(c['B'] * c['topk'], 'cpu')
    bx.x.copy_(torch.from_numpy(c['x'].copy())); bx.fun.copy_(torch.from_numpy(c['fun'].copy())); bx.status.copy_(torch.from_numpy(c['status'].copy()))
    t = [torch.from_numpy(np.array(c[k])) for k in ('n', 'cls', 'score', 'mproj', 'verts', 'bbox')]
    for solved in (True, False):
        want = pack_records_reference(*t, c['topk'], bx if solved else None).numpy()
        got = yard_pack(c, solved)
        assert got.dtype == np.float32 and bits(got) == bits(want), (name, solved, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:6])
        live = (np.arange(c['topk'])[None, :] < c['n'][:, None])
        assert not got[~live].any() and (got[live][:, 31] >= 1).all()
        if not solved:
            assert not got[..., 24:31].any() and set(got[..., 31].ravel().tolist()) <= {0.0, 1.0}


def test_kept_edge_slots_alternate():
    for k, acc in enumerate(rg.EDGE_ACCEPTS):
        c = rg.pack_case('kept_edge_%d' % k)
        flags = yard_pack(c)[0, :, 31].tolist()
        if math.isnan(acc):
            assert flags == [1.0] * len(flags)
        else:
            assert flags == [2.0, 1.0] * (len(flags) // 2), (acc, flags)
        kinds = {kind for _, kind in rg.EDGE_SLOTS}
        assert kinds == {'below', 'equal', 'nan', '-inf', '+inf'} and {s for s, _ in rg.EDGE_SLOTS} == {-1, 0, 3}
        if math.isfinite(acc):
            assert c['fun'][0] < acc == c['fun'][1] and np.nextafter(c['fun'][0], math.inf) == acc
    assert rg.EDGE_ACCEPTS[:3] == [0.1, 0.25, math.inf] and rg.pack_case('kept_edge_2')['fun'][0] == np.finfo(np.float64).max


def test_field_case_rounds_as_claimed():
    c = rg.pack_case('fields')
    rec = yard_pack(c)[0]
    assert rec[:4, 0].tolist() == [0.0, -3.0, 2.0 ** 24, -2.0 ** 24] and c['cls'][2] == 2 ** 24 + 1
    assert rec[6, 26] == np.inf and rec[6, 27] == -np.inf and rec[7, 24] == np.inf and rec[7, 29] == -np.inf
    assert [(float(a), float(b)) for a, b in c['x'][:6, :2]] == rg.YAW_PAIRS and math.copysign(1, c['x'][1, 0]) == -1
    want = [math.pi, -math.pi, 0.0, math.pi / 2, -math.pi / 2, math.atan2(3, 4)]
    assert rec[:6, 30].tolist() == [float(np.float32(v)) for v in want]
    assert (rec[:, 31] == 2).all()


def test_every_ry_is_clear_of_an_fp32_midpoint():
    n = 0
    for name in rg.PACK_ALL:
        for x0, x1 in rg.pack_case(name)['x'][:, :2]:
            assert rg.ry_clear_of_fp32_midpoints(float(x0), float(x1)), (name, x0, x1)
            n += 1
    assert n >= 150
    r = (float(np.float32(1.25)) + float(np.nextafter(np.float32(1.25), np.float32(2)))) / 2      # the check sees a midpoint
    assert not rg.ry_clear_of_fp32_midpoints(math.sin(r), math.cos(r))


# ------------------------------------------------------------------------------------------------ 2. box_project.h
def test_projection_yardstick_equals_the_reference_vectors():
    g = load_golden('project_cases.npz')
    skipped = 0
    for i in range(len(g['Ry'])):
        ry = float(g['Ry'][i])
        if abs(min(abs(math.sin(ry)), abs(math.cos(ry))) - 1e-3) < 1e-9:             # on the threshold: atan2(sin, cos) may land on either side
            skipped += 1
            continue
        d, loc = g['dimension'][i], g['location'][i]
        xs = [math.sin(ry), math.cos(ry), d[2], d[0], d[1], loc[0], loc[1], loc[2]]
        proj, rect = ref.project_box(xs, g['K'].reshape(9))
        np.testing.assert_allclose(proj, g['proj'][i], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(rect, np.concatenate([g['proj'][i][:8].min(0), g['proj'][i][:8].max(0)]), rtol=RTOL, atol=ATOL)
    assert skipped <= 8


def test_projection_yardstick_equals_the_host_form_on_the_pool():
    for name, xs, k in rg.pool():
        proj, rect = ref.project_box(xs, rg.KS[k])
        if name.startswith('zero_size'):
            continue
        assert np.isfinite(proj).all(), name
        want = kr.calc_proj_corners([xs[3], xs[4], xs[2]], xs[5:8], math.atan2(xs[0], xs[1]), rg.KS[k])
        np.testing.assert_allclose(proj, want, rtol=RTOL, atol=ATOL, err_msg=name)
        np.testing.assert_allclose(rect, np.concatenate([want[:8].min(0), want[:8].max(0)]), rtol=RTOL, atol=ATOL)


def test_corner_order():
    xs = [0.0, 1.0, 4.0, 2.0, 6.0, 0.0, 0.0, 10.0]                      # ry = 0: X = +-2, Y = +-1, Z = 10 +- 3
    K = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    proj, _ = ref.project_box(xs, K)
    signs = [(i, j, k) for i in (1, -1) for j in (1, -1) for k in (1, -1)] + [(0, 0, 0)]
    for (u, v), (i, j, k) in zip(proj, signs):
        assert u == 2.0 * i / (10.0 + 3.0 * k + 1e-6) and v == 1.0 * j / (10.0 + 3.0 * k + 1e-6)


def test_snap_window_cases():
    names = [n for n, _, _ in rg.pool()]
    assert sum(n.startswith('win_') for n in names) == 18 and sum(n.startswith('axis_') for n in names) == 5
    sides = set()
    for name, xs, k in rg.pool():
        assert rg.snap_margin(xs) >= 1e-9, name                           # no pool box on the threshold, random ones included
        ry, sn, cs = ref.box_yaw(xs[0], xs[1])
        _, sn0, cs0 = ref.box_yaw(xs[0], xs[1], snap=False)
        small = min(abs(sn0), abs(cs0))
        if name.startswith('win_'):
            size = float(name.rsplit('_', 1)[1])
            assert abs(small - size) < 1e-12, (name, small)
            assert (min(abs(sn), abs(cs)) == 0.0) == (size < 1e-3), name
            if size < 1e-3:
                moved = rg.snap_moves(xs, rg.KS[k])
                assert moved > 1e-3, (name, moved)                        # a missing snap cannot pass at the bar
                assert moved > 100 * (RTOL * 2000 + ATOL)
            else:
                assert rg.snap_moves(xs, rg.KS[k]) == 0.0
            if not name.startswith('win_nonunit'):
                sides.add((name.split('_')[1], name.split('_')[2], abs(sn0) < abs(cs0)))
        if name.startswith('axis_'):
            assert small < 1e-15 and min(abs(sn), abs(cs)) == 0.0 and max(abs(sn), abs(cs)) == 1.0
    assert len(sides) == 8                                               # four axis directions, both sides
    assert {s[2] for s in sides} == {True, False}                         # the sine is the small one, and the cosine
    nonunit = rg.pool()[rg.pool_index('win_nonunit_0.0009')][1]
    assert abs(math.hypot(nonunit[0], nonunit[1]) - 3.7) < 1e-12


def pattern(a):
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 2, np.where(np.isinf(a), np.sign(a) * 3, 0)).astype(np.int8)


def test_depth_cases():
    p = rg.pool()
    xs = p[rg.pool_index('far_corners_in_front')][1]
    assert xs[7] < 0 < xs[7] + xs[4] / 2 and xs[0] == 0                   # centre behind, the far face in front
    proj, rect = ref.project_box(xs, rg.K_PLAIN)
    assert np.isfinite(proj).all() and rect[0] < 0 < rect[2]
    xs = p[rg.pool_index('centre_behind')][1]
    assert xs[7] + math.hypot(xs[2], xs[4]) / 2 < 0                       # every corner behind
    assert np.isfinite(ref.project_box(xs, rg.K_PLAIN)[0]).all()
    for name, u in (('zero_size_inf', -math.inf), ('zero_size_nan', math.nan)):
        _, xs, k = p[rg.pool_index(name)]
        assert xs[2:5] == (0.0, 0.0, 0.0) and xs[7] + 1e-6 == 0.0
        proj, rect = ref.project_box(xs, rg.KS[k])
        assert pattern(proj).tolist() == [[pattern(u).item(), 3]] * 9 and pattern(rect).tolist() == [pattern(u).item(), 3] * 2
        row = ref.kitti_row([0.0] * 32, xs, rg.KS[k], rg.CLIP_FRAME)
        assert row[2:6] == [0.0, 299.0, 0.0, 299.0]                       # -inf and NaN clip to 0, +inf to h - 1
    # under the K with a full third row the same point is finite
    assert np.isfinite(ref.project_box(p[rg.pool_index('zero_size_inf')][1], rg.K_SKEW)[0]).all()
    assert rg.K_SKEW[1] != 0 and rg.K_SKEW[3] != 0 and rg.K_SKEW[6:] != [0.0, 0.0, 1.0]
    assert ref.fmin(math.nan, 1.0) == 1.0 == ref.fmax(1.0, math.nan) and math.isnan(ref.fmin(math.nan, math.nan))


def test_project_cases_reach_the_regimes_of_the_kernel():
    assert [rg.project_case(n)['N'] for n in rg.PROJECT_NAMES[:6]] == [1, 7, 8, 28, 29, 57]
    assert 7 * 9 <= 63 < 64 <= 7 * 9 + 8 and 28 * 9 <= 255 < 256 <= 28 * 9 + 8       # slots 7 and 28 straddle a wave / block boundary
    for name in rg.PROJECT_NAMES:
        c = rg.project_case(name)
        proj, rect = ref.project_boxes(c['x'], c['status'], c['K'], c['topk'])
        dead = c['status'] < 0
        assert not proj[dead].any() and not rect[dead].any()
        if name.endswith('_unsolved'):
            assert np.flatnonzero(dead).tolist() == sorted({0, 28, c['N'] - 1})
        else:
            assert not dead.any()
        live = ~dead
        assert (np.abs(np.nan_to_num(proj[live], nan=1.0, posinf=1.0, neginf=1.0)).sum((1, 2)) > 0).all()
    c = rg.project_case('b3k19')
    assert c['topk'] == 19 and c['K'].shape == (3, 9) and len({bits(k) for k in c['K']}) == 3
    one = rg.project_case('n57')
    assert one['topk'] == 0 and one['K'].shape == (57, 9) and bits(one['x']) == bits(c['x'])
    # one K per image is not one K per slot: the two layouts disagree on the same boxes
    a, b = ref.project_boxes(c['x'], c['status'], c['K'], 19)[0], ref.project_boxes(one['x'], one['status'], one['K'], 0)[0]
    assert (np.nan_to_num(a) != np.nan_to_num(b)).any(axis=(1, 2)).sum() >= 19


# ------------------------------------------------------------------------------------------------ 3. frames_adjust_K
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    from rtm3d_amd import _lib
    return _lib.load()


def test_geometries_are_those_of_frame_geometry(lib):
    for spec, want in zip(rg.GEOM_SPECS, rg.GEOMS):
        g = preprocess.frame_geometry([spec[:2]], rg.CANVAS, spec[2])[0]
        assert (g.h, g.w, g.rh, g.rw, g.pad_w, g.pad_h) == want
    assert rg.GEOM_SPECS[:5] == [(128, 256, None), (300, 1000, 256), (100, 201, None), (101, 223, None), (500, 300, 128)]
    assert rg.GEOMS[5][:2] == (1, 1) and rg.GEOMS[6][1] == 8192 and rg.GEOMS[6][3] < 8192


@pytest.mark.parametrize('B', rg.ADJUST_B)
def test_k_net_yardstick_equals_resize_K_and_adjust_K(B):
    c = rg.adjust_case(B)
    assert len(c['geoms']) == B and (B < 7 or set(c['geoms']) == set(rg.GEOMS))
    for b, g in enumerate(c['geoms']):
        want = preprocess.adjust_K(preprocess.resize_K(c['K'][b], (g[0], g[1]), (g[2], g[3])), g[4], g[5])[0]
        got = np.array(ref.k_net(c['K'][b], g))
        assert bits(got) == bits(want)
        assert bits(got[6:]) == bits(c['K'][b, 6:]) and (g[:2] == g[2:4] or (got[:6] != c['K'][b, :6]).any())
    assert rg.ADJUST_B == [1, 28, 29, 64, 65, 130] and 28 * 9 <= 256 < 29 * 9 == 261


# ------------------------------------------------------------------------------------------------ 4. records_to_camera
def to_camera_numpy(rec, geoms):
    out = rec.copy()
    for b, g in enumerate(geoms):
        live = rec[b, :, 31] >= 1
        v = rec[b][:, 2:24].astype(np.float64)
        v[:, 0::2] = (v[:, 0::2] - g[4]) * (np.float64(g[1]) / np.float64(g[3]))
        v[:, 1::2] = (v[:, 1::2] - g[5]) * (np.float64(g[0]) / np.float64(g[2]))
        out[b][live, 2:24] = v.astype(np.float32)[live]
    return out


def host_rows(c, clip=True):
    """kitti_results.kitti_label_values on the slots the yardstick keeps."""
    B, topk = c['B'], c['topk']
    rows = np.zeros((B, topk, 16))
    for b, g in enumerate(c['geoms']):
        for r in range(topk):
            s = b * topk + r
            if not ref.kept(c['rec'][b, r, 31], c['status'][s], c['fun'][s], c['fun_accept']):
                continue
            xs = c['x'][s]
            params = {'class': c['rec'][b, r, :1].astype(np.int64), 'Ry': np.arctan2(xs[:1], xs[1:2]), 'dimension': xs[None, [3, 4, 2]],
                      'location': xs[None, 5:8], 'K': c['K'][b][None], 'score': c['rec'][b, r, 1:2].astype(np.float64)}
            rows[b, r, :14] = kr.kitti_label_values(params, image_size=(g[1], g[0]) if clip else None)[0]
            rows[b, r, 14] = 2.0
    return rows


@pytest.mark.parametrize('name', rg.CAMERA_NAMES)
def test_camera_yardstick_equals_the_host_forms(name):
    c = rg.camera_case(name)
    got = ref.to_camera(c['rec'], c['geoms'])
    assert bits(got) == bits(to_camera_numpy(c['rec'], c['geoms']))
    live = c['rec'][..., 31] >= 1
    assert bits(got[~live]) == bits(c['rec'][~live]) and bits(got[..., :2]) == bits(c['rec'][..., :2]) and bits(got[..., 24:]) == bits(c['rec'][..., 24:])
    rows = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'])
    assert bits(rows) == bits(ref.kitti_rows(got, c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept']))   # canvas or camera records
    with np.errstate(invalid='ignore', divide='ignore'):
        want = host_rows(c)
    finite = np.isfinite(want).all(-1)                                    # numpy's clip keeps the NaN the device's fmax drops
    assert finite.sum() >= finite.size - 3
    np.testing.assert_allclose(rows[finite], want[finite], rtol=RTOL, atol=ATOL)
    keptm = rows[..., 14] == 2
    assert not rows[~keptm].any() and keptm.any() and np.isfinite(rows).all()
    for k in (0, 6, 7, 8, 9, 10, 11, 13, 14, 15):
        assert bits(rows[..., k][finite]) == bits(want[..., k][finite]), k
    assert rg.clip_margin(c) >= 1e-3, (name, rg.clip_margin(c))            # no unclipped coordinate on a clip limit


def wave_orders(flag):
    """{(first half has a row, second half has a row)} over the waves (flat slots 2m, 2m + 1) of one launch chunk."""
    f = (np.asarray(flag).reshape(-1) == 2).tolist()
    return {(f[i], f[i + 1]) for i in range(0, len(f) - 1, 2)}


def test_camera_cases_reach_the_regimes_of_the_kernel():
    assert [(c['B'], c['topk']) for c in map(rg.camera_case, rg.CAMERA_NAMES[:5])] == [(1, 1), (1, 3), (64, 1), (65, 8), (130, 3)]
    assert 1 * 3 * 32 == 96 and 65 > 64 and 130 > 2 * 64
    for name in rg.CAMERA_NAMES[2:5] + ['kept_rule']:
        c = rg.camera_case(name)
        assert wave_orders(c['rec'][..., 31]) >= {(True, False), (False, True)}, name
        assert set(c['rec'][..., 31].ravel().tolist()) == {0.0, 1.0, 2.0}
    for name in rg.CAMERA_NAMES[:5]:
        c = rg.camera_case(name)
        assert not c['rec'][c['rec'][..., 31] == 0].any()                 # empty slots are 32 zeros
        assert len(set(c['geoms'])) == min(c['B'], len(rg.GEOMS))


def test_kept_rule_case():
    c = rg.camera_case('kept_rule')
    rows = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'])
    assert np.array_equal(rows[..., 14] == 2, c['want_row']) and c['want_row'].sum() == 2 * 5
    flag, status, fun = c['rec'][0, :, 31], c['status'][:c['topk']], c['fun'][:c['topk']]
    with np.errstate(invalid='ignore'):
        small = fun < c['fun_accept']
    assert ((flag == 1) & (status >= 0) & small).sum() >= 2               # what NMS leaves: no row
    assert ((flag == 2) & ~small).sum() >= 4 and ((flag == 2) & (status < 0)).sum() >= 1          # inconsistent input: no row
    assert ((flag == 0) & (status >= 0) & small).sum() >= 1
    empty = c['rec'][flag[None, :].repeat(2, 0) == 0]
    assert (empty[:, :31] != 0).all()                                     # garbage, which stays
    assert bits(ref.to_camera(c['rec'], c['geoms'])[c['rec'][..., 31] == 0]) == bits(empty)
    # the rule before this suite (flag >= 1) writes other rows on this case: the case tells the two apart
    old = (c['rec'][..., 31] >= 1) & (c['status'].reshape(2, -1) >= 0) & np.tile(small, 2).reshape(2, -1)
    assert (old & ~c['want_row']).sum() == 2 * 2


def test_alpha_case():
    c = rg.camera_case('alpha')
    rows = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'])[0]
    un = np.array([ref.unwrapped_alpha(xs) for xs in c['x']])
    n = len(c['want_alpha'])
    assert np.abs(un[:n] - c['want_alpha']).max() < 1e-12
    assert math.pi < un[0] < 2 * math.pi and math.pi < un[1] < 2 * math.pi and -2 * math.pi < un[2] < -math.pi and -2 * math.pi < un[3] < -math.pi
    near = np.abs(np.abs(un[4:n]) - math.pi)
    assert (near <= 1e-3).all() and (near >= 1e-6).all()
    assert {(u > 0, abs(u) > math.pi) for u in un[4:n]} == {(True, True), (True, False), (False, True), (False, False)}
    assert (rows[:, 1] >= -math.pi).all() and (rows[:, 1] < math.pi).all()
    for k in range(n):
        m = round((un[k] - rows[k, 1]) / (2 * math.pi))
        assert abs(rows[k, 1] + 2 * math.pi * m - un[k]) < 1e-12 and (m != 0) == (not -math.pi <= un[k] < math.pi)
    # the exact cases: X = 0 and ry = +-pi from (+-0, -1) both give -pi exactly
    assert c['x'][n:, 5].tolist() == [0.0, 0.0] and rows[n:, 12].tolist() == [math.pi, -math.pi]
    assert rows[n:, 1].tolist() == [-math.pi, -math.pi]


def test_clip_case():
    c = rg.camera_case('clip')
    rows = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'])
    un = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'], clip=False)
    w, h = 1000, 300
    left, right, cut_left, cut_all, inside = (rows[0, k, 2:6] for k in range(5))
    assert c['kinds'] == ('left', 'right', 'cut_left', 'cut_all', 'inside')
    assert left[0] == left[2] == 0.0 and un[0, 0, 4] < 0
    assert right[0] == right[2] == w - 1 and un[0, 1, 2] > w - 1
    assert cut_left[0] == 0.0 and un[0, 2, 2] < 0 < cut_left[2] == un[0, 2, 4] < w - 1 and bits(cut_left[[1, 3]]) == bits(un[0, 2, [3, 5]])
    assert cut_all.tolist() == [0.0, 0.0, w - 1.0, h - 1.0] and un[0, 3, 2] < 0 and un[0, 3, 3] < 0 and un[0, 3, 4] > w - 1 and un[0, 3, 5] > h - 1
    assert bits(inside) == bits(un[0, 4, 2:6])
    assert c['geoms'][1][:2] == (1, 1) and not rows[1, :, 2:6].any() and (rows[1, :, 14] == 2).all()


def test_pool_case_holds_every_box_under_every_K():
    c = rg.camera_case('pool')
    assert c['B'] == 3 and c['topk'] == len(rg.pool()) and bits(c['K']) == bits(np.array(rg.KS))
    rows = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'])
    assert (rows[..., 14] == 2).all() and np.isfinite(rows).all()
    un = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'], clip=False)
    z = rg.pool_index('zero_size_nan')
    assert pattern(un[0, z, 2:6]).tolist() == [-3, 3, -3, 3] and pattern(un[2, z, 2:6]).tolist() == [2, 3, 2, 3] and np.isfinite(un[1, z]).all()
    # a missing snap shows in the rows too
    plain = ref.kitti_rows(c['rec'], c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'], snap=False)
    for name, _, _ in rg.pool():
        if name.startswith('win_') and name.endswith('0.0009'):
            k = rg.pool_index(name)
            assert np.abs(plain[0, k, 2:6] - rows[0, k, 2:6]).max() > 1e-3, name


# ------------------------------------------------------------------------------------------------ 5. NMS and the rows
def test_nms_order_case_suppresses_a_slot():
    c = rg.nms_order_case()
    went = 0
    after = c['rec'].copy()
    for b in range(c['B']):
        bev, _ = box_overlap_ref.record_ious(c['rec'][b])
        m = bev[np.triu_indices(c['topk'], 1)]
        assert np.abs(m - rg.NMS_THRESH).min() > 0.2                      # no pair near the threshold
        flags = box_overlap_ref.nms_flags(c['rec'][b], rg.NMS_THRESH, bev)
        assert flags.tolist() == [2, 1, 2, 2, 1, 2]
        after[b, :, 31] = flags
        went += int((flags == 1).sum())
        assert (np.diff(c['rec'][b, :, 1]) < 0).all()                      # score order
    assert went == 4
    args = (c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'])
    before, rows = ref.kitti_rows(c['rec'], *args), ref.kitti_rows(after, *args)
    assert (before[..., 14] == 2).all() and ((rows[..., 14] == 2) == (after[..., 31] == 2)).all()
    assert not rows[after[..., 31] == 1].any() and bits(rows[after[..., 31] == 2]) == bits(before[after[..., 31] == 2])
