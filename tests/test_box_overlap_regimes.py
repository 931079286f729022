"""CPU: the exact yardstick of tests/box_overlap_regimes.py against closed forms, against the float yardstick
(tests/box_overlap_ref.py; this defines YARD_ERR and the bar of the GPU test) and against a host restatement of box_geom.h; the
pair set really is in the regimes of box_overlaps_kernel it claims (vertex counts 3 .. 8, pairs emptied at each clip stage,
touching polygons, near-parallel edges, no fragile pair); the constructed NMS cases really give the flags they expect (host model
of records_nms3d_kernel, and the yardstick's record_ious / nms_flags on the small cases and a sample of the large ones); and
deliberately wrong variants of the two host models disagree on the cases that are there to tell them apart.  No device is used,
and nothing broken is built for one: the variants exist in the host models only.

Measured here: YARD_ERR 2.58e-13 (the float yardstick clips in world coordinates: its worst pairs are boxes of 0.3 m some 50 m
from the origin), so the bar is 16 x YARD_ERR = 4.13e-12; the restatement of box_geom.h is within 1.2e-15 of the exact yardstick."""
import collections
from fractions import Fraction as F

import numpy as np
import pytest

from tests import box_overlap_ref as ref
from tests import box_overlap_cases as cases
from tests import box_overlap_regimes as rg

ABS_TOL = 1e-9           # the ceiling of tests/test_gpu_box_overlap.py
CLOSED_FORM_TOL = 2e-14  # degenerate_cases() places b with fp64 sums (two ulps of 17 m = 7e-15 m on edges of 4 m over an area of 8 m^2)


@pytest.fixture(scope='module')
def ps():
    return rg.pair_set()


@pytest.fixture(scope='module')
def yard():
    return rg.yardstick()


def pool(ps, name):
    return np.flatnonzero(ps['pool'] == name)


# ------------------------------------------------------------------------------------------------ 1. the exact yardstick
def test_exact_yardstick_equals_the_closed_forms():
    for name, a, b, bev, vol in cases.degenerate_cases():
        for x, y in ((a, b), (b, a)):
            (gb, gv), nv = rg.exact_overlap(x, y)
            assert abs(gb - bev) <= CLOSED_FORM_TOL and abs(gv - vol) <= CLOSED_FORM_TOL, (name, gb, gv)
            assert nv >= 3 or bev == 0, (name, nv)              # (a rounded centre may leave a sliver where the closed form is 0)
    a = np.array([1.5, 2.0, 4.0, 3.0, 1.0, 17.0, 0.0])
    b = np.array([3.0, 2.0, 4.0, 5.0, 1.75, 18.0, 0.0])              # ry = 0: everything is exact
    assert rg.exact_pair(a, b)[:6] == (F(2), F(3, 2), F(8), F(8), 4, 2)
    assert rg.exact_overlap(a, b, 'iou') == ((2 / 14, 3 / 33), 4) and rg.exact_overlap(a, b, 'a') == ((0.25, 0.25), 4)
    assert rg.exact_overlap(a, b, 'b') == ((0.25, 0.125), 4)
    ok, bad = cases.invalid_boxes()
    for x in bad:
        for crit in rg.CRITERIA:
            assert rg.exact_overlap(ok, x, crit) == ((0.0, 0.0), 0) and rg.exact_overlap(x, ok, crit) == ((0.0, 0.0), 0)


def test_yard_err_and_the_bar(ps, yard):
    """YARD_ERR: the float yardstick against the exact one over the whole set (every criterion, BEV and 3D, boxes within 64 m of
    the origin).  The bar of the device test follows from it and stays under the existing ceiling."""
    assert len(ps['a']) <= 2500
    assert max(np.abs(ps['a'][:, [3, 5]]).max(), np.abs(ps['b'][:, [3, 5]]).max()) <= 64.0
    err = max(float(np.abs(yard['float'][c] - yard['exact'][c]).max()) for c in rg.CRITERIA)
    assert err == yard['yard_err']
    print('YARD_ERR %.3g over %d pairs, bar %.3g' % (err, len(ps['a']), rg.bar()))
    assert 0 < err <= 1e-11                                           # a float yardstick worse than this judges nothing
    assert rg.bar() == max(16 * err, 1e-13) <= ABS_TOL
    small = [k for k in pool(ps, 'concentric')]
    area = max(abs(ref.pair(ps['a'][k], ps['b'][k])[0] - float(rg.exact_pair(ps['a'][k], ps['b'][k])[0])) for k in small[:40])
    assert area <= 1e-12, area


def test_restatement_of_box_geom_is_within_the_bar(ps, yard):
    """The fp64 operation sequence of box_geom.h against the exact yardstick on the whole set, near-parallel edges included:
    what the device may be expected to reach.  Its final vertex count is the exact one on every pair that is not fragile."""
    worst = 0.0
    for k in range(len(ps['a'])):
        for c in rg.CRITERIA:
            got = rg.model_overlap(ps['a'][k], ps['b'][k], c)
            worst = max(worst, abs(got[0] - yard['exact'][c][k, 0]), abs(got[1] - yard['exact'][c][k, 1]))
        if ps['pool'][k] in rg.RANDOM_POOLS:
            assert got[2] == yard['nv'][k], (k, ps['pool'][k], got[2], yard['nv'][k])
    print('restatement of box_geom.h against the exact yardstick: %.3g' % worst)
    assert worst <= 1e-13 <= rg.bar()


def test_exact_yardstick_does_not_see_the_distance_from_the_origin(ps):
    """On the lattice pool a translation by 2^20 m is exact in fp64; the exact yardstick gives the SAME rationals."""
    for k in pool(ps, 'lattice')[:24]:
        a, b = ps['a'][k].copy(), ps['b'][k].copy()
        base = rg.exact_pair(a, b)
        a[3:6] += 2.0 ** 20
        b[3:6] += 2.0 ** 20
        assert rg.exact_pair(a, b) == base


# ------------------------------------------------------------------------------------------------ 2. the regimes of the pair set
def test_vertex_counts(ps, yard):
    count = collections.Counter(yard['nv'].tolist())
    print('distinct vertices of the intersection polygon: %s' % sorted(count.items()))
    for n in (3, 4, 5, 6, 7, 8):
        assert count[n] >= 16, (n, count)
    assert int(((yard['nv'] == 8) & (yard['new'] == 8)).sum()) >= 16
    assert set(yard['nv'].tolist()) <= set(range(9))
    # neighbouring lanes of the B = npairs launch hold polygons of different sizes
    changes = int((np.diff(yard['nv']) != 0).sum())
    assert changes >= 150, changes


@pytest.mark.parametrize('face', ['+x', '-x', '+z', '-z'])
def test_pairs_emptied_at_each_clip_stage(ps, yard, face):
    idx = pool(ps, 'beyond' + face)
    assert len(idx) >= 8
    stage = ['+x', '-x', '+z', '-z'].index(face)
    for k in idx:
        a, b = ps['a'][k], ps['b'][k]
        hl, hw = F(float(b[2])) / 2, F(float(b[1])) / 2
        pts = rg.in_frame_of(a, b)
        beyond = {'+x': [p[0] > hl for p in pts], '-x': [p[0] < -hl for p in pts], '+z': [p[1] > hw for p in pts], '-z': [p[1] < -hw for p in pts]}[face]
        assert all(beyond), (face, k)
        stages = []
        assert rg.model_overlap(a, b, stages=stages)[:2] == (0.0, 0.0)
        assert len(stages) == stage + 1 and stages[-1] == 0 and all(n > 0 for n in stages[:-1]), (face, k, stages)
        assert yard['nv'][k] == 0 and not yard['exact']['iou'][k].any()
        assert ref.valid(a) and ref.valid(b) and not rg._far_apart(a, b)


def test_touching_pairs_are_exact(ps, yard):
    for kind, n in (('corner', 1), ('edge', 2)):
        idx = pool(ps, 'touch_' + kind)
        assert len(idx) >= 4
        for k in idx:
            a, b = ps['a'][k], ps['b'][k]
            assert a[6] == 0 and b[6] == 0
            for box in (a, b):
                half = np.array([box[2] / 2, box[1] / 2, box[3], box[5]]) / rg.LATTICE * 4
                assert (half == np.round(half)).all() and np.abs(box[3:6]).max() <= 64
            assert yard['nv'][k] == n and not yard['exact']['iou'][k].any()
            assert rg.model_overlap(a, b)[:2] == (0.0, 0.0) and rg.model_overlap(b, a)[:2] == (0.0, 0.0)     # coincident vertices or none
            assert ps['want_bev'][k] == 0 and ps['want_vol'][k] == 0
    closed = pool(ps, 'closed_form')
    assert len(closed) == len(cases.degenerate_cases()) and np.isfinite(ps['want_bev'][closed]).all()
    assert int(np.isnan(ps['want_bev']).sum()) == len(ps['a']) - len(closed) - 12


@pytest.mark.parametrize('eps', rg.NEAR_ANGLES)
def test_near_parallel_pairs(ps, yard, eps):
    idx = pool(ps, 'near%g' % eps)
    assert len(idx) >= 16
    turns = set()
    for k in idx:
        a, b = ps['a'][k], ps['b'][k]
        ang = rg.edge_angle(a, b)
        assert F(eps) / 2 <= ang <= 2 * F(eps), (eps, float(ang))
        q = int(round((a[6] - b[6]) / (np.pi / 2)))
        turns.add(q % 4)
        la, wa = (a[2], a[1]) if q % 2 == 0 else (a[1], a[2])          # a's extents along b's axes
        assert 0.7 <= la / b[2] <= 1.3 and 0.7 <= wa / b[1] <= 1.3 and 0.7 <= a[0] / b[0] <= 1.3
        assert np.hypot(a[3] - b[3], a[5] - b[5]) > 1e-3                 # offset centres
        assert yard['exact']['iou'][k, 0] > 0.05 and yard['nv'][k] == 4
    assert len(turns) >= 3, turns                                        # on top of the quarter turns


def test_no_fragile_pair_in_the_random_part(ps):
    idx = [k for k in range(len(ps['a'])) if ps['pool'][k] in rg.RANDOM_POOLS]
    assert len(idx) == sum(n for _, n in rg.POOLS) == len(ps['a']) - 12 - len(cases.degenerate_cases())    # nothing left out
    fragile = [k for k in idx if not rg.clearance_ok(ps['a'][k], ps['b'][k])]
    assert fragile == []
    assert not rg.clearance_ok(*cases.degenerate_cases()[0][1:3])        # the check itself sees an identical pair


def test_lattice_pool_translates_and_scales_exactly(ps, yard):
    idx = pool(ps, 'lattice')
    assert len(idx) >= 64
    T = 2.0 ** 20
    for k in idx:
        for box in (ps['a'][k], ps['b'][k]):
            v = box[[0, 3, 4, 5]] / rg.LATTICE
            assert (v == np.round(v)).all() and np.abs(box[3:6]).max() <= 64
            moved = box[3:6] + T
            assert all(F(float(m)) == F(float(x)) + F(T) for m, x in zip(moved, box[3:6]))       # every sum is exact
    assert set(yard['nv'][idx].tolist()) >= {7, 8}
    big = np.abs(np.concatenate([ps['a'][:, :6], ps['b'][:, :6]])).ravel()
    assert big.max() * 2.0 ** 20 < 1e300 and big[big > 0].min() * 2.0 ** -20 > 1e-300


def test_wrong_clips_are_caught(ps, yard):
    """A clip that caps the polygon at 7 vertices against the exact yardstick and the bar."""
    bar = rg.bar()

    def off(k, **kw):
        got = rg.model_overlap(ps['a'][k], ps['b'][k], **kw)
        return max(abs(got[0] - yard['exact']['iou'][k, 0]), abs(got[1] - yard['exact']['iou'][k, 1]))
    oct8 = np.flatnonzero(yard['nv'] == 8)
    assert all(off(k) <= bar for k in oct8)
    capped = [k for k in oct8 if off(k, maxv=7) > 1e3 * bar]
    print('a polygon capped at 7 vertices: %d of %d octagons are off by more than 1000 bars' % (len(capped), len(oct8)))
    assert len(capped) >= 16
    assert all(off(k, maxv=7) <= bar for k in np.flatnonzero(yard['nv'] <= 6))        # and nothing else tells it apart


def test_open_inside_tests_cannot_show_in_an_area(ps, yard):
    """A clip with OPEN inside tests (`> 0` for `>= 0`) differs from the closed one only in vertices that lie exactly on a clip
    line: it leaves them out and puts the crossing point - the same point - in their place, or drops a polygon that has no
    interior.  The area is the same rational number, so no overlap value can tell the two clips apart; what this test pins is
    exactly that: equal exact areas, other vertex lists, and a host restatement with open tests that stays within the bar."""
    differ = 0
    for k in np.concatenate([pool(ps, 'touch_corner'), pool(ps, 'touch_edge'), pool(ps, 'closed_form'), pool(ps, 'lattice')[:8]]):
        c, o = rg.exact_pair(ps['a'][k], ps['b'][k]), rg.exact_pair(ps['a'][k], ps['b'][k], closed=False)
        assert c[:4] == o[:4]
        differ += c[4] != o[4]
    assert differ >= 12                                                  # every touching pair: 1 or 2 vertices against none
    worst = 0.0
    for k in range(len(ps['a'])):
        got = rg.model_overlap(ps['a'][k], ps['b'][k], closed=False)
        worst = max(worst, abs(got[0] - yard['exact']['iou'][k, 0]), abs(got[1] - yard['exact']['iou'][k, 1]))
    assert worst <= rg.bar()


def test_layouts(ps):
    P, Q = rg.layout_boxes()
    totals = []
    for B, ca, cb in rg.LAYOUTS:
        A, Bx, na, nb = rg.layout(B, ca, cb)
        assert A.shape == (B, ca, 7) and Bx.shape == (B, cb, 7) and ca != cb and na.shape == nb.shape == (B,)
        assert (na <= ca).all() and (nb <= cb).all()
        totals.append(B * ca * cb)
        if B > 1:
            assert 0 in na.tolist() + nb.tolist() and ca in na.tolist() and cb in nb.tolist() and any(0 < n < ca for n in na.tolist() + nb.tolist())
    assert totals == [195, 195, 585, 300, 768] and 300 % 256 and 195 < 256 and 768 == 3 * 256
    a1, b1 = rg.layout(3, 5, 13)[:2]
    a2, b2 = rg.layout(3, 13, 5)[:2]
    assert np.array_equal(a1, b2) and np.array_equal(b1, a2) and np.array_equal(rg.layout(1, 15, 39)[0][0], P.reshape(15, 7))
    nv = collections.Counter(rg.exact_cached(P[m, i], Q[m, j])[4] for m in range(3) for i in range(5) for j in range(13))
    print('layouts: vertex counts of the 195 pairs %s' % sorted(nv.items()))
    assert sum(n for v, n in nv.items() if v >= 3) >= 150 and len([v for v in nv if v >= 3]) >= 5
    for m in range(3):                                                   # pairs across sites cannot meet
        for n in range(3):
            if m != n:
                assert all(rg._far_apart(p, q) for p in P[m] for q in Q[n])


def test_extremes_on_the_host_model():
    boxes, invalid = rg.extreme_boxes()
    assert invalid.sum() == 5 and (~invalid).sum() >= 12
    assert (boxes[:, :3] >= 1e199).all(axis=1).sum() >= 5 and np.abs(boxes[~invalid, 6]).max() == 1e6
    with np.errstate(over='ignore'):
        assert np.isinf(boxes[:, 1] * boxes[:, 2]).sum() >= 5                # footprint areas that overflow
    for crit in rg.CRITERIA:
        for i, a in enumerate(boxes):
            for j, b in enumerate(boxes):
                bev, vol, _ = rg.model_overlap(a, b, crit)
                assert np.isfinite(bev) and np.isfinite(vol) and 0.0 <= bev <= 1 + 1e-12 and 0.0 <= vol <= 1 + 1e-12, (crit, i, j, bev, vol)
                if invalid[i] or invalid[j]:
                    assert bev == 0.0 and vol == 0.0


# ------------------------------------------------------------------------------------------------ 3. the NMS cases
def sample(case):
    """Every image of a small case; four images of a large one."""
    B, topk = case['rec'].shape[:2]
    return list(range(B)) if B * topk * topk <= 20000 else sorted({0, B // 4, B // 2, B - 1})


@pytest.mark.parametrize('nc', [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 128, 255, 256])
def test_schedule_visits_every_pair_once(nc):
    seen = rg.visits(nc)
    assert len(seen) == nc * (nc - 1) // 2 == len(set(seen)) and all(0 <= lo < hi < nc for lo, hi in seen)
    if nc >= 2 and nc % 2 == 0:
        assert len(set(rg.visits(nc, 'no_half_round'))) == len(seen) - nc // 2
    if nc >= 3:
        assert len(set(rg.visits(nc, 'no_wrap'))) < len(seen)
    rounds = rg.one_factorisation(nc)
    flat = [p for r in rounds for p in r]
    assert sorted(flat) == sorted(seen) and len(rounds) == nc - 1 + nc % 2
    for r in rounds:
        members = [k for p in r for k in p]
        assert len(set(members)) == len(members) == (nc // 2) * 2        # disjoint pairs; one bye for an odd count


def test_every_regime_of_the_nms_has_a_case():
    names = set(rg.NMS_NAMES)
    assert {'every_pair_nc%d_%s' % (nc, m) for nc in (2, 4, 8, 64, 256, 3, 7, 65, 255) for m in ('bev', '3d')} <= names
    assert {'counts_topk%d' % t for t in (1, 63, 64, 65, 255, 256)} <= names
    for name in ('every_pair_nc256_bev', 'every_pair_nc255_3d'):
        c = rg.nms_case(name)
        nc = c['nc']
        assert c['rec'].shape == (nc - 1 + nc % 2, nc, 32) and c['rec'].nbytes <= 8.5e6
        planted = [p for r in c['rounds'] for p in r]
        assert sorted(planted) == [(i, j) for i in range(nc) for j in range(i + 1, nc)]          # every bit of every word of every row
        assert {lo >> 5 for lo, _ in planted} == set(range(8))
    ncs = {(c['rec'].shape[1], nc) for t in rg.COUNT_TOPK for c in [rg.nms_case('counts_topk%d' % t)] for nc, first in c['spreads'] if not first}
    assert {nc for _, nc in ncs} == set(rg.COUNT_NC) and {(256, 256), (256, 255), (255, 255), (1, 1), (1, 0), (65, 65), (64, 64), (63, 63)} <= ncs
    c = rg.nms_case('counts_topk256')
    flags = c['rec'][..., 31]
    assert all((flags == v).any() for v in (np.float32(2.0000002), 3, -2, 0, 1)) and np.isnan(flags).any()
    assert np.float32(2.0000002) != np.float32(2.0)
    for m, (nc, first) in enumerate(c['spreads']):
        assert int((flags[m] == 2).sum()) == nc and not (flags[m, :first] == 2).any()
    assert (192 in [f for _, f in c['spreads']])
    for name in ('line_d1_interleaved_bev', 'line_d0.6_interleaved_bev'):
        c = rg.nms_case(name)
        assert len(c['slots']) == 128 and c['rec'].shape[1] == 256 and c['slots'] != list(range(128))
        other = np.delete(c['rec'][0, :, 31], c['slots'])
        assert set(other.tolist()) == {0.0, 1.0}
    assert abs(rg._line_iou(1, 1.0) - 0.6) < 1e-15 and abs(rg._line_iou(2, 1.0) - 1 / 3) < 1e-15
    assert rg._line_iou(1, 0.6) > 0.73 and 0.53 < rg._line_iou(2, 0.6) < 0.54 and 0.37 < rg._line_iou(3, 0.6) < 0.38


@pytest.mark.parametrize('name', rg.NMS_NAMES)
def test_nms_case_is_sound(name):
    """Lattice, expected flags against the host model and (on a sample of the large cases) against the float yardstick's own
    IoUs and greedy NMS."""
    c = rg.nms_case(name)
    rec, want = c['rec'], c['want']
    B, topk = rec.shape[:2]
    assert rec.dtype == np.float32 and rec.shape[2] == 32 and 1 <= topk <= 256 and want.shape == (B, topk)
    assert np.hypot(rg.NMS_BOX[1], rg.NMS_BOX[2]) < rg.PITCH
    changed = (want != rec[..., 31]) & ~(np.isnan(want) & np.isnan(rec[..., 31]))
    assert (rec[..., 31][changed] == 2).all() and (want[changed] == 1).all()
    images = sample(c)
    for b in images:
        model = rg.model_nms(rec[b], c['thresh'], c['ious'][b], c['aware'])
        assert model.tobytes() == want[b].tobytes(), (name, b)
    for b in images[:2] if topk > 65 else images:                        # the python pair loop over 256 slots: two images of a large case
        bev, vol = ref.record_ious(rec[b])
        ious = bev if c['metric'] == 'bev' else vol
        for (i, j), v in c['ious'][b].items():
            assert abs(ious[i, j] - v) <= 2e-5, (name, b, i, j, ious[i, j], v)     # fp32 centres: an ulp at 154 m is 1.5e-5 m, on 4 m
        assert int((ious > 0).sum()) == 2 * sum(v > 0 for v in c['ious'][b].values())             # only the planted pairs meet
        m = ious[np.triu_indices(topk, 1)]
        if np.isfinite(c['thresh']) and 0 < c['thresh'] < 1:
            assert np.abs(m[m > 0] - c['thresh']).min(initial=1.0) > 1e-3
        flags = ref.nms_flags(rec[b], c['thresh'], ious, class_aware=c['aware'])
        assert flags.tobytes() == want[b].tobytes(), (name, b)


def test_threshold_and_odd_cases_say_what_they_claim():
    rec, iou = rg.threshold_images()
    assert iou[(0, 1)] == 1.0 and iou[(2, 3)] == 0.0 and 0 < iou[(4, 5)] < 2e-4 and abs(iou[(6, 7)] - 1 / 3) < 1e-15
    bev = ref.record_ious(rec[0])[0]
    assert bev[2, 3] == 0.0 and bev[4, 5] > 0                           # touching is exactly 0, the overlap of 2^-10 m is not
    w = {n: rg.nms_case(n)['want'][0, :11].tolist() for n in rg.NMS_NAMES if n.startswith('thresh_')}
    assert w['thresh_0_blind'] == [2, 1, 2, 2, 2, 1, 2, 1, 2, 2, 2]       # touching stays, any positive overlap goes, invalid boxes stay
    assert w['thresh_1.5_blind'] == [2] * 11 == w['thresh_inf_blind'] == w['thresh_inf_aware']
    assert w['thresh_-1_blind'] == [2] + [1] * 10                        # only the first candidate, invalid boxes go too
    assert w['thresh_-1_aware'] == [2, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1]      # the first of each class
    for name in (n for n in rg.NMS_NAMES if n.startswith('odd_')):
        c = rg.nms_case(name)
        got = c['want'][0]
        invalid = [k for k in range(18) if not ref.valid(c['rec'][0, k, 24:31].astype(np.float64))]
        assert invalid == [1, 4, 7, 10, 13, 16] and (got[invalid] == 2).all() and c['thresh'] >= 0
        assert got[[5, 8, 11, 14, 17]].tolist() == [1] * 5 and got[2] == (2 if c['aware'] else 1)
        assert got[19] == (1 if c['metric'] == 'bev' else 2)             # equal footprints, disjoint vertical extents
        if c['aware']:
            assert np.isnan(c['rec'][0, 0, 0]) and np.isnan(c['rec'][0, 2, 0])


@pytest.mark.parametrize('topk', [100, 130])
def test_clustered_images_hold_a_pair_whose_own_iou_decides(topk):
    """What the GPU test of the threshold arithmetic needs from cases.nms_records, shown on the float yardstick's IoUs: a slot
    that stays at a threshold equal to its IoU with its suppressor and goes one float under it - which `>=` would get wrong."""
    rec = cases.nms_records(topk)[0]
    for metric, M in zip(('bev', '3d'), ref.record_ious(rec)):
        M = np.triu(M, 1)
        i, j = rg.strict_pair(rec, M, cases.NMS_THRESH[metric])
        iou = {(a, b): M[a, b] for a, b in np.argwhere(M > 0)}
        thr = float(M[j, i])
        assert rg.model_nms(rec, thr, iou)[i] == 2 and rg.model_nms(rec, thr, iou, variant='ge')[i] == 1
        assert rg.model_nms(rec, thr, iou).tobytes() == ref.nms_flags(rec, thr, M).tobytes()


# ------------------------------------------------------------------------------------------------ 4. wrong kernels
WRONG = {            # wrong variant of the host model -> the cases that must tell it from the expected flags
    'no_half_round': ['every_pair_nc%d_bev' % nc for nc in rg.EVEN_NC],                    # the last round of an even count not run
    'no_wrap': ['every_pair_nc%d_bev' % nc for nc in (4, 8, 64, 256) + rg.ODD_NC],         # a pair whose partner lies past nc - 1 dropped
    'rows4': ['every_pair_nc256_bev', 'every_pair_nc255_3d', 'line_d1_full_bev', 'line_d0.6_full_bev'],
    'non_survivors': ['line_d1_full_bev', 'line_d0.6_full_bev', 'line_d1_interleaved_bev', 'line_d0.6_interleaved_bev', 'line_d1_full_3d'],
    'ge': ['thresh_0_blind', 'thresh_0_aware', 'odd_bev_0_blind', 'odd_3d_0_blind'],       # >= for >
    'swapped': ['every_pair_nc2_bev', 'every_pair_nc3_3d', 'line_d1_full_bev', 'counts_topk64', 'thresh_-1_blind'],   # bit `later` in row `earlier`
}


@pytest.mark.parametrize('variant', rg.NMS_VARIANTS)
def test_wrong_nms_kernels_are_caught(variant):
    assert set(WRONG) == set(rg.NMS_VARIANTS)
    for name in WRONG[variant]:
        c = rg.nms_case(name)
        images = list(range(c['rec'].shape[0])) if c['rec'].shape[1] <= 65 else sample(c)
        off = [b for b in images if rg.model_nms(c['rec'][b], c['thresh'], c['ious'][b], c['aware'], variant).tobytes() != c['want'][b].tobytes()]
        print('%s: caught by %s in %d of %d images looked at' % (variant, name, len(off), len(images)))
        assert off, (variant, name)
        if name.startswith('every_pair') and variant in ('no_half_round', 'no_wrap') and c['rec'].shape[1] <= 65:
            missed = set(rg.visits(c['nc'])) - set(rg.visits(c['nc'], variant))
            assert sorted(p for b in off for p in c['rounds'][b] if p in missed) == sorted(missed)       # every missed pair shows
