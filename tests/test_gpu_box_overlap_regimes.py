"""GPU: rtm3d_box_overlaps and rtm3d_records_nms3d (csrc/box_overlap.hip on csrc/box_geom.h) in every regime of their kernels,
over the cases of tests/box_overlap_regimes.py.  tests/test_box_overlap_regimes.py asserts on the CPU that each case is in the
regime it is named for and that the cases tell wrong kernels from the right one.

box_overlaps_kernel against the EXACT yardstick (fractions.Fraction after numpy's fp64 cos / sin): one seeded set of pairs
launched as B = npairs, cap_a = cap_b = 1 - polygons of 3 .. 8 distinct vertices, pairs emptied at each of the four clips,
touching polygons, edges 1e-15 .. 1e-4 rad from parallel - for all three criteria and both outputs within
BAR = max(16 x YARD_ERR, 1e-13), YARD_ERR the float yardstick's own error against the exact one on this set; the closed forms
within 1e-12; then the same pairs in product layouts with cap_a != cap_b and ragged counts (bit-identical to the 1 x 1 launch),
one output NULL, exact translation by 2^20 m, exact scaling by 2^20 and 2^-20 (bit-identical), sizes of 1e200 / |ry| of 1e6 /
invalid boxes in one wave.

records_nms3d_kernel against flags that follow from the construction of each case: every pair of candidates planted exactly
once over the images of a 1-factorisation (nc = topk in 2 .. 256, even and odd, both metrics), lines of 256 and of 128
interleaved candidates that only survivors may thin, every nc in {0, 1, 2, 3, 63, 64, 65, 128, 255, 256} at topk in
{1, 63, 64, 65, 255, 256} with flags that are no candidates, thresholds 0, 1.5, -1 and +inf, invalid and NaN-class candidates,
and thresholds set to exactly the device's own IoU of a pair (the NMS runs the arithmetic of the overlap matrix, and is strict).

Measured on an MI355X (the figures the tests print; copied to profiles/box_overlap.txt): YARD_ERR 2.58e-13 (the float yardstick
against the exact one; its worst pairs are boxes of 0.3 m some 50 m from the origin), so BAR = 16 x YARD_ERR = 4.13e-12; the device
against the exact yardstick over the 710 pairs, three criteria, BEV and 3D: 1.11e-15 (criterion 'a', a pair of the general pool) -
the figure of the host restatement of box_geom.h; closed forms 8.88e-16 (bar 1e-12); the five layouts 4.44e-16 .. 6.66e-16;
translation and scaling change no bit; the extremes differ from the host restatement by at most 8.88e-16.  Every NMS case gives
the constructed flags.  No kernel needed a change."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, box_overlap                      # noqa: E402
from tests import box_overlap_ref as ref                     # noqa: E402
from tests import box_overlap_cases as cases                 # noqa: E402
from tests import box_overlap_regimes as rg                  # noqa: E402

ABS_TOL = 1e-9          # the hard ceiling of tests/test_gpu_box_overlap.py
EXACT_TOL = 1e-12       # closed forms
_runs = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def launch(dev, A, Bx, crit, na=None, nb=None):
    """(bev, vol) of one rtm3d_box_overlaps launch as numpy arrays; A (B, cap_a, 7), Bx (B, cap_b, 7)."""
    tA, tB = torch.from_numpy(np.array(A)).to(dev), torch.from_numpy(np.array(Bx)).to(dev)       # copies: the cases are read-only
    tna = None if na is None else torch.from_numpy(np.asarray(na, np.int32)).to(dev)
    tnb = None if nb is None else torch.from_numpy(np.asarray(nb, np.int32)).to(dev)
    bev, vol = box_overlap.overlaps(tA, tB, tna, tnb, criterion=crit)
    return bev.cpu().numpy(), vol.cpu().numpy()


def one_by_one(dev, a, b, crit):
    """Pairs (a[k], b[k]) as B = n, cap_a = cap_b = 1: (n, 2) [bev, vol]."""
    bev, vol = launch(dev, a[:, None, :], b[:, None, :], crit)
    return np.stack([bev.reshape(-1), vol.reshape(-1)], 1)


def first_run(dev, crit):
    """The undisturbed 1 x 1 run of the pair set, made once per criterion and shared."""
    if crit not in _runs:
        ps = rg.pair_set()
        _runs[crit] = one_by_one(dev, ps['a'], ps['b'], crit)
        _runs[crit].setflags(write=False)
    return _runs[crit]


def same_bits(x, y):
    return np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


# ------------------------------------------------------------------------------------------------ 1. box_overlaps_kernel
def test_pair_set_equals_the_exact_yardstick(dev):
    ps, yard, bar = rg.pair_set(), rg.yardstick(), rg.bar()
    n = len(ps['a'])
    assert n % 256 and n > 512                                        # more than two blocks, the last one partly filled
    worst, worst_closed, where = 0.0, 0.0, None
    closed = np.isfinite(ps['want_bev'])
    for crit in rg.CRITERIA:
        got = first_run(dev, crit)
        assert got.shape == (n, 2) and np.isfinite(got).all() and (got >= 0).all() and (got <= 1 + EXACT_TOL).all()
        err = np.abs(got - yard['exact'][crit])
        if err.max() > worst:
            worst, where = float(err.max()), (crit, ps['pool'][int(err.max(1).argmax())])
        if crit == 'iou':
            worst_closed = float(max(np.abs(got[closed, 0] - ps['want_bev'][closed]).max(), np.abs(got[closed, 1] - ps['want_vol'][closed]).max()))
            touch = np.char.startswith(ps['pool'], 'touch_') | np.char.startswith(ps['pool'], 'beyond')
            assert not got[touch].any()                               # touching or apart: exactly 0
    print('box overlap regimes: %d pairs, device against the exact yardstick %.3g (%s), YARD_ERR %.3g, bar %.3g; closed forms %.3g (bar %g)'
          % (n, worst, where, yard['yard_err'], bar, worst_closed, EXACT_TOL))
    assert worst_closed <= EXACT_TOL
    assert worst <= bar <= ABS_TOL, (worst, where)


def test_entries_beyond_the_counts_are_zero(dev):
    ps = rg.pair_set()
    n = len(ps['a'])
    na, nb = (np.arange(n) % 7 != 0).astype(np.int32), (np.arange(n) % 11 != 3).astype(np.int32)
    for crit in rg.CRITERIA:
        bev, vol = launch(dev, ps['a'][:, None, :], ps['b'][:, None, :], crit, na, nb)
        got = np.stack([bev.reshape(-1), vol.reshape(-1)], 1)
        counted = (na * nb).astype(bool)
        assert not got[~counted].any() and same_bits(got[counted], first_run(dev, crit)[counted])


@pytest.mark.parametrize('shape', rg.LAYOUTS, ids=lambda s: '%dx%dx%d' % s)
def test_layouts_are_bit_identical_to_one_pair_per_image(dev, shape):
    """cap_a != cap_b both ways round, ragged counts with 0 and the full count, 195 / 300 / 585 / 768 pairs: every counted pair
    has the bits of its 1 x 1 launch and is within the bar of the exact yardstick; every other entry is exactly 0."""
    B, ca, cb = shape
    A, Bx, na, nb = rg.layout(B, ca, cb)
    flat_a = np.repeat(A, cb, axis=1).reshape(-1, 7)                   # pair (m, i, j) at m * ca * cb + i * cb + j
    flat_b = np.tile(Bx, (1, ca, 1)).reshape(-1, 7)
    counted = np.zeros((B, ca, cb), bool)
    for m in range(B):
        counted[m, :na[m], :nb[m]] = True
    assert 0 < counted.sum() < counted.size
    worst = 0.0
    for crit in rg.CRITERIA:
        single = one_by_one(dev, flat_a, flat_b, crit).reshape(B, ca, cb, 2)
        bev, vol = launch(dev, A, Bx, crit, na, nb)
        assert bev.shape == vol.shape == (B, ca, cb)
        assert not bev[~counted].any() and not vol[~counted].any()
        assert same_bits(bev[counted], single[..., 0][counted]) and same_bits(vol[counted], single[..., 1][counted])
        full_bev, full_vol = launch(dev, A, Bx, crit)                  # and with every entry counted
        assert same_bits(full_bev, single[..., 0]) and same_bits(full_vol, single[..., 1])
        for m, i, j in np.argwhere(np.ones_like(counted)):             # the yardstick on every pair, counted or not
            want = rg.ratios(rg.exact_cached(A[m, i], Bx[m, j]), A[m, i], Bx[m, j], crit)
            worst = max(worst, abs(full_bev[m, i, j] - want[0]), abs(full_vol[m, i, j] - want[1]))
    print('layout %s: %d counted pairs of %d, device against the exact yardstick %.3g (bar %.3g)' % (shape, counted.sum(), counted.size, worst, rg.bar()))
    assert worst <= rg.bar()


def test_one_output_null(dev):
    """rtm3d_box_overlaps with exactly one of d_bev / d_3d NULL: the other output has the bits of the two-output run, and the
    buffer that was not passed keeps its sentinel."""
    A, Bx, na, nb = rg.layout(5, 6, 10)
    B, ca, cb = 5, 6, 10
    lib = _lib.load()
    tA, tB = torch.from_numpy(A.copy()).to(dev), torch.from_numpy(Bx.copy()).to(dev)
    tna, tnb = torch.from_numpy(na.copy()).to(dev), torch.from_numpy(nb.copy()).to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for crit in (0, 1, 2):
        out = {}
        for which in ('both', 'bev', '3d'):
            bev = torch.full((B, ca, cb), -7.0, dtype=torch.float64, device=dev)
            vol = torch.full((B, ca, cb), -7.0, dtype=torch.float64, device=dev)
            _lib.check(lib.rtm3d_box_overlaps(stream, B, ca, cb, tna.data_ptr(), tnb.data_ptr(), tA.data_ptr(), tB.data_ptr(), crit,
                                              bev.data_ptr() if which != '3d' else None, vol.data_ptr() if which != 'bev' else None), 'box_overlaps')
            torch.cuda.synchronize()
            out[which] = (bev.cpu().numpy(), vol.cpu().numpy())
        assert (out['both'][0] >= 0).all() and (out['both'][1] >= 0).all() and (out['both'][0] > 0).any() and (out['both'][1] > 0).any()
        assert same_bits(out['bev'][0], out['both'][0]) and (out['bev'][1] == -7.0).all()
        assert same_bits(out['3d'][1], out['both'][1]) and (out['3d'][0] == -7.0).all()


def test_exact_translation_changes_no_bit(dev):
    """h, X, Y, Z on the 2^-10 lattice within +-64: adding 2^20 to X and Z of both boxes (and to Y as well in a second run) is
    exact, and so is every difference box_pair takes first.  The device gives the bits of the untranslated run - at a million
    metres from the origin, where the float yardstick is off by 2e-5."""
    ps, yard = rg.pair_set(), rg.yardstick()
    idx = np.flatnonzero(ps['pool'] == 'lattice')
    T = 2.0 ** 20
    for crit in rg.CRITERIA:
        base = first_run(dev, crit)[idx]
        for move in ((3, 5), (3, 4, 5)):
            a, b = ps['a'][idx].copy(), ps['b'][idx].copy()
            a[:, move] += T
            b[:, move] += T
            got = one_by_one(dev, a, b, crit)
            assert same_bits(got, base), (crit, move, float(np.abs(got - base).max()))
            assert np.abs(got - yard['exact'][crit][idx]).max() <= rg.bar()


@pytest.mark.parametrize('power', [20, -20])
def test_exact_scaling_changes_no_bit(dev, power):
    """h, w, l, X, Y, Z times 2^20 or 2^-20: every operation of box_geom.h scales exactly, so every output keeps its bits; an
    absolute epsilon anywhere in the clip would not."""
    ps = rg.pair_set()
    scale = np.array([2.0 ** power] * 6 + [1.0])
    for crit in rg.CRITERIA:
        got = one_by_one(dev, ps['a'] * scale, ps['b'] * scale, crit)
        base = first_run(dev, crit)
        assert same_bits(got, base), (crit, power, int((got != base).sum()), float(np.abs(got - base).max()))


def test_extremes_stay_finite(dev):
    """Sizes of 1e200 (footprint areas and shoelace products overflow), |ry| up to 1e6, the invalid boxes of the project, all in
    the lanes of one wave: every output is finite and in [0, 1 + 1e-12]; an invalid box overlaps nothing."""
    boxes, invalid = rg.extreme_boxes()
    t = torch.from_numpy(boxes.copy()).to(dev)
    n = len(boxes)
    assert n * n <= 512
    for crit in rg.CRITERIA:
        bev, vol = (x.cpu().numpy() for x in box_overlap.overlaps(t, t, criterion=crit))
        for m in (bev, vol):
            assert m.shape == (n, n) and np.isfinite(m).all() and (m >= 0).all() and (m <= 1 + EXACT_TOL).all(), (crit, m[~np.isfinite(m) | (m > 1)])
            assert not m[invalid].any() and not m[:, invalid].any()
        host = np.array([[rg.model_overlap(a, b, crit)[:2] for b in boxes] for a in boxes])
        print('extremes %s: largest difference from the host restatement %.3g' % (crit, max(np.abs(bev - host[..., 0]).max(), np.abs(vol - host[..., 1]).max())))
        assert abs(bev[0, 0] - 1.0) <= EXACT_TOL and (np.diag(bev)[1:7] > 0.99).all()                         # the ordinary boxes, |ry| up to 1e6


# ------------------------------------------------------------------------------------------------ 2. records_nms3d_kernel
def run_nms(dev, rec, thresh, metric, aware, want):
    """One launch on (B, topk, 32) records with random KITTI rows: the flags are ``want`` and every other byte of the records
    is unchanged, the rows of the slots that went are zeroed and no others, a second call changes nothing."""
    B, topk = rec.shape[:2]
    rows0 = np.random.Generator(np.random.PCG64(B * 1000 + topk)).standard_normal((B, topk, 16))
    t, rows = torch.from_numpy(np.array(rec)).to(dev), torch.from_numpy(rows0.copy()).to(dev)
    assert box_overlap.nms3d_records(t, thresh, metric=metric, class_aware=aware, kitti_rows=rows) is t
    got, got_rows = t.cpu().numpy(), rows.cpu().numpy()
    expect = np.array(rec)
    expect[..., 31] = want
    diff = np.argwhere(got[..., 31].view(np.uint32) != expect[..., 31].view(np.uint32))
    assert len(diff) == 0, (len(diff), diff[:8].tolist())
    assert got.tobytes() == expect.tobytes()
    went = (rec[..., 31] == 2) & (want == 1)
    expect_rows = rows0.copy()
    expect_rows[went] = 0.0
    assert got_rows.tobytes() == expect_rows.tobytes()
    box_overlap.nms3d_records(t, thresh, metric=metric, class_aware=aware, kitti_rows=rows)
    assert t.cpu().numpy().tobytes() == expect.tobytes() and rows.cpu().numpy().tobytes() == expect_rows.tobytes()
    return int(went.sum())


@pytest.mark.parametrize('name', rg.NMS_NAMES)
def test_nms_cases_give_the_constructed_flags(dev, name):
    c = rg.nms_case(name)
    went = run_nms(dev, c['rec'], c['thresh'], c['metric'], c['aware'], c['want'])
    assert went == int(((c['rec'][..., 31] == 2) & (c['want'] == 1)).sum())
    if name.startswith('every_pair'):
        assert went == c['nc'] * (c['nc'] - 1) // 2                    # every pair of candidates, once


def test_all_count_cases_without_the_rows(dev):
    """The same images without KITTI rows (d_kitti = NULL), as a (B, 1, topk, 32) tensor."""
    for topk in rg.COUNT_TOPK:
        c = rg.nms_case('counts_topk%d' % topk)
        t = torch.from_numpy(np.array(c['rec'])).to(dev).unsqueeze(1)
        got = box_overlap.nms3d_records(t, c['thresh']).cpu().numpy()[:, 0]
        expect = np.array(c['rec'])
        expect[..., 31] = c['want']
        assert got.tobytes() == expect.tobytes()


@pytest.mark.parametrize('topk', [100, 130])
@pytest.mark.parametrize('metric', ['bev', '3d'])
def test_nms_runs_the_arithmetic_of_the_overlap_matrix_and_is_strict(dev, topk, metric):
    """A clustered image; M = the device's own overlaps of double(rec[:, 24:31]) (upper triangle: a = the earlier slot).  With
    iou_thresh set to exactly M[j, i] of a pair that suppresses at the usual threshold, to the float just under it, and to other
    entries of M, the flags equal the yardstick's greedy NMS on M - no gap condition: any other arithmetic in the NMS kernel, or a
    `>=`, flips the pair whose IoU the threshold is."""
    rec = cases.nms_records(topk)[:1]
    boxes = torch.from_numpy(rec[0, :, 24:31].astype(np.float64)).to(dev)
    M = box_overlap.overlaps(boxes, boxes)[0 if metric == 'bev' else 1].cpu().numpy()
    M = np.triu(M, 1)
    usual = cases.NMS_THRESH[metric]
    base = ref.nms_flags(rec[0], usual, M)
    i, j = rg.strict_pair(rec[0], M, usual)
    cand = M[np.ix_(rec[0, :, 31] == 2, rec[0, :, 31] == 2)]
    values = np.unique(cand[cand > 0])
    assert len(values) >= 10
    tried = [M[j, i], np.nextafter(M[j, i], 0.0), values[0], values[len(values) // 2], values[-1], np.nextafter(values[-1], 2.0)]
    flips = 0
    for thr in tried:
        want = ref.nms_flags(rec[0], float(thr), M)
        run_nms(dev, rec, float(thr), metric, False, want[None])
        flips += int((want != base).sum())
    at, under = ref.nms_flags(rec[0], float(tried[0]), M), ref.nms_flags(rec[0], float(tried[1]), M)
    assert at[i] == 2 and under[i] == 1 and at[j] == under[j] == 2      # the pair itself does not suppress at its own IoU
    assert flips >= 3
