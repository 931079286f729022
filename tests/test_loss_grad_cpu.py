"""CPU (-m "not gpu"): the loss-gradient rule.  tests/loss_grad_ref.py - the numpy restatement the device is tested against -
is checked here against the reference-run fixture tests/golden/loss_grad_cases.npz (tests/golden/make_loss_grad_golden.py: the
reference's own loss.backward() in fp32 and fp64), and the regime cases of tests/loss_grad_cases.py are checked to hold what
they are named for."""
import numpy as np
import pytest

from tests import loss_cases as lc, loss_grad_cases as gc
from tests.util import load_golden

F32 = np.float32


@pytest.mark.parametrize('name', lc.FIXTURE_CASES)
def test_restatement_matches_the_reference_run(name):
    """Per map: the zero pattern equal to the reference's, max abs error against its fp64 gradient within max(4 x its own max
    |fp32 - fp64| over the map, 4 fp32 ulp of the map's largest magnitude).  Measured (max error / bar): heat map 9.0e-8 / 4.2e-7
    (fx_b1), 1.05e-7 / 4.2e-7, 7.1e-8 / 3.1e-7, 7.1e-8 / 2.5e-7 (fx_pow), 5.7e-7 / 2.3e-6 (fx_none: no positive, the divisor is
    1); the regression maps at most 3.2e-9 (m_off of fx_b1, bar 1.35e-8), each at most 0.3 of its bar."""
    g = load_golden('loss_grad_cases.npz')
    r = gc.restated(name)
    for k, what in enumerate(gc.MAPS):
        f64, bar = gc.fixture_bar(g, name, k)
        assert r['g32'][k].dtype == F32
        err = gc.compare(r['g32'][k], f64, bar, (name, what))
        print(name, what, 'max abs error vs the reference fp64 run %.3g, bar %.3g' % (err, bar))
    if name == 'fx_none':
        assert all(not r['g32'][k].any() for k in (1, 2, 3)) and r['g32'][0].all() and r['counts'][0] == 0


def test_fixture_logits_keep_clear_of_the_clamp_bounds():
    edge = np.log(1e-4 / (1 - 1e-4))
    for name in lc.FIXTURE_CASES:
        x = np.abs(gc.make(name)['logits'][0].astype(np.float64))
        assert (np.abs(x - abs(edge)) > 1e-3).all()


def _at(r, k, idx):
    return r['g32'][k][idx]


def test_regime_cases_hold_what_they_are_named_for():
    """The cases the backward adds reach the branches they are built for (checked on the restatement)."""
    # collisions: two objects on one m_proj cell in fx_b1; in 'collide' the corners of a far box fall into at most three v_proj
    # cells, two objects share v_proj cells and the m_proj cell
    r = gc.restated('fx_b1')
    assert max(r['contrib']['m_off'].values()) >= 2 and max(r['contrib']['ver_coor'].values()) >= 2
    r = gc.restated('collide')
    tab = r['tab']
    for i in (0, 1, 2):
        cells = {(int(tab[i, 32 + 2 * v]), int(tab[i, 33 + 2 * v])) for v in range(8)}
        assert len(cells) <= 3 and tab[i, 80:88].all() and tab[i, 4] == 1, (i, cells)
    shared = {(int(tab[0, 32 + 2 * v]), int(tab[0, 33 + 2 * v])) for v in range(8)} & {(int(tab[1, 32 + 2 * v]), int(tab[1, 33 + 2 * v])) for v in range(8)}
    assert shared and (tab[0, 8:10] == tab[1, 8:10]).all()
    n = r['contrib']['v_off'].values()
    assert max(n) >= 6 and sum(n) == 2 * r['counts'][2] and len(n) < sum(n) // 2
    assert max(r['contrib']['m_off'].values()) == 2 and max(r['contrib']['ver_coor'].values()) == 2
    # clamp: +-12 saturates on every kind of cell - exact zeros - and +-9.2 stays inside
    r = gc.restated('clamp')
    m, hm = r['spec']['marks'], r['m_hm']
    assert hm[m['positive+12']] == 1 and hm[m['noise+12']] == F32(0.9999) and 0 < hm[m['gaussian+12']] < 1 and hm[m['empty+12']] == 0
    for k, idx in m.items():
        if k.startswith('inside'):
            assert _at(r, 0, idx) != 0 and np.isfinite(_at(r, 0, idx)), k
        else:
            assert _at(r, 0, idx) == 0, k
    assert (r['g32'][0] == 0).sum() == 8
    # num_pos == 0 with objects present: the divisor is 1, nothing is selected
    r = gc.restated('noise_only')
    assert r['counts'].tolist() == [0, 0, 0, 0, 0] and np.isnan(r['items'][1:]).all() and r['g32'][0].all()
    assert all(not r['g32'][k].any() and not np.signbit(r['g32'][k]).any() for k in (1, 2, 3))
    # an empty selection next to a full one: NaN items, finite maps
    r = gc.restated('mask3d_off')
    assert r['counts'].tolist() == [1, 0, 0, 1, 0] and np.isnan(r['items'][[1, 3, 4]]).all() and np.isfinite(r['items'][[0, 2]]).all()
    assert not r['g32'][1].any() and not r['g32'][3].any() and (r['g32'][2] != 0).sum() == 2 and all(np.isfinite(a).all() for a in r['g32'])
    # sign(0): the planted elements are +0.0f while their neighbours in the same cell are not
    r = gc.restated('sign0')
    for k, idx in r['spec']['marks'].items():
        v = _at(r, 1, idx)
        assert v == 0 and not np.signbit(v) and r['contrib']['ver_coor'][idx] == 1, k
        assert _at(r, 1, (idx[0], idx[1] ^ 1) + idx[2:]) != 0
    # non-finite logits: each affects its own element only
    r, base = gc.restated('nonfinite'), gc.restated('fx_b5_odd')
    m = r['spec']['marks']
    nan_at = lambda k: {tuple(i) for i in np.argwhere(np.isnan(r['g32'][k]))}
    assert nan_at(0) == {m['hm_nan'], m['hm_nan_pos']} and nan_at(1) == {m['vc_nan']} and nan_at(2) == {m['mo_nan']} and nan_at(3) == {m['vo_nan']}
    assert _at(r, 0, m['hm_pinf']) == 0 and _at(r, 0, m['hm_ninf']) == 0
    assert r['m_hm'][m['hm_nan_pos']] == 1 and r['contrib']['v_off'][m['vo_nan']] >= 1
    # parameters: a zero weight gives a zero map, a negative one flips the sign, upstream scales
    r, base = gc.restated('weights'), gc.restated('fx_b1')
    assert r['spec']['upstream'] == 0.5 and not r['g32'][1].any()
    nz = base['g32'][2] != 0
    assert nz.any() and (np.sign(r['g32'][2][nz]) == -np.sign(base['g32'][2][nz])).all()
    np.testing.assert_array_equal(r['g32'][0], base['g32'][0])                # 2.0 * 0.5 = 1: the same factor
    r = gc.restated('pow_weights')
    assert (r['spec']['case']['alpha'], r['spec']['case']['beta']) == (1.5, 3.0)


def test_restatement_fp64_switch_runs_the_same_rule():
    """The fp64 run differs from the fp32 run by rounding only: same NaN and zero patterns, distance far below the values."""
    for name in ('fx_b1', 'fx_pow', 'collide', 'nonfinite'):
        r = gc.restated(name)
        for k in range(4):
            assert r['g64'][k].dtype == np.float64
            d, bar = gc.restatement_bar(r, k)
            gc.compare(r['g32'][k], r['g64'][k], 1e-6 * max(1.0, float(np.nanmax(np.abs(r['g64'][k])))), (name, k))
            assert d <= bar
