"""The case table of the 2D decode suite (tests/decode2d_cases.py) against the reference, without a GPU: every case's regime is
derived from its inputs and the reference alone and must be the regime the case names; every promised regime has a case; the
two torch sigmoid forms reproduce torch.sigmoid of the whole tensor; the NumPy restatement of the contract equals the oracle bit
for bit on every case without score ties (and as a set of detections on the others), so no case goes uncompared."""
import numpy as np
import pytest
import torch

from oracle import smoke_ref
from tests import decode2d_cases as dc
from tests import decode2d_ref as R

_regimes = {}


def regime(name):
    if name not in _regimes:
        _regimes[name] = dc.regime(dc.build(name))
    return _regimes[name]


def assert_slots_equal(got, ref, fields=('cls', 'score', 'mproj', 'verts', 'bbox')):
    """Bit-equal below n[b]; NaN in the same places."""
    np.testing.assert_array_equal(got['n'], ref['n'])
    for b, n in enumerate(ref['n']):
        for k in fields:
            g, r = got[k][b, :n], ref[k][b, :n]
            if g.dtype == np.float32:
                np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg='%s image %d: NaN pattern' % (k, b))
                m = ~np.isnan(r)
                np.testing.assert_array_equal(R.bits(g[m]), R.bits(r[m]), err_msg='%s image %d' % (k, b))
            else:
                np.testing.assert_array_equal(g, r, err_msg='%s image %d' % (k, b))


@pytest.mark.parametrize('name', list(dc.CASES))
def test_case_names_its_regime(name):
    r, c = regime(name), dc.CASES[name]
    assert r['ties'] == c['ties'], (r['ties'], r['min_gap_ulps'])
    for k, want in c['expect'].items():
        got = r[k]
        if k == 'cells':
            want = sorted(want)
        assert got == want, (k, got, want)
    if not r['defined']:
        # a few ulp between neighbouring scores, so that neither sigmoid form can flip the order
        assert r['min_gap_ulps'] >= 16, r['min_gap_ulps']


def test_every_regime_has_a_case():
    rs = {name: regime(name) for name in dc.CASES}
    for what, pred in dc.COVERAGE.items():
        assert any(pred(r) for r in rs.values()), what
    topks = {dc.build(n)['topk'] for n in dc.CASES}
    assert {1, 30, 100, 256} <= topks
    for rel in (-1, 0, 1):                                             # candidates == topk - 1, topk, topk + 1
        assert any(r['cand'][0] == dc.build(n)['topk'] + rel for n, r in rs.items()), rel
    assert {rs[n]['n'][0] for n in dc.SUB_CASES} == set(dc.SUB_N)
    shapes = {dc.build(n)['heat'].shape[2:] for n in dc.CASES}
    assert any(h == 1 and w > 1 for h, w in shapes) and any(w == 1 and h > 1 for h, w in shapes) and (1, 1) in shapes
    assert any(len(r['n']) > 1 and 0 in r['n'] and max(r['n']) > 0 for r in rs.values())       # an empty image in a batch
    # the non-finite cases keep n + (NaN heat cells) below topk: the reference lets a NaN cell occupy a top-k slot
    for n, r in rs.items():
        if r['nan_heat']:
            assert max(r['n']) + r['nan_heat'] < dc.build(n)['topk']


@pytest.mark.parametrize('name', list(dc.CASES))
def test_sigmoid_forms_reproduce_torch(name):
    inp = dc.build(name)
    for b in range(inp['heat'].shape[0]):
        h = inp['heat'][b]
        if h.size < R.GRAIN:
            np.testing.assert_array_equal(R.bits(R.sig_positional(h)), R.bits(torch.sigmoid(torch.from_numpy(h.copy())).numpy()))
    r = regime(name)
    if r['defined']:
        o = R.oracle(inp)
        H, W = inp['heat'].shape[2:]
        for b, n in enumerate(o['n']):
            if n == 0:
                continue
            if r['ties']:
                continue
            flat = dc.reference_candidates(inp['heat'][b], inp['thresh'])[1][:n]        # no ties: the oracle's order
            y, x = flat % (H * W) // W, flat % W
            np.testing.assert_array_equal(flat // (H * W), o['cls'][b, :n])
            g = np.ascontiguousarray(inp['moff'][b][:, y, x])
            if not np.isfinite(g).all():
                continue
            np.testing.assert_array_equal(R.bits(R.sig_positional(g)), R.bits(torch.sigmoid(torch.from_numpy(g)).numpy()))
            # kept scores: the form the position names
            lg = inp['heat'][b][o['cls'][b, :n], y, x]
            want = np.where(flat < r['vec_end'], R.sig_vector(lg), R.sig_scalar(lg))
            np.testing.assert_array_equal(R.bits(o['score'][b, :n]), R.bits(want))


def test_distinguishing_values_differ():
    v = R.distinguishing(1, 64, -3.0, 3.0)
    assert len(np.unique(v)) == 64 and (R.bits(R.sig_vector(v)) != R.bits(R.sig_scalar(v))).all()
    np.testing.assert_array_equal(v, R.distinguishing(1, 64, -3.0, 3.0))


def canon(s, b, H, W):
    n = s['n'][b]
    rows = [(float(s['score'][b, i]), int(s['cls'][b, i]), s['mproj'][b, i].tobytes(), s['verts'][b, i].tobytes(), s['bbox'][b, i].tobytes())
            for i in range(n)]
    return sorted(rows, key=lambda t: (-t[0], t[1], t[2]))


@pytest.mark.parametrize('name', list(dc.CASES))
def test_contract_equals_oracle(name):
    inp, r = dc.build(name), regime(name)
    c, o = R.contract(inp), R.oracle(inp)
    for b in range(len(r['cand'])):
        sc, flat = R.candidates(inp['heat'][b], inp['thresh'])
        sr, fr = dc.reference_candidates(inp['heat'][b], inp['thresh'])
        np.testing.assert_array_equal(flat, fr)
        np.testing.assert_array_equal(R.bits(sc), R.bits(sr))
    if not r['ties']:
        assert_slots_equal(c, o)
        return
    # ties: the contract's rows are ordered by score, then flat index
    np.testing.assert_array_equal(c['n'], o['n'])
    H, W = inp['heat'].shape[2:]
    for b, n in enumerate(c['n']):
        flat = c['cls'][b, :n] * H * W + (c['mproj'][b, :n, 1] // 4).astype(int) * W + (c['mproj'][b, :n, 0] // 4).astype(int)
        key = list(zip(-c['score'][b, :n].astype(np.float64), flat))
        assert key == sorted(key) and len(set(flat)) == n
        np.testing.assert_array_equal(np.sort(c['score'][b, :n]), np.sort(o['score'][b, :n]))
        if r['cut_byte'][b] is None or r['cut_byte'][b] < 4:           # no cut inside a tie: the same detections, in another order
            assert canon(c, b, H, W) == canon(o, b, H, W)


def test_smoke_formulas_equal_the_oracle_decode():
    """decode2d_ref.smoke is oracle/smoke_ref.decode's closed form for given peaks."""
    rng = np.random.Generator(np.random.PCG64(8))
    heat = np.full((1, 3, 8, 16), -6.0, np.float32)
    for c, y, x, v in [(0, 1, 1, 2.0), (1, 7, 15, 1.5), (2, 4, 9, 1.0)]:
        heat[0, c, y, x] = v
    reg = rng.standard_normal((1, 8, 8, 16)).astype(np.float32)
    K = np.array([700.0, 0, 30.0, 0, 710.0, 16.0, 0, 0, 1])
    dim_ref = [[1.5, 1.6, 3.9], [1.7, 0.6, 0.8], [1.7, 0.6, 1.8]]
    d = smoke_ref.decode(torch.from_numpy(heat), torch.from_numpy(reg), K, dim_ref, 0.4, 10, 4.0)[0]
    x8, _, _ = R.smoke(d['cls'], d['xy'][:, 0].astype(int), d['xy'][:, 1].astype(int), reg[0], K, dim_ref, 4.0)
    np.testing.assert_array_equal(x8, d['x8'])
