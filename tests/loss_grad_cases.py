"""Cases of the loss-gradient tests (tests/test_loss_grad_cpu.py, tests/test_gpu_loss_grad.py): every case of tests/loss_cases.py
plus the regimes the backward adds.  A gradient case is a dict: case (a loss_cases case), logits (the four fp32 maps), weights
(W_MKF, W_VFM, W_M_OFF, W_V_OFF), upstream (None = 1), marks (named cells the CPU test looks at).  Deterministic numpy only; all
on the 3 x 24 x 40 and 3 x 13 x 37 maps with B <= 5."""
import numpy as np

from tests import loss_cases as lc, loss_grad_ref as gref, loss_ref as ref

F32 = np.float32
DEFAULT_WEIGHTS = (1.0, 1.0, 0.5, 0.5)
NEW_CASES = ('collide', 'clamp', 'noise_only', 'mask3d_off', 'sign0', 'nonfinite', 'weights', 'pow_weights')
ALL_CASES = lc.ALL_CASES + NEW_CASES
MAPS = ('heat map', 'ver_coor', 'm_off', 'v_off')


def _far(img, X, Y, H, W, Z=80.0, ry=0.3):
    """A small far pedestrian: at Z = 80 its eight corners span well under one map cell across and about one down."""
    dim, loc = lc.DIMS[1], (X, Y, Z)
    return (img, 1, 0, lc.fit_bbox(dim, loc, ry, lc.camera(H, W), H, W), dim, loc, ry)


def _table(c):
    b = lc.batch(c)
    return b, ref.object_table(b.rows, b.K, c['B'], c['H'], c['W'])


def make(name):
    """-> {'case', 'logits', 'weights', 'upstream', 'marks'}"""
    if name in lc.ALL_CASES:
        c = lc.make(name)
        return {'case': c, 'logits': lc.logits(c), 'weights': DEFAULT_WEIGHTS, 'upstream': None, 'marks': {}}
    weights, upstream, marks = DEFAULT_WEIGHTS, None, {}
    if name == 'collide':
        # two far boxes 2 cm apart: their 16 corners truncate into the same few v_proj cells and they share the m_proj cell; a
        # third far box elsewhere, and a plain near object
        H, W = 13, 37
        c = lc._case(1, H, W, [_far(0, 2.0, 1.2, H, W), _far(0, 2.02, 1.2, H, W), _far(0, -9.0, 0.9, H, W, ry=-1.0),
                               lc._plain(0, 0, 0, lc._box_at(9, 9))], seed=21)
        lg = lc.logits(c)
    elif name == 'clamp':
        # both images hold a real object and a noise object; image 0 gets +12, image 1 -12 on the positive centre, the noise
        # centre, a cell inside the real object's Gaussian and a cell no object reaches; cells (0, 0) and (0, 1) of class 0 get
        # logits whose sigmoid lies just inside each bound (logit(0.9999) = 9.2102...)
        H, W = 24, 40
        objs = sum([[lc._plain(b, 2, 0, lc._box_at(20, 7, 8.0)), lc._plain(b, 1, 1, lc._box_at(10, 6))] for b in range(2)], [])
        c = lc._case(2, H, W, objs, seed=22)
        lg = lc.logits(c)
        cells = {'positive': (2, 7, 20), 'noise': (1, 6, 10), 'gaussian': (2, 8, 21), 'empty': (0, 20, 35)}
        for b, v in ((0, 12.0), (1, -12.0)):
            for k, (cl, y, x) in cells.items():
                lg[0][b, cl, y, x] = v
                marks['%s%+d' % (k, v)] = (b, cl, y, x)
        for b in range(2):
            lg[0][b, 0, 0, 0], lg[0][b, 0, 0, 1] = 9.2, -9.2
        marks['inside_hi'], marks['inside_lo'] = (0, 0, 0, 0), (0, 0, 0, 1)
    elif name == 'noise_only':               # no positive: the divisor is 1; no selection: the regression maps are all zero
        H, W = 13, 37
        c = lc._case(2, H, W, [lc._plain(0, 1, 1, lc._box_at(10, 6)), lc._plain(1, 0, 1, lc._box_at(30, 3))], seed=23)
        lg = lc.logits(c)
    elif name == 'mask3d_off':               # the only real object has mask_3d = 0: ver_coor and vertex_off select nothing
        H, W = 13, 37
        c = lc._case(1, H, W, [lc._plain(0, 0, 0, lc._box_at(12, 6))], seed=24, mask_3d=[0.0])
        lg = lc.logits(c)
    elif name == 'sign0':                    # two ver_coor logits set to their fp32 targets exactly
        c = lc.make('fx_b2_empty')
        c['seed'] = 25
        lg = lc.logits(c)
        _, tab = _table(c)
        i = [k for k, t in enumerate(tab) if t[2] and not t[3] and t[4] and t[5] and t[80] and t[83]][0]
        t = tab[i]
        b, mx, my = int(t[0]), int(t[8]), int(t[9])
        for ch in (0, 7):                    # vertex 0 channel 0, vertex 3 channel 1
            lg[1][b, ch, my, mx] = F32(t[64 + ch])
            marks['sign0_%d' % ch] = (b, ch, my, mx)
    elif name == 'nonfinite':                # a NaN and a +-inf heat-map logit, NaN regression logits on cells that take part
        c = lc.make('fx_b5_odd')
        c['seed'] = 26
        lg = lc.logits(c)
        _, tab = _table(c)
        i = [k for k, t in enumerate(tab) if t[2] and not t[3] and t[4] and t[5] and t[81]][0]
        t = tab[i]
        b, mx, my = int(t[0]), int(t[8]), int(t[9])
        lg[0][3, 1, 5, 7], lg[0][0, 0, 2, 2], lg[0][4, 2, 12, 36] = np.nan, np.inf, -np.inf
        lg[0][b, int(t[1]), my, mx] = np.nan                                   # a NaN on a positive centre too
        lg[1][b, 3, my, mx] = np.nan                                           # vertex 1, channel 1
        lg[2][b, 0, my, mx] = np.nan
        lg[3][b, 1, int(t[35]), int(t[34])] = np.nan                           # v_proj of vertex 1
        marks.update(hm_nan=(3, 1, 5, 7), hm_pinf=(0, 0, 2, 2), hm_ninf=(4, 2, 12, 36), hm_nan_pos=(b, int(t[1]), my, mx),
                     vc_nan=(b, 3, my, mx), mo_nan=(b, 0, my, mx), vo_nan=(b, 1, int(t[35]), int(t[34])))
    elif name == 'weights':                  # a zero and a negative weight, an upstream factor
        c = lc.make('fx_b1')                 # (fx_b1's own logits: the CPU test compares the two)
        lg, weights, upstream = lc.logits(c), (2.0, 0.0, -0.75, 0.25), 0.5
    elif name == 'pow_weights':              # the powf instances with weights and an upstream factor
        c = lc.make('fx_pow')
        c['seed'] = 28
        lg, weights, upstream = lc.logits(c), (0.5, 1.5, 1.0, 2.0), 0.5
    else:
        raise KeyError(name)
    return {'case': c, 'logits': lg, 'weights': weights, 'upstream': upstream, 'marks': marks}


_cache = {}


def restated(name):
    """{'spec', 'batch', 'tab', 'm_hm', 'items', 'counts', 'g32', 'g64', 'contrib'} of the restatement, computed once per case and
    read only."""
    if name not in _cache:
        s = make(name)
        c = s['case']
        b, tab = _table(c)
        dims = (c['B'], c['C'], c['H'], c['W'])
        hm = ref.heatmap(tab, b.img_start, *dims)
        items, counts = ref.loss(tab, b.img_start, *dims, s['logits'], c['alpha'], c['beta'], s['weights'])
        contrib = {}
        kw = dict(alpha=c['alpha'], beta=c['beta'], weights=s['weights'], upstream=s['upstream'], m_hm=hm)
        g32 = gref.grad(tab, b.img_start, *dims, s['logits'], counts, contributions=contrib, **kw)
        g64 = gref.grad(tab, b.img_start, *dims, s['logits'], counts, f64=True, **kw)
        for a in [tab, hm, items, counts] + g32 + g64 + list(s['logits']):
            a.setflags(write=False)
        _cache[name] = {'spec': s, 'batch': b, 'tab': tab, 'm_hm': hm, 'items': items, 'counts': counts, 'g32': g32, 'g64': g64,
                        'contrib': contrib}
    return _cache[name]


def ulp_floor(g):
    """4 fp32 ulp of the largest finite magnitude of a map."""
    a = np.abs(np.asarray(g, np.float64))
    a = a[np.isfinite(a)]
    return 4.0 * float(np.spacing(F32(a.max(initial=0.0))))


def compare(got, want, bar, what):
    """NaNs in the same places, zeros in the same places, the rest within bar: -> the max abs error."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN pattern', np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    ok = ~np.isnan(want)
    assert np.array_equal((got == 0) & ok, (want == 0) & ok), (what, 'zero pattern', np.argwhere(((got == 0) != (want == 0)) & ok)[:5])
    err = float(np.abs(got.astype(np.float64)[ok] - want.astype(np.float64)[ok]).max(initial=0.0))
    assert err <= bar, (what, err, bar)
    return err


def fixture_bar(g, name, k):
    """max(4 x the reference's own max |fp32 run - fp64 run| over map k, 4 fp32 ulp of the map's largest magnitude): (f64, bar)."""
    f32, f64 = g['%s/g%d_f32' % (name, k)], g['%s/g%d_f64' % (name, k)]
    return f64, max(4.0 * float(np.abs(f32.astype(np.float64) - f64).max(initial=0.0)), ulp_floor(f64))


def restatement_bar(r, k):
    """max(4 x the distance between the restatement's fp32 and fp64 runs over map k, the 4-ulp floor): (distance, bar)."""
    a, b = r['g32'][k].astype(np.float64), r['g64'][k]
    ok = ~np.isnan(b)
    d = float(np.abs(a[ok] - b[ok]).max(initial=0.0))
    return d, max(4.0 * d, ulp_floor(b))
