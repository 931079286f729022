"""Cases of the validation-loss tests (tests/test_loss_cpu.py, tests/test_gpu_loss.py) and of the reference-run fixture
(tests/golden/make_loss_golden.py): deterministic numpy only.  A case is a dict: B, H, W, C, the per-object arrays img_id, cls,
noise, bbox (input pixels), dim (h w l), loc (bottom centre), ry, mask_3d (None: derived), K (B, 9) in input pixels, alpha,
beta, seed (of its logits)."""
import numpy as np

from tests import loss_ref as ref

DS = 4.0
DIMS = ((1.5, 1.6, 3.9), (1.75, 0.65, 0.85), (1.7, 0.6, 1.75))
FIXTURE_CASES = ('fx_b1', 'fx_b2_empty', 'fx_b5_odd', 'fx_pow', 'fx_none')


def camera(H, W):
    f = 0.9 * DS * W
    return np.array([f, 0.0, DS * W / 2, 0.0, f, DS * H / 2, 0.0, 0.0, 1.0])


def corners_uvz(dim, loc, ry, K):
    """(8, 3) u, v, depth of the box corners in input pixels (case construction only: where an object lands)."""
    h, w, l = dim
    s, c = np.sin(ry), np.cos(ry)
    out = []
    for j in range(8):
        sx, sy, sz = (-1.0 if j & 4 else 1.0), (-1.0 if j & 2 else 1.0), (-1.0 if j & 1 else 1.0)
        X = c * l / 2 * sx + s * w / 2 * sz + loc[0]
        Y = h / 2 * sy + loc[1] - h / 2
        Z = -s * l / 2 * sx + c * w / 2 * sz + loc[2]
        out.append(((K[0] * X + K[2] * Z) / (Z + 1e-6), (K[4] * Y + K[5] * Z) / (Z + 1e-6), Z))
    return np.array(out)


def fit_bbox(dim, loc, ry, K, H, W):
    uv = corners_uvz(dim, loc, ry, K)
    lo, hi = uv[:, :2].min(0), uv[:, :2].max(0)
    return [float(np.clip(lo[0], 0, DS * W - 1)), float(np.clip(lo[1], 0, DS * H - 1)),
            float(np.clip(hi[0], 0, DS * W - 1)), float(np.clip(hi[1], 0, DS * H - 1))]


def _case(B, H, W, objs, alpha=2.0, beta=4.0, seed=0, mask_3d=None, K=None):
    """objs: (img, cls, noise, bbox, dim, loc, ry), sorted by img here."""
    objs = sorted(objs, key=lambda o: o[0])
    col = lambda k, shape: np.array([o[k] for o in objs], np.float64).reshape((len(objs),) + shape)
    return {'B': B, 'H': H, 'W': W, 'C': 3, 'img_id': col(0, ()), 'cls': col(1, ()), 'noise': col(2, ()), 'bbox': col(3, (4,)),
            'dim': col(4, (3,)), 'loc': col(5, (3,)), 'ry': col(6, ()), 'mask_3d': None if mask_3d is None else np.asarray(mask_3d, np.float64),
            'K': np.tile(camera(H, W), (B, 1)) if K is None else np.asarray(K, np.float64), 'alpha': alpha, 'beta': beta, 'seed': seed}


def _scene(rng, img, n, H, W):
    """n plausible objects of image img: classes 0..2, every fourth a noise row, every fifth cls -1."""
    K = camera(H, W)
    out = []
    for i in range(n):
        cls = int(rng.integers(0, 3))
        dim = tuple(np.array(DIMS[cls]) * rng.uniform(0.9, 1.1, 3))
        Z = rng.uniform(7, 30)
        X = rng.uniform(-0.4, 0.4) * Z * DS * W / K[0]
        loc = (X, rng.uniform(1.3, 1.9) * Z / 15 + 0.5, Z)
        ry = rng.uniform(-np.pi, np.pi)
        out.append((img, -1 if i % 5 == 4 else cls, 1 if i % 4 == 3 and i % 5 != 4 else 0, fit_bbox(dim, loc, ry, K, H, W), dim, loc, ry))
    return out


def _twin(o, shift, cls=None):
    """A copy of object o moved by shift input pixels, of class cls (None: the same class)."""
    b = [o[3][0] + shift, o[3][1], o[3][2] + shift, o[3][3]]
    return (o[0], o[1] if cls is None else cls, 0, b, o[4], o[5], o[6])


def _box_at(mx, my, half=6.0):
    """An input-pixel box whose centre truncates to map cell (mx, my)."""
    cx, cy = DS * mx + 1.5, DS * my + 2.5
    return [cx - half, cy - half, cx + half, cy + half]


def _plain(img, cls, noise, bbox, Z=15.0, X=0.0, ry=0.3):
    return (img, cls, noise, bbox, DIMS[max(cls, 0)], (X, 1.6, Z), ry)


def make(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == 'fx_b1':                      # one image: a scene, two same-class Gaussians overlapping, another class on the same cell
        s = _scene(rng, 0, 6, 24, 40)
        real = [o for o in s if o[1] >= 0 and o[2] == 0][0]
        return _case(1, 24, 40, s + [_twin(real, 9.0), _twin(real, 0.0, (real[1] + 1) % 3)], seed=1)
    if name == 'fx_b2_empty':                # objects next to an empty image
        return _case(2, 24, 40, _scene(rng, 0, 7, 24, 40), seed=2)
    if name == 'fx_b5_odd':                  # B = 5 on the odd map
        return _case(5, 13, 37, sum([_scene(rng, b, n, 13, 37) for b, n in enumerate((3, 0, 5, 1, 4))], []), seed=3)
    if name == 'fx_pow':                     # alpha, beta that are no squares
        return _case(2, 13, 37, _scene(rng, 0, 4, 13, 37) + _scene(rng, 1, 3, 13, 37), alpha=1.5, beta=3.0, seed=4)
    if name == 'fx_none':                    # no object in the whole batch
        return _case(2, 13, 37, [], seed=5)
    H, W = 13, 37
    if name == 'borders':                    # squares clipped at each border, centres in (0, 0) and (W - 1, H - 1)
        cells = [(0, 0), (W - 1, H - 1), (0, 6), (W - 1, 5), (17, 0), (20, H - 1)]
        return _case(1, H, W, [_plain(0, i % 3, 0, _box_at(mx, my, 9.0)) for i, (mx, my) in enumerate(cells)], seed=6)
    if name == 'noise':                      # image 0: a noise object alone; image 1: a noise object on a real object's centre
        return _case(2, H, W, [_plain(0, 1, 1, _box_at(10, 6)), _plain(1, 2, 0, _box_at(20, 7)), _plain(1, 2, 1, _box_at(20, 7, 8.0)),
                               _plain(1, 0, 0, _box_at(5, 3))], seed=7)
    if name == 'ignored':                    # cls = -1 rows between real ones, one on a real object's cell
        return _case(1, H, W, [_plain(0, -1, 0, _box_at(8, 4)), _plain(0, 0, 0, _box_at(8, 4)), _plain(0, -1, 0, _box_at(30, 9)),
                               _plain(0, 2, 0, _box_at(25, 8))], seed=8)
    if name == 'vertices':
        # 0: a near box whose corners leave the map; 1: a corner moved to u = -0.5 map cells (it truncates to 0 and stays in);
        # 2: corners behind the camera (derived mask_3d false); 3: a plain box
        K = camera(H, W)
        near = (0, 0, 0, _box_at(18, 6, 30.0), DIMS[0], (0.5, 1.6, 4.0), 0.4)
        dim, loc, ry = DIMS[1], [-3.0, 1.7, 12.0], 0.2
        uvz = corners_uvz(dim, loc, ry, K)
        j = int(np.argmin(uvz[:, 0]))
        loc[0] += (-0.5 * DS - uvz[j, 0]) * uvz[j, 2] / K[0]
        edge = (0, 1, 0, _box_at(1, 6), dim, tuple(loc), ry)
        behind = (0, 2, 0, _box_at(30, 5), (1.7, 1.6, 1.8), (0.2, 1.5, 0.5), 0.0)
        return _case(1, H, W, [near, edge, behind, _plain(0, 0, 0, _box_at(9, 9))], seed=9)
    if name == 'vertices_mask3d':            # the same objects, mask_3d supplied by the caller (the opposite of the derived one)
        c = make('vertices')
        c['mask_3d'] = np.array([0.0, 1.0, 1.0, 0.0])
        return c
    if name == 'zero_size':                  # R = 0: a single cell
        return _case(1, H, W, [_plain(0, 0, 0, [50.0, 22.0, 50.0, 22.0]), _plain(0, 1, 1, [90.5, 30.0, 90.5, 30.0])], seed=10)
    if name == 'huge':                       # a box wider than the map: R > W
        return _case(1, H, W, [_plain(0, 1, 0, [-2000.0, -300.0, 2100.0, 380.0]), _plain(0, 1, 0, _box_at(30, 3))], seed=11)
    if name == 'outside':                    # m_proj outside the map on each side; centre -0.5 truncates to 0 and stays inside
        boxes = [[-40.0, 10.0, -8.0, 30.0], [DS * W + 2, 10.0, DS * W + 30, 30.0], [40.0, -50.0, 60.0, -6.0], [40.0, DS * H + 1, 60.0, DS * H + 9],
                 [-9.0, 10.0, 5.0, 30.0]]
        return _case(2, H, W, [_plain(i % 2, i % 3, 0, b) for i, b in enumerate(boxes)] + [_plain(0, 0, 0, _box_at(12, 6))], seed=12)
    if name == 'many':                       # 150 objects in one image: two LDS chunks, the second neither full nor a multiple of 64
        objs = []
        for i in range(150):
            objs.append(_plain(0, i % 3, 1 if i % 7 == 0 else 0, _box_at((i * 5) % W, (i * 3) % H, 3.0 + i % 4), Z=10.0 + i % 9, X=(i % 11) - 5.0))
        return _case(2, H, W, objs + [_plain(1, 0, 0, _box_at(4, 4))], seed=13)
    raise KeyError(name)


REGIME_CASES = ('borders', 'noise', 'ignored', 'vertices', 'vertices_mask3d', 'zero_size', 'huge', 'outside', 'many')
ALL_CASES = FIXTURE_CASES + REGIME_CASES


def logits(case, scale=2.0):
    """The four fp32 logit maps of a case (heat map, ver_coor, m_off, v_off)."""
    rng = np.random.default_rng(1000 + case['seed'])
    B, H, W = case['B'], case['H'], case['W']
    return [(rng.standard_normal((B, ch, H, W)) * scale).astype(np.float32) for ch in (case['C'], 16, 2, 2)]


def batch(case):
    from rtm3d_amd.loss import LabelBatch
    return LabelBatch(case['B'], case['img_id'], case['cls'], case['noise'], case['bbox'], case['dim'], case['loc'], case['ry'], case['K'],
                      mask_3d=case['mask_3d'], num_classes=case['C'], down_sample=DS)


# ---- shared by the CPU and the GPU tests: the restatement of every case (computed once, read only) and the bars of the issue
_cache = {}


def restated(name):
    """(case, batch, table, m_hm, items, counts) of the restatement, computed once per case."""
    if name not in _cache:
        c = make(name)
        b = batch(c)
        tab = ref.object_table(b.rows, b.K, c['B'], c['H'], c['W'])
        hm = ref.heatmap(tab, b.img_start, c['B'], c['C'], c['H'], c['W'])
        items, counts = ref.loss(tab, b.img_start, c['B'], c['C'], c['H'], c['W'], logits(c), c['alpha'], c['beta'])
        for a in (tab, hm, items, counts):
            a.setflags(write=False)
        _cache[name] = (c, b, tab, hm, items, counts)
    return _cache[name]


def ulp_diff32(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_heatmap(hm, want, tab):
    """Equal after rounding to fp32; at most 1 fp32 ulp where the two exps differ; centre cells exactly 1.0f / 0.9999f."""
    assert hm.dtype == np.float32 and hm.shape == want.shape
    d = ulp_diff32(hm, want)
    assert d.max(initial=0) <= 1, d.max()
    assert ((hm == 0) == (want == 0)).all()
    H, W = hm.shape[2:]
    for t in tab:
        mx, my = int(t[8]), int(t[9])
        if t[2] == 0 or not (0 <= mx < W and 0 <= my < H):
            continue
        v = hm[int(t[0]), int(t[1]), my, mx]
        assert v == np.float32(1.0) or (t[3] != 0 and v >= np.float32(0.9999)), (t[:4], v)
        if t[3] == 0:
            assert v == np.float32(1.0)
    return int(d.max(initial=0))


def fixture_bar(g, name):
    """max(4 x the stored fp32-vs-fp64 distance, 1e-5 relative) per loss item: (f64 items, bar)."""
    f32, f64 = g[name + '/items_f32'], g[name + '/items_f64']
    return f64, np.maximum(4 * np.abs(f32 - f64), 1e-5 * np.abs(f64))


def check_items_against_fixture(items, g, name):
    f64, bar = fixture_bar(g, name)
    assert (np.isnan(items) == np.isnan(f64)).all(), (items, f64)
    ok = ~np.isnan(f64)
    err = np.abs(items.astype(np.float64) - f64)
    assert (err[ok] <= bar[ok]).all(), (name, err, bar)
    return (err[ok] / np.abs(f64[ok])).max()
