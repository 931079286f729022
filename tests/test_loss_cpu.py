"""CPU (-m "not gpu"): the validation-loss rule.  tests/loss_ref.py - the numpy restatement the device is tested against -
is checked here against the reference-run fixture tests/golden/loss_cases.npz (tests/golden/make_loss_golden.py), together
with the host side of rtm3d_amd.loss: class mapping, refusals, validation of a batch before anything is launched."""
import numpy as np
import pytest

from rtm3d_amd import loss as L
from tests import loss_cases as lc, loss_ref as ref
from tests.util import load_golden

restated, check_heatmap, check_items_against_fixture = lc.restated, lc.check_heatmap, lc.check_items_against_fixture


@pytest.mark.parametrize('name', lc.FIXTURE_CASES)
def test_restatement_matches_the_reference_run(name):
    """Per-object fields and R exactly equal; m_hm equal after rounding to fp32 (<= 1 ulp where the exps differ; measured: 0
    ulp on every case); the five losses within max(4 x |fp32 run - fp64 run| of the reference, 1e-5 relative) of its fp64 run.
    Measured: the reference's own fp32-vs-fp64 distance is 1e-9 .. 1.1e-7 relative on these cases (largest on the vertex_off
    term of fx_b1, 1.07e-7, and the total of fx_b5_odd, 9.6e-8), the restatement's distance to the fp64 run at most 9.8e-8
    relative (fx_pow; 4.4e-8, 7.9e-8, 3.9e-8, 5.6e-8 on the others), so the 1e-5 relative arm of the bar is the one that binds.
    The fixture's v_* fields and mask_3d are what the reference's _build_targets made of corners projected by the reference's
    calc_proj_corners / create_corners (the devkit module its dataset calls is not in its tree): a matrix product where the rule
    has a fixed scalar order, so v_proj, v_mask and mask_3d are equal but v_off and v_coor_off agree to 1e-9 (measured 7.1e-15), not bit for bit."""
    g = load_golden('loss_cases.npz')
    c, b, tab, hm, items, counts = restated(name)
    N = len(tab)
    np.testing.assert_array_equal(tab[:, 6:8], g[name + '/centers'].reshape(N, 2))
    np.testing.assert_array_equal(tab[:, 8:10], g[name + '/m_proj'].reshape(N, 2))
    np.testing.assert_array_equal(tab[:, 10:12], g[name + '/m_off'].reshape(N, 2))
    np.testing.assert_array_equal(tab[:, 13], g[name + '/sigma'])
    np.testing.assert_array_equal(tab[:, 14], g[name + '/radius'])
    np.testing.assert_array_equal(tab[:, 32:48].reshape(N, 8, 2), g[name + '/v_proj'].reshape(N, 8, 2))
    np.testing.assert_allclose(tab[:, 48:64].reshape(N, 8, 2), g[name + '/v_off'].reshape(N, 8, 2), rtol=0, atol=1e-9)
    np.testing.assert_allclose(tab[:, 64:80].reshape(N, 8, 2), g[name + '/v_coor_off'].reshape(N, 8, 2), rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(tab[:, 80:88] != 0, g[name + '/v_mask'].reshape(N, 8))
    np.testing.assert_array_equal(tab[:, 4] != 0, g[name + '/mask_3d'].reshape(N))
    if N:
        print(name, 'v_off', np.abs(tab[:, 48:64].reshape(N, 8, 2) - g[name + '/v_off']).max(), 'v_coor_off', np.abs(tab[:, 64:80].reshape(N, 8, 2) - g[name + '/v_coor_off']).max())
    worst = check_heatmap(hm, g[name + '/m_hm'].astype(np.float32), tab)
    rel = check_items_against_fixture(items, g, name)
    print(name, 'm_hm ulp', worst, 'items rel', rel, 'counts', counts)
    if name == 'fx_none':
        assert counts.tolist() == [0, 0, 0, 0, 0] and np.isnan(items[1:]).all() and np.isfinite(items[0])
    else:
        assert counts[0] > 0 and counts[1] > 0 and counts[3] > 0 and counts[4] == 0


def test_regime_cases_hold_what_they_are_named_for():
    """The regime cases of the GPU tests reach the branches they are built for (checked on the restatement)."""
    c, b, tab, hm, items, counts = restated('borders')
    assert hm[0, 0, 0, 0] == 1 and hm[0, 1, 12, 36] == 1 and (tab[:, 14] >= 2).all()
    c, b, tab, hm, items, counts = restated('noise')
    assert hm[0, 1, 6, 10] == np.float32(0.9999) and hm[1, 2, 7, 20] == 1 and counts[0] == 2
    c, b, tab, hm, items, counts = restated('ignored')
    assert counts[0] == 2 and counts[3] == 2 and hm[0, :, 9, 30].max() == 0
    c, b, tab, hm, items, counts = restated('vertices')
    assert (tab[0, 80:88] == 0).any() and tab[0, 4] == 1                      # corners outside the map
    v = tab[1, 16:32].reshape(8, 2)
    j = int(np.argmin(v[:, 0]))
    assert -1 < v[j, 0] < 0 and tab[1, 32 + 2 * j] == 0 and tab[1, 48 + 2 * j] < 0 and tab[1, 80 + j] == 1
    assert tab[2, 4] == 0 and tab[3, 4] == 1                                  # corners behind the camera
    c2, b2, tab2, hm2, items2, counts2 = restated('vertices_mask3d')
    assert tab2[:, 4].tolist() == [0, 1, 1, 0] and counts2[1] != counts[1] and np.array_equal(tab2[:, 5:], tab[:, 5:])
    c, b, tab, hm, items, counts = restated('zero_size')
    assert tab[:, 14].tolist() == [0, 0] and (hm != 0).sum() == 2 and sorted(hm[hm != 0].tolist()) == [np.float32(0.9999), 1.0]
    c, b, tab, hm, items, counts = restated('huge')
    assert tab[0, 14] > c['W'] and (hm[0, 1] > 0).all()
    c, b, tab, hm, items, counts = restated('outside')
    assert counts[4] == 4 and counts[3] == 2 and ((tab[:, 6] < 0) & (tab[:, 6] > -1) & (tab[:, 8] == 0) & (tab[:, 5] == 1)).sum() == 1
    c, b, tab, hm, items, counts = restated('many')
    n0 = int(b.img_start[1])
    assert n0 == 150 and n0 > 128 and n0 % 64 != 0


def test_class_mapping():
    """_transform_obj_label: Person_sitting doubles into a noise row of Pedestrian and one of Cyclist; Van / Truck become noise
    Cars; DontCare / Tram / Misc become cls -1 (mask 0)."""
    types = ['Car', 'Person_sitting', 'Van', 'DontCare', 'Cyclist', 'Truck', 'Tram', 'Pedestrian']
    cls, noise, rep = L.transform_obj_label(types, L.DEFAULTS[('DATASET', 'OBJs')], L.DEFAULT_RELATE_OBJS)
    assert cls.tolist() == [0, 1, 2, 0, -1, 2, 0, -1, 1] and noise.tolist() == [0, 1, 1, 1, 0, 0, 1, 0, 0]
    assert rep == [1, 2, 1, 1, 1, 1, 1, 1]
    rows = [[('Person_sitting', 0, 0, 0.1, 100., 50., 140., 90., 1.2, 0.6, 0.8, 1., 1.5, 12., 0.2), ('DontCare', -1, -1, -10, 5., 5., 20., 20., -1, -1, -1, -1000, -1000, -1000, -10)],
            [('Car', 0, 0, 0.1, 200., 60., 260., 100., 1.5, 1.6, 3.9, -2., 1.6, 20., -1.0, 0.9)]]
    K = np.array([[[700., 0, 600.], [0, 700., 180.], [0, 0, 1.]]] * 2)
    b = L.LabelBatch.from_kitti(rows, K, None, scale=(0.5, 0.25), pad=(8.0, 3.0), mask_3d=[[1, 0], [1]])
    assert b.N == 4 and b.B == 2 and b.img_start.tolist() == [0, 3, 4]
    assert b.rows[:, 1].tolist() == [1, 2, -1, 0] and b.rows[:, 2].tolist() == [1, 1, 0, 0] and b.rows[:, 16].tolist() == [1, 1, 0, 1]
    assert b.rows[0, 3:7].tolist() == [58.0, 15.5, 78.0, 25.5] and np.array_equal(b.rows[0, 3:13], b.rows[1, 3:13])
    assert b.K[0].tolist() == [350., 0, 308., 0, 175., 48., 0, 0, 1.]
    assert np.array_equal(b.rows[:, 14], np.sin(b.rows[:, 13])) and np.array_equal(b.rows[:, 15], np.cos(b.rows[:, 13]))
    # a custom class list
    cfg = {'DATASET': {'OBJs': ['Cyclist', 'Car'], 'RELATE_OBJs': [[], ['Van']]}}
    cls, noise, _ = L.transform_obj_label(['Car', 'Van', 'Pedestrian'], cfg['DATASET']['OBJs'], cfg['DATASET']['RELATE_OBJs'])
    assert cls.tolist() == [1, 1, -1] and noise.tolist() == [0, 1, 0]
    assert L.LabelBatch.from_kitti(rows, K, cfg).num_classes == 2
    from rtm3d_amd import kitti_eval
    lab = kitti_eval._frames_to_labels([0, 1], [[list(r) + [0.0] * (16 - len(r)) for r in f] for f in rows])
    assert np.array_equal(L.LabelBatch.from_kitti(lab, K).rows, L.LabelBatch.from_kitti(rows, K).rows)


def test_dynamic_sigma_is_refused_by_name():
    cfg = {'DATASET': {'GAUSSIAN_GEN_TYPE': 'dynamic_sigma'}}
    for make in (lambda: L.RTM3DLoss(cfg), lambda: L.ValidationLoss(cfg), lambda: L.LabelBatch.from_kitti([[]], np.eye(3)[None], cfg)):
        with pytest.raises(NotImplementedError, match='GAUSSIAN_GEN_TYPE'):
            make()
    L.RTM3DLoss({'DATASET': {'GAUSSIAN_GEN_TYPE': 'dynamic_radius'}})
    import rtm3d_amd
    lo = L.RTM3DLoss(rtm3d_amd.kitti_config('DLA-34'))                       # the keys the tree lacks: the reference's defaults
    assert (lo.alpha, lo.beta, lo.weights) == (2.0, 4.0, (1.0, 1.0, 0.5, 0.5))
    lo = L.RTM3DLoss({'TRAINING': {'W_VFM': 2.0}, 'MODEL': {'FOCAL_LOSS_BEDA': 3.0}})
    assert (lo.alpha, lo.beta, lo.weights) == (2.0, 3.0, (1.0, 2.0, 0.5, 0.5))
    with pytest.raises(ValueError, match='FOCAL_LOSS'):
        L.RTM3DLoss({'MODEL': {'FOCAL_LOSS_ALPHA': 0.0}})


def test_batch_is_validated_on_the_host_before_anything_is_launched():
    """Every refusal is a ValueError raised by the constructor: no device, no library call (this test runs without a GPU)."""
    c = lc.make('fx_b1')
    good = dict(B=c['B'], img_id=c['img_id'], cls=c['cls'], noise=c['noise'], bbox=c['bbox'], dimension=c['dim'], location=c['loc'],
                Ry=c['ry'], K=c['K'])
    assert L.LabelBatch(**good).N == len(c['cls'])

    def bad(match, **kw):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            L.LabelBatch(**a)

    bad('img_id', img_id=np.where(np.arange(len(c['cls'])) == 2, 1, c['img_id']))                 # outside 0..B-1
    bad('non-decreasing', B=2, img_id=np.array([0, 1] + [0] * (len(c['cls']) - 2)), K=np.tile(c['K'], (2, 1)))
    bad('cls', cls=np.where(np.arange(len(c['cls'])) == 1, 3, c['cls']))
    bad('cls', cls=c['cls'] + 0.5)
    bad('noise', noise=c['noise'] + 2)
    bad('not finite', bbox=np.where(np.arange(4) == 1, np.nan, c['bbox']))
    bad('not finite', location=c['loc'] * np.inf)
    bad('bbox coordinate', bbox=c['bbox'] * 1e7)
    bad('x2 < x1', bbox=c['bbox'][:, [2, 1, 0, 3]] + np.array([1.0, 0, 0, 0]))
    bad('y2 < y1', bbox=c['bbox'][:, [0, 3, 2, 1]] + np.array([0, 1.0, 0, 0]))
    bad('shape', dimension=c['dim'][:, :2])
    bad('K', K=c['K'][:, :8])
    bad('K', K=c['K'] * np.nan)
    bad('mask_3d', mask_3d=np.full(len(c['cls']), 2.0))
    bad('down_sample', down_sample=0.0)
    bad('B =', B=0)
    with pytest.raises(ValueError, match='15 fields'):
        L.LabelBatch.from_kitti([[('Car', 0, 0)]], np.eye(3)[None])
    with pytest.raises(ValueError, match='mask_3d'):
        L.LabelBatch.from_kitti([[('Car', 0, 0, 0, 1, 1, 2, 2, 1, 1, 1, 0, 1, 9, 0)]], np.eye(3)[None], mask_3d=[[1, 0]])
    with pytest.raises(RuntimeError, match='CUDA'):
        L.LabelBatch(**good).to('cpu')
    with pytest.raises(TypeError, match='LabelBatch'):
        L.RTM3DLoss()([None] * 4, object())
