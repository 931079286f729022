"""CPU: the host pieces of rtm3d_amd/kitti_eval.py - label files, ``clean``, ``thresholds``, ``ap_from_counts`` - against the
plain-loop restatement of tests/kitti_eval_ref.py and hand values; the device part refuses to run without a GPU."""
import numpy as np
import pytest

from rtm3d_amd import kitti_eval as ke
from rtm3d_amd import kitti_results
from tests import kitti_eval_cases as cases
from tests import kitti_eval_ref as ref


def labels(frames):
    return ke._frames_to_labels(list(range(len(frames))), cases.frame_rows(frames))


def test_label_round_trip_through_the_result_writer(tmp_path):
    rng = np.random.Generator(np.random.PCG64(3))
    n = 5
    params = {'class': np.array([0, 1, 2, 0, 7]), 'Ry': rng.uniform(-3, 3, n), 'dimension': rng.uniform(0.5, 4.0, (n, 3)),
              'location': np.stack([rng.uniform(-8, 8, n), rng.uniform(0.5, 1.5, n), rng.uniform(8, 40, n)], 1),
              'K': np.tile(cases.K.reshape(-1), (n, 1)), 'score': rng.uniform(0.1, 1.0, n)}
    assert kitti_results.write_kitti_label_file(str(tmp_path / 'det' / '000003.txt'), params, image_size=cases.IMAGE) == n
    kitti_results.write_kitti_label_file(str(tmp_path / 'det' / '000001.txt'), None)
    lab = ke.read_label_dir(str(tmp_path / 'det'), ['000001', '000002', '000003'], results=True)       # 000002: no file
    assert lab.n.tolist() == [0, 0, n] and lab.cap == n
    vals = kitti_results.kitti_label_values(params, cases.IMAGE)
    assert lab.type[2].tolist() == ['Car', 'Pedestrian', 'Cyclist', 'Car', 'DontCare']
    assert np.all(lab.truncation[2] == -1) and np.all(lab.occlusion[2] == -1)
    two = lambda a: np.array([float('%.2f' % v) for v in np.ravel(a)]).reshape(np.shape(a))           # noqa: E731
    assert np.array_equal(lab.alpha[2], two(vals[:, 1])) and np.array_equal(lab.rect[2], two(vals[:, 2:6]))
    assert np.array_equal(lab.hwl[2], two(vals[:, 6:9])) and np.array_equal(lab.xyz[2], two(vals[:, 9:12]))
    assert np.array_equal(lab.ry[2], two(vals[:, 12]))
    assert np.array_equal(lab.score[2], np.array([float('%.4f' % v) for v in vals[:, 13]]))
    assert ke.read_label_dir(str(tmp_path / 'det'), results=True).frame_ids == ['000001', '000003']
    # ground-truth lines (15 fields) and the errors
    gt, _ = cases.split(n_frames=2)
    cases.write_dir(str(tmp_path / 'gt'), gt, results=False)
    g = ke.read_label_dir(str(tmp_path / 'gt'))
    want = labels(gt)
    for f in ke.Labels.FIELDS:
        assert np.array_equal(getattr(g, f), getattr(want, f)), f
    assert g.n.tolist() == [len(fr) for fr in gt] and not g.score.any()
    with pytest.raises(FileNotFoundError):
        ke.read_label_dir(str(tmp_path / 'gt'), ['000007'])
    with pytest.raises(ValueError, match='result line'):                 # a ground-truth line is no result line
        ke.read_label_dir(str(tmp_path / 'gt'), results=True)
    (tmp_path / 'bad').mkdir()
    (tmp_path / 'bad' / '000000.txt').write_text('Car 0 0 0 1 2 3 4 1 1 1 0 0 10 0\nCar 0 0 0 1 2 x 4 1 1 1 0 0 10 0\n')
    with pytest.raises(ValueError, match=r'000000\.txt line 2'):
        ke.read_label_dir(str(tmp_path / 'bad'))


def clean_list():
    """Every branch of ``clean``, each limit on both sides, the neighbouring classes, DontCare, lower-case names."""
    def g(t, occ=0, trunc=0.0, height=50.0):
        o = cases.dontcare_obj([10.0, 20.0, 60.0, 20.0 + height])
        o.update(type=t, occlusion=float(occ), truncation=trunc)
        return o
    gts = [g('Car'), g('car'), g('Van'), g('van'), g('Pedestrian'), g('Person_sitting'), g('person_sitting'), g('Cyclist'), g('cyclist'),
           g('DontCare'), g('dontcare'), g('Truck'), g('Misc'), g('Tram')]
    for t in ('Car', 'Pedestrian', 'Cyclist'):
        gts += [g(t, occ=o) for o in (1, 2, 3)]
        gts += [g(t, trunc=v) for v in (0.15, 0.16, 0.3, 0.31, 0.5, 0.51)]
        gts += [g(t, height=h) for h in (40.0, 39.99, 25.0, 24.99)]
        gts += [g(t, occ=2, trunc=0.5, height=25.0), g(t, occ=1, trunc=0.3, height=25.0)]
    o = g('Car', height=-45.0)                      # |y2 - y1|
    gts.append(o)
    dets = [g(t, occ=-1, trunc=-1, height=h) for t in ('Car', 'car', 'Van', 'Pedestrian', 'Person_sitting', 'Cyclist', 'CYCLIST', 'DontCare')
            for h in (40.0, 39.99, 25.0, 24.99, -30.0)]
    return gts, dets


def test_clean_equals_the_restatement():
    gts, dets = clean_list()
    frames_g, frames_d = [gts, gts[::-1][:7], []], [dets, [], dets[:3]]
    gt, det = labels(frames_g), labels(frames_d)
    seen = set()
    for cls in ('Car', 'Pedestrian', 'Cyclist', 'car'):
        for d, name in enumerate(ke.DIFFICULTIES):
            gflag, dflag, dontcare, n_gt = ke.clean(gt, det, cls, name if cls == 'Car' else d)
            assert gflag.dtype == np.int8 and dflag.dtype == np.int8
            total = 0
            for f in range(3):
                wg, wd, wdc, wn = ref.clean_frame(frames_g[f], frames_d[f], cls, d)
                ng, nd = len(frames_g[f]), len(frames_d[f])
                assert gflag[f, :ng].tolist() == wg and dflag[f, :nd].tolist() == wd, (cls, d, f)
                assert np.all(gflag[f, ng:] == -1) and np.all(dflag[f, nd:] == -1)
                assert np.nonzero(dontcare[f])[0].tolist() == wdc
                total += wn
                seen |= {('g', v) for v in wg} | {('d', v) for v in wd}
            assert n_gt == total and n_gt > 0
    assert seen == {(s, v) for s in 'gd' for v in (-1, 0, 1)}
    # the limits, by hand: occlusion 1 / truncation 0.16 / height 39.99 are out at easy and in at moderate
    car = labels([[gts[0], dict(gts[0], occlusion=1.0), dict(gts[0], truncation=0.16), dict(gts[0], rect=[0.0, 0.0, 9.0, 39.99])]])
    none = labels([[]])
    assert ke.clean(car, none, 'Car', 'easy')[0].tolist() == [[0, 1, 1, 1]]
    assert ke.clean(car, none, 'Car', 'moderate')[0].tolist() == [[0, 0, 0, 0]]


@pytest.mark.parametrize('n_gt', [1, 2, 40, 41, 500])
def test_thresholds_equal_the_restatement(n_gt):
    rng = np.random.Generator(np.random.PCG64(n_gt))
    for n_tp in sorted({0, 1, max(n_gt // 3, 1), n_gt}):                 # fewer and more true positives than sample points
        scores = np.round(rng.random(n_tp), 2)                          # rounded: equal scores occur
        got = ke.thresholds(scores, n_gt)
        want = ref.thresholds(list(scores), n_gt)
        assert got.tolist() == want and len(got) <= 41
        if n_tp == n_gt and n_gt == 500:
            assert len(got) == 41
        if n_tp:
            assert got[0] == scores.max() and np.all(np.diff(got) <= 0)
    assert len(ke.thresholds([0.5, 0.4], 0)) == 0 and len(ke.thresholds([], 7)) == 0


def test_ap_from_counts_hand_values():
    assert ke.ap_from_counts([], []) == (0.0, 0.0)
    assert ke.ap_from_counts(np.ones(41), np.zeros(41)) == (100.0, 100.0)
    # precision 1 at the first 21 thresholds, nothing after: p[0::4] has 6 ones of 11, p[1:41] has 20 of 40
    r11, r40 = ke.ap_from_counts([5] * 21, [0] * 21)
    assert r11 == pytest.approx(100.0 * 6 / 11, abs=1e-12) and r40 == 50.0
    # the running maximum from the right lifts the dip at k = 1; tp + fp == 0 counts as 0
    r11, r40, a11, a40 = ke.ap_from_counts([1, 1, 3, 0], [0, 3, 1, 0], [1.0, 0.5, 1.5, 0.0])
    p = [1.0, 0.75, 0.75] + [0.0] * 38
    assert r11 == pytest.approx(100.0 * 1.0 / 11, abs=1e-12) and r40 == pytest.approx(100.0 * 1.5 / 40, abs=1e-12)
    assert (r11, r40) == pytest.approx(ref.average_precision(p), abs=1e-12)
    assert (a11, a40) == pytest.approx(ref.average_precision([1.0, 0.125, 0.375, 0.0]), abs=1e-12)
    with pytest.raises(ValueError):
        ke.ap_from_counts(np.ones(42), np.ones(42))


def test_from_rows_keeps_the_flag_2_rows():
    _, det = cases.split(n_frames=3)
    rows = cases.kitti_rows(det, 40)
    lab = ke.from_rows(rows, ['a', 'b', 'c'])
    want = labels(det)
    assert lab.frame_ids == ['a', 'b', 'c'] and lab.n.tolist() == want.n.tolist()
    for f in ke.Labels.FIELDS:
        assert np.array_equal(getattr(lab, f), getattr(want, f)), f
    rows[0, 0, 14] = 1.0                                                # not kept: no detection
    assert ke.from_rows(rows).n[0] == want.n[0] - 1


def test_evaluate_needs_the_gpu():
    gt, det = cases.split(n_frames=2)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ke.evaluate(labels(gt), labels(det), device='cpu')
    import torch
    with pytest.raises(RuntimeError, match='no CPU path'):
        ke.rect_overlaps(torch.zeros(1, 2, 4, dtype=torch.float64), torch.zeros(1, 2, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ke.Evaluator(labels(gt), device='cpu').result()
