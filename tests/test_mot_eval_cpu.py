"""CPU: the yardstick of the tracking evaluation (tests/mot_eval_ref.py) pinned by hand-computed cases, and the host parts of
rtm3d_amd/mot_eval.py and kitti_results.py: file round trip, duplicate ids, closing formulas, the KITTI preprocessing decision."""
import numpy as np
import pytest

from rtm3d_amd import kitti_results, mot_eval
from tests import kitti_eval_ref
from tests import mot_eval_cases as mc
from tests import mot_eval_ref as ref
from tests import mot_eval_regimes as mr
from tests import track_assign_ref as ar


def both(a, thr=0.5):
    h = ref.hota(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'])
    c = ref.clear(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], thr)
    return h, ref.hota_metrics(h), c, ref.clear_metrics(c)


def test_perfect_tracker():
    h, hm, c, cm = both(mr.hand('perfect'))
    assert all(np.array_equal(v, np.ones(19)) for v in hm.values())
    assert cm['MOTA'] == 1.0 and cm['MOTP'] == 1.0 and cm['IDSW'] == 0 and cm['Frag'] == 0 and cm['MT'] == 2 and (cm['TP'], cm['FN'], cm['FP']) == (10, 0, 0)


def test_ids_that_swap_halfway():
    h, hm, c, cm = both(mr.hand('swap_halfway'))
    # every pair (g, t) is matched in 2 of the 4 frames both ids live: assa = 2 / (4 + 4 - 2) = 1 / 3; AssA = 4 * 2 * (1 / 3) / 8
    assert np.array_equal(h['potential'][0], np.full((2, 2), 2.0)) and np.array_equal(h['mc'][0, 7], np.full((2, 2), 2))
    assert np.array_equal(hm['DetA'], np.ones(19)) and np.allclose(hm['AssA'], 1.0 / 3.0, rtol=0, atol=1e-15)
    assert np.allclose(hm['HOTA'], np.sqrt(1.0 / 3.0), rtol=0, atol=1e-15) and np.allclose(hm['AssRe'], 0.5) and np.allclose(hm['AssPr'], 0.5)
    assert cm['IDSW'] == 2 and cm['MOTA'] == (8 - 0 - 2) / 8 and cm['Frag'] == 0 and cm['TP'] == 8


@pytest.mark.parametrize('new_id', [False, True])
def test_track_lost_for_two_frames(new_id):
    h, hm, c, cm = both(mr.hand('lost_new_id' if new_id else 'lost_same_id'))
    assert cm['Frag'] == 1 and cm['IDSW'] == (1 if new_id else 0) and (cm['TP'], cm['FN'], cm['FP']) == (10, 2, 0)
    assert c['frag'][0].tolist() == [2, 1] and c['matched'][0].tolist() == [4, 6] and c['idcount'][0].tolist() == [6, 6]
    assert abs(cm['MOTP'] - (4 * 0.9 + 6 * 0.8) / 10) < 1e-14


def test_empty_frames_leave_the_carried_state_alone():
    # frame 4: tracker 1 overlaps better than tracker 0, but tracker 0 held the ground truth in the last PROCESSED frame (frame 0)
    h, hm, c, cm = both(mr.hand('empty_frames'))
    assert c['clear_match'][4, 0] == 1 and cm['IDSW'] == 0 and cm['Frag'] == 0 and c['frag'][0, 0] == 1
    assert (cm['TP'], cm['FN'], cm['FP']) == (2, 1, 2) and abs(c['simsum'][0] - 1.3) < 1e-15
    assert h['match'][4, 0] in (0, 1) and h['gcount'][0, 0] == 3 and h['tcount'][0].tolist() == [2, 2]
    # the frame in which the tracker is empty counts in the ground truth's life, as it does in HOTA's gcount
    assert c['idcount'][0, 0] == 3 and c['matched'][0, 0] == 2 and (cm['MT'], cm['PT'], cm['ML']) == (0, 1, 0)
    # the same frames with the gap PROCESSED (another pair keeps the tracker non-empty): prev is cleared, the better overlap wins
    b = mr.hand('gap_processed')
    c2 = ref.clear(b['sim'], b['ng'], b['nt'], b['gid'], b['tid'], b['seq_start'])
    assert c2['clear_match'][2, 0] == 0 and c2['counts'][0, 3] == 1 and c2['frag'][0, 0] == 2


def test_frames_with_an_empty_tracker_count_in_the_life_of_an_object():
    # present for 10 frames, matched in 2, the tracker empty in the other 8: 2 of 10, not 2 of 2 - never "mostly tracked".  2 / 10 is
    # ">= 0.2", which test_mt_pt_ml_boundaries pins as partly tracked; with one more empty frame (2 of 11) the object is mostly lost
    h, hm, c, cm = both(mr.hand('empty_tracker_8_of_10'))
    assert c['idcount'][0, 0] == 10 and c['matched'][0, 0] == 2 and h['gcount'][0, 0] == 10
    assert (cm['MT'], cm['PT'], cm['ML']) == (0, 1, 0) and (cm['TP'], cm['FN'], cm['FP'], cm['IDSW'], cm['Frag']) == (2, 8, 0, 0, 0)
    h, hm, c, cm = both(mr.hand('empty_tracker_9_of_11'))
    assert c['idcount'][0, 0] == 11 and c['matched'][0, 0] == 2 and (cm['MT'], cm['PT'], cm['ML']) == (0, 0, 1)
    assert (cm['TP'], cm['FN'], cm['FP'], cm['IDSW'], cm['Frag']) == (2, 9, 0, 0, 0) and abs(cm['MOTP'] - 0.7) < 1e-15


def test_mt_pt_ml_boundaries():
    o = dict(counts=np.array([[30, 5, 2, 1]]), simsum=np.array([24.0]),
             idcount=np.array([[10, 10, 5, 10, 0, 5]]), matched=np.array([[8, 9, 1, 1, 0, 5]]), frag=np.array([[3, 1, 0, 2, 0, 1]]))
    want = dict(MT=2, PT=2, ML=1, Frag=3, IDSW=1, TP=30, FN=5, FP=2, MOTA=27 / 35, MOTP=0.8, Recall=30 / 35, Precision=30 / 32)
    for got in (ref.clear_metrics(o), mot_eval.clear_metrics(o['counts'], o['simsum'], o['idcount'], o['matched'], o['frag'])):
        assert got == want                 # 8 / 10 is not "> 0.8": partly tracked; 1 / 5 is ">= 0.2": partly tracked; 1 / 10 mostly lost


def test_assign_is_optimal_and_never_matches_a_non_candidate():
    rng = np.random.Generator(np.random.PCG64(5))
    for n, m in ((1, 1), (3, 4), (4, 3), (5, 5)):
        for _ in range(6):
            w = np.where(rng.random((n, m)) < 0.5, rng.random((n, m)), 0.0)
            col, total, _ = ref.assign(w)
            assert abs(total - ar.brute_force(np.where(w > 0, w, np.nan))) < 1e-12
            assert all(w[i, col[i]] > 0 for i in range(n) if col[i] >= 0) and len(set(col[col >= 0])) == int((col >= 0).sum())
    # not "solve the full matrix, then filter": the pair (1, 0) is no candidate and its row stays free instead
    col, total, margin = ref.assign(np.array([[0.9, 0.8], [0.0, 0.7]]))
    assert col.tolist() == [0, 1] and abs(total - 1.6) < 1e-15 and abs(margin - 0.7) < 1e-12
    assert ref.assign(np.array([[0.5, 0.5], [0.5, 0.5]]))[2] == 0.0                        # a tie has no margin
    assert ref.assign(np.zeros((2, 3)))[0].tolist() == [-1, -1]


def test_closing_formulas_on_fixed_counts():
    tp, fn, fp = np.full((2, 19), 6), np.full((2, 19), 2), np.full((2, 19), 4)
    tp[1], fn[1], fp[1] = 0, 0, 0
    mc_ = np.zeros((2, 19, 2, 2), np.int32)
    mc_[0, :, 0, 0], mc_[0, :, 1, 1], mc_[0, :, 0, 1] = 3, 2, 1
    gcount, tcount = np.array([[4, 4], [0, 0]]), np.array([[5, 5], [0, 0]])
    loc = np.zeros((2, 19))
    loc[0] = 4.5
    got = mot_eval.hota_metrics(tp, fn, fp, loc, mc_, gcount, tcount)
    assa = (3 * 3 / 6 + 2 * 2 / 7 + 1 * 1 / 8) / 6
    assert np.allclose(got['DetA'], 0.5, atol=1e-15) and np.allclose(got['DetRe'], 0.75) and np.allclose(got['DetPr'], 0.6, atol=1e-15)
    assert np.allclose(got['AssA'], assa, atol=1e-15) and np.allclose(got['AssRe'], (9 / 4 + 4 / 4 + 1 / 4) / 6, atol=1e-15)
    assert np.allclose(got['AssPr'], (9 / 5 + 4 / 5 + 1 / 5) / 6, atol=1e-15) and np.allclose(got['LocA'], 0.75)
    assert np.allclose(got['HOTA'], np.sqrt(0.5 * assa), atol=1e-15)
    want = ref.hota_metrics(dict(tp=tp, fn=fn, fp=fp, loc=loc, mc=mc_, gcount=gcount, tcount=tcount))
    assert all(np.array_equal(got[k], want[k]) for k in want)
    empty = mot_eval.hota_metrics(np.zeros((1, 19)), np.zeros((1, 19)), np.zeros((1, 19)), np.zeros((1, 19)), np.zeros((1, 19, 1, 1)), [[0]], [[0]])
    assert np.array_equal(empty['LocA'], np.ones(19)) and not empty['HOTA'].any()
    assert np.array_equal(mot_eval.ALPHAS, np.array(ref.ALPHAS)) and mot_eval.ALPHAS[18] == 0.05 + 18 * 0.05


def test_generated_cases_have_a_margin_and_the_host_agrees_with_the_yardstick():
    gt, trk, metric, seed = mc.case('three_seq_bbox')
    a = mc.arrays(gt, trk, 'Car', metric)
    h, c, margin = mc.yardstick(a)
    assert margin >= mc.MARGIN and a['seq_start'].tolist() == [0, 12, 24, 36] and int(a['ng'].max()) <= 8
    assert c['counts'][:, 3].sum() > 0 and c['counts'][:, 1].sum() > 0 and c['counts'][:, 2].sum() > 0
    for s in range(3):                                       # ids are dense per sequence, in order of first appearance
        ids = a['gid'][12 * s:12 * s + 12]
        flat = ids[ids >= 0]
        assert sorted(set(flat.tolist())) == list(range(int(flat.max()) + 1)) and flat[0] == 0
    table = mot_eval.slot_tables(a['gid'], a['ng'], int(a['gid'].max()) + 1)
    f, k = 5, 2
    assert table[f, a['gid'][f, k]] == k and (table[f] >= 0).sum() == a['ng'][f]


def test_tracking_file_round_trip_and_duplicates(tmp_path):
    rng = np.random.Generator(np.random.PCG64(3))
    frames = []
    for f in range(4):
        rows = np.zeros((6, 16))
        rows[:, 0] = [0, 1, 0, 2, 0, 0]
        rows[:, 1:14] = np.round(rng.uniform(-3, 300, (6, 13)), 6)
        rows[:, 14] = [2, 2, 1, 2, 0, 2]
        frames.append((np.array([3, -4, 5, 6, 0, 7]), rows))
    frames[2] = None
    n = kitti_results.write_tracking_file(str(tmp_path / 'res' / '0003.txt'), frames)
    assert n == 9                                            # per frame ids 3, 6, 7: confirmed and 3D-kept
    back = mot_eval.read_tracking_dir(str(tmp_path / 'res'), results=True)
    assert back.names == ['0003'] and len(back.frames[0]) == 4 and len(back.frames[0][2][1]) == 0
    ids, rows = back.frames[0][1]
    assert ids.tolist() == [3, 6, 7] and [r[0] for r in rows] == ['Car', 'Cyclist', 'Car']
    assert rows[1][1:3] == (-1.0, -1.0) and np.array_equal(np.array(rows[1][3:]), frames[1][1][3, 1:14])
    assert kitti_results.write_tracking_file(str(tmp_path / 'all' / '0003.txt'), frames, include_tentative=True) == 12
    assert mot_eval.read_tracking_dir(str(tmp_path / 'all'), results=True).frames[0][0][0].tolist() == [3, 4, 6, 7]
    with open(str(tmp_path / 'res' / '0004.txt'), 'w') as fh:
        fh.write('0 1 Car 0 0 0 1 2 3 4 1 1 1 0 0 5 0\n0 -1 DontCare -1 -1 -10 1 2 3 4 -1 -1 -1 -1000 -1000 -1000 -10\n'
                 '0 -1 DontCare -1 -1 -10 5 6 7 8 -1 -1 -1 -1000 -1000 -1000 -10\n')
    gt = mot_eval.read_tracking_dir(str(tmp_path / 'res'))                                  # 17 fields: a label file; DontCare may repeat
    assert gt.frames[1][0][0].tolist() == [1, -1, -1] and gt.frames[1][0][1][0][15] == 0.0
    with pytest.raises(ValueError, match='0004.txt line 1'):
        mot_eval.read_tracking_dir(str(tmp_path / 'res'), results=True)
    with open(str(tmp_path / 'res' / '0004.txt'), 'a') as fh:
        fh.write('0 1 Car 0 0 0 1 2 3 4 1 1 1 0 0 5 0\n')
    with pytest.raises(ValueError, match='track id .1. stands more than once'):
        mot_eval.read_tracking_dir(str(tmp_path / 'res'))
    t = mot_eval.Tracks()
    t.add('s', 0, [1, 2], [('Car',) + (0.0,) * 15] * 2)
    with pytest.raises(ValueError, match='more than once'):
        t.add('s', 0, [2], [('Car',) + (0.0,) * 15])


def test_preprocessing_rule_on_one_frame():
    def rect(x):
        return (x, 100.0, x + 50.0, 150.0)
    gt = [('Car', 0.0, 0.0, rect(0.0)), ('Van', 0.0, 0.0, rect(100.0)), ('DontCare', -1.0, -1.0, (400.0, 90.0, 470.0, 160.0)),
          ('Car', 0.0, 3.0, rect(200.0)), ('Car', 0.3, 0.0, rect(300.0)), ('Pedestrian', 0.0, 0.0, rect(500.0)), ('Car', 0.0, 2.0, rect(600.0))]
    trk = [('Car', rect(2.0)), ('Car', rect(101.0)), ('Car', rect(203.0)), ('Pedestrian', rect(0.0)), ('Car', rect(410.0)),
           ('Car', rect(700.0)), ('Car', rect(304.0)), ('Car', rect(503.0)), ('Car', rect(445.0))]
    rows = [g for g in gt if g[0] != 'DontCare']
    cols = [t for t in trk if t[0] == 'Car']
    sim = np.array([[kitti_eval_ref.rect_overlap(g[3], t[1], 0) for t in cols] for g in rows])
    keep_g, keep_t, margin = ref.preprocess_frame('Car', gt, trk, sim)
    # kept: the Car at 0 and the one with occlusion 2.  Tracker boxes: on the Van, on the occluded and on the truncated Car: removed;
    # inside the DontCare region by more than half: removed; by 25 of 50 columns = exactly half: stays; matched to the Pedestrian: stays
    assert keep_g == [0, 6] and keep_t == [0, 5, 7, 8]
    # the host's vectorised rule on the same frame
    col = ref.assign(np.where(sim >= 0.5 - ref.EPS, sim, 0.0))[0]
    share = np.array([[max(ref.rect_share(t[1], g[3]) for g in gt if g[0] == 'DontCare') for t in cols]])
    assert share[0, 7] == 0.5 and share[0, 3] > 0.5
    kg, kt = mot_eval.preprocess_keep('Car', np.array([[g[0] for g in rows]]), np.array([[g[2] for g in rows]]), np.array([[g[1] for g in rows]]),
                                      [len(rows)], col[None, :], [len(cols)], len(cols), share)
    assert np.flatnonzero(kg[0]).tolist() == [0, 5] and np.flatnonzero(kt[0]).tolist() == [0, 4, 6, 7]    # rows / columns without DontCare / Pedestrian
    kg, kt = mot_eval.preprocess_keep('Pedestrian', np.array([[g[0] for g in rows]]), np.zeros((1, 6)), np.zeros((1, 6)), [6],
                                      np.full((1, 6), -1), [0], 1, np.zeros((1, 1)))
    assert np.flatnonzero(kg[0]).tolist() == [4] and not kt.any()


def test_device_entry_points_raise_without_a_gpu_tensor():
    with pytest.raises(RuntimeError, match='no CPU path'):
        import torch
        mot_eval.assign(torch.zeros(1, 2, 2, dtype=torch.float64), [2], [2])
    with pytest.raises(ValueError, match='metric'):
        mot_eval.evaluate(mot_eval.Tracks(), mot_eval.Tracks(), metric='giou')
