"""GPU: rtm3d_rect_overlaps and rtm3d_kitti_match (csrc/kitti_eval.hip) and the protocol of rtm3d_amd/kitti_eval.py against
the plain-loop restatement of tests/kitti_eval_ref.py, which walks the detections sequentially as the devkit states it.

Bars: rectangle overlaps bit-equal to the same numpy expression (one fp64 operation order, no contraction on either side);
tp / fp / fn, thresholds and the scores of the true positives exactly equal; similarity within 1e-9 relative (fp64 sums of at
most 1e6 terms in [0, 1] in any order differ by less than n * 2^-53 ~ 1e-10); AP / AOS within 1e-9.

Measured on the MI355X: largest AP / AOS disagreement with the restatement 4.3e-14; similarity equal in the matching cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib                           # noqa: E402
from rtm3d_amd import kitti_eval as ke               # noqa: E402
from tests import kitti_eval_cases as cases          # noqa: E402
from tests import kitti_eval_ref as ref              # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_RTOL = 1e-9
AP_TOL = 1e-9


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def labels(frames):
    return ke._frames_to_labels(['%06d' % f for f in range(len(frames))], cases.frame_rows(frames))


# ------------------------------------------------------------------------------------------------ 1. rectangle overlaps
def test_rect_overlaps_are_bit_equal_to_numpy(dev):
    rng = np.random.Generator(np.random.PCG64(11))
    B, ca, cb = 5, 70, 9                                              # more than one block, no multiple of it
    xy = rng.uniform(0, 100, (B, ca + cb, 2))
    r = np.concatenate([xy, xy + rng.uniform(1, 60, (B, ca + cb, 2))], 2)
    a, b = r[:, :ca].copy(), r[:, ca:].copy()
    b[0, 0] = [10, 10, 20, 20]
    a[0, :8] = [[20, 10, 30, 20],          # touching along an edge
                [20, 20, 30, 30],          # touching at a corner
                [12, 12, 18, 18],          # nested in b
                [0, 0, 40, 40],            # b nested in a
                [10, 10, 20, 20],          # identical
                [15, 15, 15, 25],          # zero width
                [15, 15, 15, 15],          # a point
                [np.nan, 10, 20, 20]]      # NaN
    b[0, 1] = [14, 14, 14, 14]             # a zero-area rectangle on the other side
    b[0, 2] = [10, np.nan, 20, 20]
    b[0, 3] = [12, 12, np.inf, 18]
    a[1, 0] = [30, 30, 10, 10]             # inverted
    na = np.array([ca, ca - 3, 1, 0, 64], np.int32)
    nb = np.array([cb, 2, cb, cb, 0], np.int32)
    ta, tb, tna, tnb = (torch.from_numpy(v).to(dev) for v in (a, b, na, nb))
    for crit, name in enumerate(('iou', 'a', 'b')):
        got = ke.rect_overlaps(ta, tb, tna, tnb, name).cpu().numpy()
        want = ref.rect_overlaps_numpy(a, b, na, nb, crit)
        assert got.shape == (B, ca, cb) and np.isfinite(got).all()
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        for i in range(8):                                           # and the loop form of the rule on the hand cases
            for j in range(4):
                if np.isfinite(a[0, i]).all() and np.isfinite(b[0, j]).all():
                    assert got[0, i, j] == ref.rect_overlap(a[0, i], b[0, j], crit), (name, i, j)
        assert (got[0] > 0).sum() > 50 and not got[3].any() and not got[4].any()
        assert not got[0, 7].any() and not got[0, :, 2].any() and not got[0, :, 3].any()      # NaN / infinite rectangles overlap nothing
    iou = ke.rect_overlaps(ta, tb, tna, tnb).cpu().numpy()[0]
    assert iou[0, 0] == 0 and iou[1, 0] == 0 and iou[4, 0] == 1.0 and iou[2, 0] == 0.36 and iou[5, 0] == 0 and iou[6, 1] == 0
    assert ke.rect_overlaps(ta, tb, tna, tnb, 'a').cpu().numpy()[0, 2, 0] == 1.0
    with pytest.raises(RuntimeError, match='criterion'):
        _lib.check(_lib.load().rtm3d_rect_overlaps(None, 1, 1, 1, tna.data_ptr(), tnb.data_ptr(), ta.data_ptr(), tb.data_ptr(), 3,
                                                   ta.data_ptr()), 'rect_overlaps')


# ------------------------------------------------------------------------------------------------ 2. the matching
def upload(c, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items() if isinstance(v, np.ndarray)}


def match_reference(c):
    """The restatement on one case: (true-positive score lists per item, counts (G, T, 3), similarity (G, T))."""
    F, G = len(c['nd']), len(c['min_overlap'])
    tps = {}
    counts = np.zeros((G, c['thr'].shape[1], 3), np.int64)
    sim = np.zeros((G, c['thr'].shape[1]))
    for f in range(F):
        nd, ng = int(c['nd'][f]), int(c['ng'][f])
        ov = c['overlap'][f, :nd, :ng].tolist()
        sc = c['score'][f, :nd].tolist()
        for g in range(G):
            gf, df = c['gflag'][f, g, :ng].tolist(), c['dflag'][f, g, :nd].tolist()
            mo = float(c['min_overlap'][g])
            tps[(f, g)] = ref.match_frame(ov, gf, df, sc, mo)
            for k in range(int(c['nthr'][g])):
                r = ref.match_frame(ov, gf, df, sc, mo, thresh=float(c['thr'][g, k]), dc_ov=[[2.0 * v] for v in c['dc_hit'][f, g, :nd].tolist()],
                                    alpha_g=c['alpha_g'][f, :ng].tolist(), alpha_d=c['alpha_d'][f, :nd].tolist())
                counts[g, k] += r[:3]
                sim[g, k] += r[3]
    return tps, counts, sim


@pytest.mark.parametrize('n_g', cases.MATCH_NG)
@pytest.mark.parametrize('n_d', cases.MATCH_ND)
def test_matching_equals_the_sequential_restatement(dev, n_d, n_g):
    c = cases.match_case(n_d, n_g)
    want_tps, want_counts, want_sim = match_reference(c)
    t = upload(c, dev)
    F, G = len(c['nd']), len(c['min_overlap'])
    ms = ke.match_scores(t['nd'], t['ng'], t['gflag'], t['dflag'], t['score'], t['overlap'], t['min_overlap']).cpu().numpy()
    assert ms.shape == (F, G, c['cap_g'])
    n_tp = 0
    for f in range(F):
        for g in range(G):
            got = [(int(i), float(ms[f, g, i])) for i in np.nonzero(ms[f, g] != -np.inf)[0]]
            assert got == want_tps[(f, g)], (f, g, got, want_tps[(f, g)])
            n_tp += len(got)
    assert not np.isnan(ms).any()
    tp, fp, fn, sim = ke.match_counts(t['nd'], t['ng'], t['gflag'], t['dflag'], t['score'], t['overlap'], t['min_overlap'], t['nthr'], t['thr'],
                                      dc_hit=t['dc_hit'], alpha_g=t['alpha_g'], alpha_d=t['alpha_d'])
    got_counts = torch.stack([tp, fp, fn], 2).cpu().numpy()
    for g in range(G):
        n = int(c['nthr'][g])
        assert np.array_equal(got_counts[g, :n], want_counts[g, :n]), (g, got_counts[g, :n], want_counts[g, :n])
        assert not got_counts[g, n:].any()
    sim = sim.cpu().numpy()
    assert sim.shape == (F, G, c['thr'].shape[1]) and np.isfinite(sim).all()
    got_sim = sim.sum(0)
    print('n_d %d n_g %d: %d true positives in scores mode, counts %s, similarity error %.3g'
          % (n_d, n_g, n_tp, want_counts.sum((0, 1)).tolist(), np.abs(got_sim - want_sim).max()))
    assert np.all(np.abs(got_sim - want_sim) <= SIM_RTOL * np.maximum(np.abs(want_sim), 1e-300) + 0.0), (got_sim, want_sim)
    if n_d >= 63 and n_g >= 5:                                       # the case is not empty: every outcome occurs
        assert n_tp > 0 and (want_counts.sum((0, 1)) > 0).all()
    # a second chunk adds to the counts; without the DontCare flags no false positive is removed; without angles no similarity
    tp2, fp2, fn2, sim0 = ke.match_counts(t['nd'], t['ng'], t['gflag'], t['dflag'], t['score'], t['overlap'], t['min_overlap'], t['nthr'], t['thr'],
                                          counts=(tp.clone(), fp.clone(), fn.clone()))
    assert torch.equal(tp2, 2 * tp) and torch.equal(fn2, 2 * fn) and bool((fp2 >= 2 * fp).all()) and not sim0.any()


def test_matching_refuses_more_than_256_detections(dev):
    F, G, cap_d, cap_g = 1, 1, 257, 2
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)          # noqa: E731
    with pytest.raises(RuntimeError, match='cap_d 257 is more than the 256'):
        ke.match_scores(z(F, dt=torch.int32), z(F, dt=torch.int32), z(F, G, cap_g, dt=torch.int8), z(F, G, cap_d, dt=torch.int8), z(F, cap_d),
                        z(F, cap_d, cap_g), z(G))
    gt = labels([[cases.dontcare_obj([0, 0, 10, 10])]])
    det = labels([[cases.dontcare_obj([0, 0, 10, 10])] * 257])
    with pytest.raises(ValueError, match='257 detections'):
        ke.evaluate(gt, det, device=dev)


# ------------------------------------------------------------------------------------------------ 3. the whole protocol
def device_overlaps(gt_frames, det_frames, dev):
    """The device's own matrices, as the lists the restatement takes."""
    gt, det = labels(gt_frames), labels(det_frames)
    ov = {k: v.cpu().numpy() for k, v in ke.overlap_matrices(gt, det, dev).items()}
    out = {m: [ov[m][f, :len(det_frames[f]), :len(gt_frames[f])].tolist() for f in range(len(gt_frames))] for m in ke.METRICS}
    ndc = [sum(g['type'] == 'DontCare' for g in fr) for fr in gt_frames]
    dc = [ov['dontcare'][f, :len(det_frames[f]), :ndc[f]].tolist() for f in range(len(gt_frames))]
    return out, dc


@pytest.fixture(scope='module')
def protocol(dev, tmp_path_factory):
    gt_frames, det_frames = cases.split()
    det_frames[5] = []                                               # a frame without detections: no result file
    root = tmp_path_factory.mktemp('kitti')
    cases.write_dir(str(root / 'gt'), gt_frames, results=False)
    cases.write_dir(str(root / 'det'), det_frames, results=True, skip_empty=True)
    assert not os.path.exists(str(root / 'det' / '000005.txt'))
    gt = ke.read_label_dir(str(root / 'gt'))
    det = ke.read_label_dir(str(root / 'det'), gt.frame_ids, results=True)
    res = ke.evaluate(gt, det, device=dev)
    ov, dc = device_overlaps(gt_frames, det_frames, dev)
    want = ref.evaluate(gt_frames, det_frames, cases.SPLIT_CLASSES, ke.MIN_OVERLAP, ov, dc)
    return {'gt_frames': gt_frames, 'det_frames': det_frames, 'root': root, 'gt': gt, 'det': det, 'res': res, 'want': want}


def test_protocol_equals_the_restatement(protocol):
    res, want = protocol['res'], protocol['want']
    assert len(protocol['gt']) == 24
    worst = 0.0
    for (m, c, d), w in sorted(want.items()):
        vals = [w['ap_r11'], w['ap_r40']] + ([w['aos_r11'], w['aos_r40']] if m == 'bbox' else [])
        print(m, c, ke.DIFFICULTIES[d], 'n_gt %d, %d thresholds,' % (w['n_gt'], len(w['thresholds'])), ' '.join('%.3f' % v for v in vals))
        assert all(5.0 < v < 95.0 for v in vals), ('a degenerate split', m, c, d, vals)          # on the restatement alone
        assert res.n_gt[c][d] == w['n_gt']
        assert res.thresholds[m][c][d].tolist() == w['thresholds'], (m, c, d)
        k = res.counts[m][c][d]
        assert k['tp'].tolist() == w['tp'] and k['fp'].tolist() == w['fp'] and k['fn'].tolist() == w['fn'], (m, c, d)
        assert np.allclose(k['similarity'], w['similarity'], rtol=SIM_RTOL, atol=0.0)
        got = [res.ap_r11[m][c][d], res.ap_r40[m][c][d]] + ([res.aos_r11[c][d], res.aos_r40[c][d]] if m == 'bbox' else [])
        worst = max(worst, max(abs(a - b) for a, b in zip(got, vals)))
    print('AP / AOS: largest disagreement with the restatement %.3g (bar %g)' % (worst, AP_TOL))
    assert worst <= AP_TOL
    # the DontCare regions did remove false positives
    plain = ref.evaluate(protocol['gt_frames'], protocol['det_frames'], ('Car',), ke.MIN_OVERLAP,
                         {'bbox': device_overlaps(protocol['gt_frames'], protocol['det_frames'], 'cuda')[0]['bbox']},
                         [[[] for _ in fr] for fr in protocol['det_frames']])
    assert sum(plain[('bbox', 'Car', 2)]['fp']) > sum(want[('bbox', 'Car', 2)]['fp'])
    table = res.table()
    assert 'Car AP_R40@0.70, 0.70, 0.70:' in table and 'Pedestrian AP_R11@0.50, 0.50, 0.50:' in table and table.count('aos  AP:') == 6


def test_rows_and_evaluator_give_the_file_result(protocol, dev):
    want = protocol['res'].to_json()
    rows = torch.from_numpy(cases.kitti_rows(protocol['det_frames'], 40)).to(dev)
    ids = protocol['gt'].frame_ids
    assert ke.evaluate(protocol['gt'], ke.from_rows(rows, ids), device=dev).to_json() == want
    # 24 frames in three chunks, the last one short: the same counts; the similarity is summed in another order
    chunked = ke.evaluate(protocol['gt'], protocol['det'], device=dev, chunk_frames=10).to_json()
    assert chunked['thresholds'] == want['thresholds'] and chunked['ap_r40'] == want['ap_r40'] and chunked['n_gt'] == want['n_gt']
    for m in ke.METRICS:
        for c in want['classes']:
            for a, b in zip(chunked['counts'][m][c], want['counts'][m][c]):
                assert (a['tp'], a['fp'], a['fn']) == (b['tp'], b['fp'], b['fn'])
                assert np.allclose(a['similarity'], b['similarity'], rtol=SIM_RTOL, atol=0.0)
    ev = ke.Evaluator(protocol['gt'], device=dev)
    ev.add_rows(ids[10:], rows[10:])                                 # out of order, in two batches
    ev.add_rows(ids[:10], rows[:10].cpu())
    assert ev.result().to_json() == want
    with pytest.raises(ValueError, match='added before'):
        ev.add_rows(ids[:1], rows[:1])


def test_cli_writes_the_same_json(protocol, tmp_path):
    out = str(tmp_path / 'ap.json')
    r = subprocess.run([sys.executable, '-m', 'rtm3d_amd.kitti_eval', str(protocol['root'] / 'gt'), str(protocol['root'] / 'det'), '--json', out],
                       cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert 'Car AP_R40@0.70, 0.70, 0.70:' in r.stdout
    assert json.load(open(out)) == json.loads(json.dumps(protocol['res'].to_json()))


# ------------------------------------------------------------------------------------------------ 4. analytic checks
def test_analytic_cases(dev):
    gt_frames = cases.analytic_split()
    gt = labels(gt_frames)
    res = ke.evaluate(gt, labels(cases.perfect(gt_frames)), device=dev)
    for c in cases.SPLIT_CLASSES:
        assert res.n_gt[c] == (48, 48, 48)
        for m in ke.METRICS:
            assert res.ap_r40[m][c] == (100.0,) * 3 and res.ap_r11[m][c] == (100.0,) * 3, (m, c, res.ap_r40[m][c])
            assert all(len(t) == 41 for t in res.thresholds[m][c])
        assert res.aos_r40[c] == (100.0,) * 3 and res.aos_r11[c] == (100.0,) * 3
    turned = ke.evaluate(gt, labels(cases.perfect(gt_frames, turn=np.pi)), device=dev)
    for c in cases.SPLIT_CLASSES:
        for m in ke.METRICS:
            assert turned.ap_r40[m][c] == (100.0,) * 3 and turned.ap_r11[m][c] == (100.0,) * 3, (m, c)
        assert max(turned.aos_r40[c] + turned.aos_r11[c]) <= 1e-12 and min(turned.aos_r40[c] + turned.aos_r11[c]) >= 0.0
    none = ke.evaluate(gt, labels([[] for _ in gt_frames]), device=dev)
    extra = ke.evaluate(gt, labels(cases.perfect(gt_frames)), classes=('Car', 'Tram'), min_overlap={'Tram': 0.5}, device=dev)
    assert extra.n_gt['Tram'] == (0, 0, 0) and extra.ap_r40['bbox']['Car'] == (100.0,) * 3
    for c in cases.SPLIT_CLASSES:
        assert none.n_gt[c] == (48, 48, 48)
    for r, cs in ((none, cases.SPLIT_CLASSES), (extra, ('Tram',))):
        for c in cs:
            for m in ke.METRICS:
                assert r.ap_r40[m][c] == (0.0,) * 3 and r.ap_r11[m][c] == (0.0,) * 3
                assert all(len(t) == 0 for t in r.thresholds[m][c])
            assert r.aos_r40[c] == (0.0,) * 3 and r.aos_r11[c] == (0.0,) * 3
    assert 'NaN' not in json.dumps(extra.to_json()) and 'NaN' not in json.dumps(none.to_json())
    with pytest.raises(ValueError, match='min_overlap'):
        ke.evaluate(gt, labels(cases.perfect(gt_frames)), classes=('Tram',), device=dev)
