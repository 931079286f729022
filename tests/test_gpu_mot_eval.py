"""GPU: the tracking evaluation (csrc/mot_eval.hip, rtm3d_amd/mot_eval.py) against the yardstick tests/mot_eval_ref.py.
rtm3d_mot_assign against scipy in every regime of its solver; the HOTA and CLEAR device outputs on generated sequences - integer
outputs EQUAL, fp64 outputs and final metrics within 1e-9 (the bar of the tracker tests), the yardstick's margin >= 1e-6 asserted
first; determinism of the whole evaluator; a Tracker scored end to end, greedy against optimal; the KITTI preprocessing; refusals.

Measured on an MI355X (the figure each case prints; copied to profiles/mot_eval.txt): the largest disagreement of potential, loc,
simsum and of every final metric is 0 in all four generated cases and in the end-to-end cases."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, kitti_eval, mot_eval, track         # noqa: E402
from tests import mot_eval_cases as mc                          # noqa: E402
from tests import mot_eval_ref as ref                           # noqa: E402
from tests import track_assign_ref as ar                        # noqa: E402
from tests import track_cases as tc                             # noqa: E402

TOL = 1e-9
INT_KEYS = ('gcount', 'tcount', 'match', 'tp', 'fn', 'fp', 'mc', 'clear_match', 'counts', 'idcount', 'matched', 'frag')
FLOAT_KEYS = ('potential', 'loc', 'simsum')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------------------------------------------- ASSIGN
def random_w(seed, n, m, density=0.6):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.where(rng.random((n, m)) < density, rng.uniform(0.05, 1.0, (n, m)), 0.0)


def with_margin(first_seed, n, m, edit=None, density=0.6):
    """A score matrix whose optimum is unique by >= MARGIN on the yardstick's own numbers: (w, match, total)."""
    for seed in range(first_seed, first_seed + 50):
        w = random_w(seed, n, m, density)
        if edit:
            edit(w)
        col, total, margin = ref.assign(w)
        if margin >= mc.MARGIN:
            return w, col, total
    raise RuntimeError('no seed gives a %d x %d matrix a margin' % (n, m))


def zero_row(w):
    w[1, :] = 0.0


def zero_col(w):
    w[:, 2] = 0.0


def no_candidate(w):
    w[:] = 0.0


REGIMES = [('1x1', 1, 1, None), ('1x7', 1, 7, None), ('7x1', 7, 1, None), ('more_rows', 9, 5, None), ('more_columns', 5, 9, None),
           ('no_candidate', 4, 6, no_candidate), ('zero_row', 5, 5, zero_row), ('zero_column', 5, 5, zero_col),
           ('63x63', 63, 63, None), ('64x64', 64, 64, None), ('65x65', 65, 65, None), ('64x65', 64, 65, None), ('65x3', 65, 3, None),
           ('256x256', 256, 256, None)]


def device_assign(dev, ws, cap_g, cap_t):
    F = len(ws)
    w = np.zeros((F, cap_g, cap_t))
    ng, nt = np.array([x.shape[0] for x in ws], np.int32), np.array([x.shape[1] for x in ws], np.int32)
    for f, x in enumerate(ws):
        w[f, :x.shape[0], :x.shape[1]] = x
        w[f, x.shape[0]:, :] = 0.9                            # entries beyond ng / nt are never read
        w[f, :, x.shape[1]:] = 0.9
    out = mot_eval.assign(torch.from_numpy(w).to(dev), ng, nt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('name,n,m,edit', REGIMES, ids=[r[0] for r in REGIMES])
def test_assign_equals_scipy(dev, name, n, m, edit):
    w, col, total = with_margin(1000 + 50 * [r[0] for r in REGIMES].index(name), n, m, edit, density=0.6 if n < 100 else 0.2)
    got = device_assign(dev, [w], n + (3 if n < 250 else 0), m + (2 if m < 250 else 0))[0]
    assert np.array_equal(got[:n], col), (name, np.flatnonzero(got[:n] != col)[:8].tolist())
    assert (got[n:] == -1).all()
    got_total = float(sum(w[i, got[i]] for i in range(n) if got[i] >= 0))
    assert abs(got_total - total) <= 1e-9
    print('%s: total %.12g, device - scipy %.3g' % (name, total, got_total - total))


def test_assign_300_frames_of_different_sizes_in_one_launch(dev):
    rng = np.random.Generator(np.random.PCG64(77))
    ws, want = [], []
    for f in range(300):
        n, m = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        if n == 0 or m == 0:
            w, col = np.zeros((n, m)), np.full(n, -1)
        else:
            w, col, _ = with_margin(5000 + 50 * f, n, m)
        ws.append(w)
        want.append(col)
    got = device_assign(dev, ws, 12, 12)
    for f in range(300):
        n = ws[f].shape[0]
        assert np.array_equal(got[f, :n], want[f]) and (got[f, n:] == -1).all(), f


@pytest.mark.parametrize('n,m', [(2, 2), (3, 5), (70, 70)])
def test_assign_exact_ties_are_deterministic_and_optimal(dev, n, m):
    w = np.full((n, m), 0.5)
    w[0, 0] = 0.0
    a, b = device_assign(dev, [w, w], n, m), device_assign(dev, [w, w], n, m)
    assert a.tobytes() == b.tobytes() and np.array_equal(a[0], a[1])
    col = a[0]
    hit = col[col >= 0]
    assert len(set(hit.tolist())) == len(hit) and all(w[i, col[i]] > 0 for i in range(n) if col[i] >= 0)
    assert abs(0.5 * len(hit) - ref.assign(w, with_margin=False)[1]) <= 1e-9


# ------------------------------------------------------------------------------------------------------------ HOTA / CLEAR
def compare(name, got, h, c):
    want = dict(h, **c)
    for k in INT_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:6].tolist())
    worst = 0.0
    for k in FLOAT_KEYS:
        err = float(np.abs(got[k] - want[k]).max())
        worst = max(worst, err)
        assert err <= TOL, (name, k, err)
    return worst


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_device_outputs_equal_the_yardstick(dev, name):
    gt, trk, metric, seed = mc.case(name)
    cpu = mc.arrays(gt, trk, 'Car', metric)
    p = mot_eval.prepare(gt, trk, 'Car', metric, preprocess=False, device=dev)
    for k in ('ng', 'nt', 'gid', 'tid', 'seq_start'):
        assert np.array_equal(p[k], cpu[k]), k
    sim = p['sim'].cpu().numpy()
    assert float(np.abs(sim - cpu["sim"]).max()) <= 1e-9          # the CPU restatement the seeds were chosen on
    h, c, margin = mc.yardstick(dict(p, sim=sim))
    assert margin >= mc.MARGIN, margin                        # on the yardstick's own numbers, from the device's similarities
    got = mot_eval.run_device(p['sim'], p['ng'], p['nt'], p['gid'], p['tid'], p['seq_start'])
    worst = compare(name, got, h, c)
    res = mot_eval.evaluate(gt, trk, classes=('Car',), metric=metric, preprocess=False, device=dev)
    hm, cm = ref.hota_metrics(h), ref.clear_metrics(c)
    for k in mot_eval.HOTA_FIELDS:
        worst = max(worst, float(np.abs(res.hota['Car'][k] - hm[k]).max()), abs(res.hota_mean['Car'][k] - float(np.mean(hm[k]))))
    for k in mot_eval.CLEAR_FIELDS:
        assert isinstance(cm[k], float) or res.clear['Car'][k] == cm[k], k
        worst = max(worst, abs(res.clear['Car'][k] - cm[k]))
    assert worst <= TOL
    assert 'HOTA' in res.table() and res.to_json()['clear']['Car']['IDSW'] == cm['IDSW'] > 0
    print('%s (seed %d, %s): HOTA %.4f MOTA %.4f IDSW %d; largest disagreement of potential / loc / simsum / any metric %.3g (bar %g)'
          % (name, seed, metric, res.hota_mean['Car']['HOTA'], cm['MOTA'], cm['IDSW'], worst, TOL))


def test_the_whole_evaluator_is_deterministic(dev):
    gt, trk, metric, _ = mc.case('many_ids_iou3d')
    runs = []
    for _ in range(2):
        p = mot_eval.prepare(gt, trk, 'Car', metric, preprocess=False, device=dev)
        runs.append(dict(mot_eval.run_device(p['sim'], p['ng'], p['nt'], p['gid'], p['tid'], p['seq_start']), sim=p['sim'].cpu().numpy()))
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


# ------------------------------------------------------------------------------------------------------------- end to end
def rows16(rec):
    """(topk, 16) KITTI rows of one stream's records (the layout of rtm3d_records_to_camera) with a pinhole rectangle."""
    rec = np.asarray(rec, np.float64)
    rows = np.zeros((rec.shape[0], 16))
    for k in np.flatnonzero(rec[:, 31] == 2):
        r = mc.label_row('x', rec[k, 24:31], score=rec[k, 1])
        rows[k, 0], rows[k, 1:14], rows[k, 14] = rec[k, 0], r[3:16], 2.0
    return rows


def run_tracker(case, dev, assignment, identity, names=('Car', 'Pedestrian', 'Cyclist')):
    """(gt, trk): the case's own boxes with their identities as ground truth, the tracker's confirmed output as result."""
    B = case['frames'][0].shape[0]
    t = track.Tracker(B, case['T'], track.TrackParams(**case['params']), dev, assignment=assignment)
    gt, trk = mot_eval.Tracks(), mot_eval.Tracks()
    ev = mot_eval.Evaluator(gt, classes=('Car',), preprocess=False, device=dev, class_names=names)
    for f, rec in enumerate(case['frames']):
        ego = None if case['egos'] is None else torch.from_numpy(case['egos'][f]).to(dev)
        ids = t.update(torch.from_numpy(rec).to(dev), dt=case['dt'], ego=ego).cpu().numpy()
        for b in range(B):
            rows = rows16(rec[b])
            det = np.flatnonzero((rec[b, :, 31] == 2) & (rec[b, :, 1].astype(np.float64) >= case['params']['min_score']))
            gt.add('%04d' % b, f, [identity(b, f, k, rec[b, k]) for k in det],
                   [(names[int(rec[b, k, 0])],) + (0.0, 0.0) + tuple(rows[k, 1:14]) for k in det])
            ev.add_frame('%04d' % b, f, ids[b], rows)
    return gt, ev.trk, ev


def score_both_ways(dev, gt, trk, ev, cls='Car'):
    res = ev.result()
    p = mot_eval.prepare(gt, trk, cls, 'iou3d', preprocess=False, device=dev)
    h, c, margin = mc.yardstick(dict(p, sim=p['sim'].cpu().numpy()))
    hm, cm = ref.hota_metrics(h), ref.clear_metrics(c)
    worst = max(float(np.abs(res.hota[cls][k] - hm[k]).max()) for k in hm)
    worst = max([worst] + [abs(res.clear[cls][k] - cm[k]) for k in cm])
    assert margin >= mc.MARGIN, margin
    assert all(res.clear[cls][k] == cm[k] for k in ('IDSW', 'Frag', 'MT', 'PT', 'ML', 'TP', 'FN', 'FP')) and worst <= TOL
    return res, margin, worst


@pytest.mark.parametrize('assignment', ['greedy', 'optimal'])
def test_a_tracker_scored_end_to_end_equals_the_yardstick(dev, assignment):
    case = tc.case('three_streams_classes')[0]
    scores = [sorted({float(np.float32(o['score'])) for o in objs}) for objs in case['objs']]
    gt, trk, ev = run_tracker(case, dev, assignment, lambda b, f, k, r: scores[b].index(float(r[1])))
    res, margin, worst = score_both_ways(dev, gt, trk, ev)
    assert margin >= mc.MARGIN and res.n_gt['Car'] > 100 and res.clear['Car']['TP'] > 60
    print('three_streams_classes, %s: HOTA %.4f MOTA %.4f IDSW %d, largest disagreement with the yardstick %.3g'
          % (assignment, res.hota_mean['Car']['HOTA'], res.clear['Car']['MOTA'], res.clear['Car']['IDSW'], worst))


def test_chain_dist_optimal_keeps_identities_greedy_switches_them(dev):
    case = ar.fixed('chain_dist')[0]
    idsw = {}
    for assignment in ('optimal', 'greedy'):
        # the object at x = 3 i (frame 0) or 3 i + 1.505 (frame 1) is object i
        gt, trk, ev = run_tracker(case, dev, assignment, lambda b, f, k, r: int(np.floor(float(r[27]) / 3.0 + 1e-3)))
        res, margin, worst = score_both_ways(dev, gt, trk, ev)
        idsw[assignment] = res.clear['Car']['IDSW']
        assert res.clear['Car']['TP'] == 2 * 2 * ar.CHAIN and res.clear['Car']['FN'] == 0
    assert idsw['optimal'] == 0 and idsw['greedy'] > 0
    print('chain_dist: IDSW optimal %d, greedy %d' % (idsw['optimal'], idsw['greedy']))


def test_kitti_preprocessing_on_the_device_equals_the_rule(dev):
    gt0, trk, metric, _ = mc.case('three_seq_bbox')
    gt = mot_eval.Tracks()
    n = 0
    for s, name in enumerate(gt0.names):                      # every 5th ground truth a Van, every 7th occluded, every 11th truncated
        for f, (ids, rows) in enumerate(gt0.frames[s]):
            new = []
            for r in rows:
                n += 1
                r = list(r)
                if n % 5 == 0:
                    r[0] = 'Van'
                if n % 7 == 0:
                    r[2] = 3.0
                if n % 11 == 0:
                    r[1] = 0.2
                new.append(tuple(r))
            tb = trk.frames[s][f][1]
            dc = [('DontCare', -1.0, -1.0, -10.0) + (t[4] - 5.0, t[5] - 5.0, t[6] + 5.0, t[7] + 5.0) + (-1.0, -1.0, -1.0, -1000.0, -1000.0, -1000.0, -10.0, 0.0)
                  for t in tb if t[15] == 0.4][:1]            # a region round the frame's first false positive
            gt.add(name, f, list(ids) + [-1] * len(dc), new + dc)
    p = mot_eval.prepare(gt, trk, 'Car', metric, preprocess=True, device=dev)
    raw = mot_eval.prepare(gt, trk, 'Car', metric, preprocess=False, device=dev)
    f, margin, removed = 0, np.inf, 0
    for s, name in enumerate(gt.names):
        for (gids, grows), (tids, trows) in zip(gt.frames[s], trk.frames[s]):
            g = [(r[0], r[1], r[2], r[4:8]) for r in grows]
            t = [(r[0], r[4:8]) for r in trows]
            rows = [i for i, r in enumerate(g) if r[0] != 'DontCare']
            gl = kitti_eval._frames_to_labels([0], [[grows[i] for i in rows]])
            tl = kitti_eval._frames_to_labels([0], [list(trows)])
            sim = mc.cpu_similarity(gl, tl, metric)[0][:len(rows), :len(trows)]
            keep_g, keep_t, m = ref.preprocess_frame('Car', g, t, sim)
            margin = min(margin, m)
            assert p['ng'][f] == len(keep_g) and p['nt'][f] == len(keep_t), (f, keep_g, keep_t)
            removed += len(trows) - len(keep_t)
            f += 1
    assert margin >= mc.MARGIN and removed > 10 and p['ng'].sum() < raw['ng'].sum() and f == len(p['ng'])
    res = mot_eval.evaluate(gt, trk, classes=('Car', 'Pedestrian'), metric=metric, device=dev)
    assert res.n_gt['Car'] == int(p['ng'].sum()) and res.n_trk['Car'] == int(p['nt'].sum()) and res.n_gt['Pedestrian'] == 0
    assert res.clear['Pedestrian']['TP'] == 0 and res.hota_mean['Car']['HOTA'] > 0.2


def test_command_line_on_files(dev, tmp_path, capsys):
    gt, trk, metric, _ = mc.case('three_seq_bbox')
    for tracks, sub in ((gt, 'gt'), (trk, 'res')):
        (tmp_path / sub).mkdir()
        for name, frames in zip(tracks.names, tracks.frames):
            with open(str(tmp_path / sub / (name + '.txt')), 'w') as fh:
                for f, (ids, rows) in enumerate(frames):
                    for i, r in zip(ids, rows):
                        fh.write('%d %d %s %d %d ' % (f, i, r[0], r[1], r[2]) + ' '.join('%.6f' % v for v in r[3:]) + '\n')
    out = str(tmp_path / 'res.json')
    assert mot_eval.main([str(tmp_path / 'gt'), str(tmp_path / 'res'), '--metric', metric, '--classes', 'Car', '--json', out]) == 0
    printed = capsys.readouterr().out
    want = mot_eval.evaluate(mot_eval.read_tracking_dir(str(tmp_path / 'gt')), mot_eval.read_tracking_dir(str(tmp_path / 'res'), results=True),
                             classes=('Car',), metric=metric, device=dev)
    import json
    with open(out) as fh:
        got = json.load(fh)
    assert got == json.loads(json.dumps(want.to_json())) and printed.strip() == want.table()
    assert got['clear']['Car']['IDSW'] > 0 and got['sequences'] == ['0000', '0001', '0002'] and len(got['hota']['Car']['HOTA']) == 19


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(dev):
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    F, cap = 2, 4
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=dev)        # noqa: E731
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=dev)    # noqa: E731
    n, ids, seq, w = i32(F), i32(F, cap), torch.tensor([0, 2], dtype=torch.int32, device=dev), f64(F, cap, cap)
    match, counts, simsum, per_id, ws = i32(F, cap), i32(1, 4), f64(1), i32(1, 8), torch.zeros(1 << 16, dtype=torch.uint8, device=dev)

    def refused(rc, word):
        msg = lib.rtm3d_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    for bad in (0, 257):
        refused(lib.rtm3d_mot_assign(stream, F, bad, cap, n.data_ptr(), n.data_ptr(), w.data_ptr(), match.data_ptr()), 'cap_g')
        refused(lib.rtm3d_mot_assign(stream, F, cap, bad, n.data_ptr(), n.data_ptr(), w.data_ptr(), match.data_ptr()), 'cap_t')
        assert lib.rtm3d_mot_workspace_bytes(1, F, bad, cap, 8, 8) == 0 and lib.rtm3d_mot_workspace_bytes(1, F, cap, bad, 8, 8) == 0
    refused(lib.rtm3d_mot_assign(stream, F, cap, cap, n.data_ptr(), n.data_ptr(), None, match.data_ptr()), 'null')

    def clear(thr, sim_ptr, cap_g=cap):
        return lib.rtm3d_mot_clear(stream, 1, F, cap_g, cap, 8, 8, seq.data_ptr(), n.data_ptr(), n.data_ptr(), ids.data_ptr(), ids.data_ptr(), sim_ptr,
                                   thr, match.data_ptr(), counts.data_ptr(), simsum.data_ptr(), per_id.data_ptr(), per_id.data_ptr(), per_id.data_ptr(),
                                   ws.data_ptr())
    refused(clear(float('nan'), w.data_ptr()), 'finite')
    refused(clear(float('inf'), w.data_ptr()), 'finite')
    refused(clear(0.5, None), 'null')
    refused(clear(0.5, w.data_ptr(), 257), 'cap_g')
    refused(lib.rtm3d_mot_hota(stream, 1, F, cap, cap, 8, 8, seq.data_ptr(), n.data_ptr(), n.data_ptr(), ids.data_ptr(), ids.data_ptr(), ids.data_ptr(),
                               ids.data_ptr(), w.data_ptr(), w.data_ptr(), per_id.data_ptr(), per_id.data_ptr(), match.data_ptr(), counts.data_ptr(),
                               counts.data_ptr(), counts.data_ptr(), w.data_ptr(), per_id.data_ptr(), None), 'null')
    refused(lib.rtm3d_mot_hota(stream, 0, F, cap, cap, 8, 8, *([None] * 18)), 'S (sequences)')
    torch.cuda.synchronize()
    for t in (match, counts, per_id):
        assert bool((t == 7).all())
    assert bool((simsum == 7.0).all()) and not bool(ws.any())
    with pytest.raises(ValueError, match='holds 256'):
        big = mot_eval.Tracks()
        big.add('s', 0, list(range(257)), [('Car',) + (0.0,) * 15] * 257)
        mot_eval.evaluate(big, mot_eval.Tracks(), classes=('Car',), preprocess=False, device=dev)
