"""GPU: the optimal association of the tracker (rtm3d_tracks_update_assign, csrc/track.hip, step 3b of the rule) against the numpy
yardstick tests/track_assign_ref.py, frame by frame, by the comparison rule of tests/test_gpu_track.py: ids, classes, ages, hits,
misses, scores, record slots and the three counters EQUAL, filtered states and covariances within 1e-9.  Every sequence's margin
(threshold, heading and uniqueness of the optimum) is asserted first: >= 1e-6 in every frame, on the yardstick's own numbers.
Then the chain the greedy rule gets wrong, exact ties, a frame without candidates, assign = 0 through the new entry point, the
evaluator's entry point on the tracker's own gains, and Engine.detect with an optimal tracker.

Measured on an MI355X (the figure each case prints; copied to profiles/track.txt): 0 in dense_3d, overflow_bev,
three_streams_classes and chain_dist, 1.78e-15 in crossing_dist_ego."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine, track, mot_eval   # noqa: E402
from tests import track_ref as ref                   # noqa: E402
from tests import track_cases as tc                  # noqa: E402
from tests import track_assign_ref as ar             # noqa: E402
from tests.util import load_golden                   # noqa: E402

TOL = 1e-9
EXACT = [0, 1, 2, 3, 4, 5, 6, 22, 23]                 # id, class, age, hits, misses, score, record slot, the two zero fields
FLOAT = list(range(7, 22))                            # h w l X Y Z ry vx vy vz, Ppp Ppv Pvv, var ry, var dim


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def run_device(case, dev, assignment):
    """[(ids, table)] per frame as numpy."""
    B = case['frames'][0].shape[0]
    trk = track.Tracker(B, case['T'], track.TrackParams(**case['params']), dev, assignment=assignment)
    assert trk.assignment == assignment
    out = []
    for f, rec in enumerate(case['frames']):
        d_rec = torch.from_numpy(rec).to(dev)
        ego = None if case['egos'] is None else torch.from_numpy(case['egos'][f]).to(dev)
        ids = trk.update(d_rec, dt=case['dt'], ego=ego)
        torch.cuda.synchronize()
        assert d_rec.cpu().numpy().tobytes() == rec.tobytes()                 # the records are read only
        out.append((ids.cpu().numpy(), trk.state.cpu().numpy().copy()))
    return out


def compare(case, got, want):
    B, T = case['frames'][0].shape[0], case['T']
    assert len(got) == len(want) and min(float(w[2].min()) for w in want) >= tc.MARGIN
    worst = 0.0
    for f, ((ids, table), w_res) in enumerate(zip(got, want)):
        w_ids, w_table = w_res[0], w_res[1]
        assert np.array_equal(ids, w_ids), (case['name'], f, np.argwhere(ids != w_ids)[:8].tolist())
        assert np.array_equal(table[:, :ref.HEADER], w_table[:, :ref.HEADER]), (case['name'], f, table[:, :3], w_table[:, :3])
        g = table[:, ref.HEADER:].reshape(B, T, ref.SLOT)
        w = w_table[:, ref.HEADER:].reshape(B, T, ref.SLOT)
        assert np.array_equal(g[..., EXACT], w[..., EXACT]), (case['name'], f)
        err = float(np.abs(g[..., FLOAT] - w[..., FLOAT]).max())
        worst = max(worst, err)
        assert err <= TOL, (case['name'], f, err)
    print('%s, optimal: largest disagreement of a filtered state or covariance over %d frames %.3g (bar %g)'
          % (case['name'], len(got), worst, TOL))


@pytest.mark.parametrize('name', ['dense_3d', 'overflow_bev', 'three_streams_classes', 'crossing_dist_ego'])
def test_sequences_equal_the_yardstick_under_the_optimal_rule(dev, name):
    case, want = ar.case(name)
    assert len(want) == 12
    compare(case, run_device(case, dev, 'optimal'), want)


def test_chain_dist_keeps_every_identity_where_greedy_breaks_them(dev):
    case, want = ar.fixed('chain_dist')
    got = run_device(case, dev, 'optimal')
    compare(case, got, want)
    n = ar.CHAIN
    for b in range(2):
        born, now = got[0][0][b], got[1][0][b]
        assert sorted(born[:n].tolist()) == list(range(1, n + 1)) and not born[n:].any()
        assert np.array_equal(now, born)                                      # every detection carries the id it was born with
        assert got[1][1][b, 0] == n                                           # issued: no id was given out in frame 1
    greedy = run_device(case, dev, 'greedy')
    for b in range(2):
        assert np.array_equal(greedy[0][0][b], got[0][0][b])
        assert (greedy[1][0][b] != greedy[0][0][b]).any() and greedy[1][1][b, 0] == n + 1


def test_exact_ties_are_matched_and_deterministic(dev):
    case, want = ar.fixed('exact_ties')
    assert want[1][2][0] == 0.0 and want[1][3][0] == 3.0                      # a tie on the yardstick's side too: optimum 3.0
    a = run_device(case, dev, 'optimal')
    ids0, ids1 = a[0][0][0], a[1][0][0]
    assert ids0[:2].tolist() == [1, 2] and sorted(ids1[:2].tolist()) == [1, 2] and not ids1[2:].any() and a[1][1][0, 0] == 2
    slots = a[1][1][0, ref.HEADER:].reshape(case['T'], ref.SLOT)
    f0, f1 = case['frames'][0][0].astype(np.float64), case['frames'][1][0].astype(np.float64)
    gain = 0.0
    for t in (0, 1):
        k = int(slots[t, 6])
        assert k in (0, 1) and slots[t, 0] == t + 1 and ids1[k] == t + 1
        aff = -np.sqrt(((f0[t, 27:30] - f1[k, 27:30]) ** 2).sum())
        assert aff > case['params']['thresh']                                 # every matched pair is a candidate
        gain += aff - case['params']['thresh']
    assert abs(gain - want[1][3][0]) <= 1e-9
    b = run_device(case, dev, 'optimal')
    for (ia, ta), (ib, tb) in zip(a, b):
        assert ia.tobytes() == ib.tobytes() and ta.tobytes() == tb.tobytes()


def test_frame_without_candidates_equals_greedy_bit_for_bit(dev):
    case, want = ar.fixed('no_candidates')
    a, g = run_device(case, dev, 'optimal'), run_device(case, dev, 'greedy')
    for (ia, ta), (ig, tg) in zip(a, g):
        assert ia.tobytes() == ig.tobytes() and ta.tobytes() == tg.tobytes()
    assert a[1][0][0][:5].tolist() == [6, 7, 8, 0, 0] and tuple(a[1][1][0, :3]) == (8.0, 2.0, 2.0)
    slots = a[1][1][0, ref.HEADER:].reshape(case['T'], ref.SLOT)
    assert (slots[:5, 4] == 1).all() and (slots[:5, 6] == -1).all() and np.array_equal(a[1][0], want[1][0])


def test_assign_0_through_the_new_entry_is_tracks_update(dev):
    case = tc.case('twins_class_blind')[0]
    lib = _lib.load()
    B, topk, T = case['frames'][0].shape[0], case['topk'], case['T']
    p = track.TrackParams(**case['params']).to_c()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    states = [torch.zeros(B, ref.HEADER + ref.SLOT * T, dtype=torch.float64, device=dev) for _ in range(2)]
    ids = [torch.zeros(B, topk, dtype=torch.int32, device=dev) for _ in range(2)]
    ws = torch.empty(int(lib.rtm3d_tracks_workspace_bytes(B, topk, T)), dtype=torch.uint8, device=dev)
    for rec in case['frames']:
        d_rec = torch.from_numpy(rec).to(dev)
        _lib.check(lib.rtm3d_tracks_update(stream, B, topk, T, d_rec.data_ptr(), 1.0, None, ctypes.byref(p), states[0].data_ptr(),
                                           ids[0].data_ptr(), ws.data_ptr()), 'tracks_update')
        _lib.check(lib.rtm3d_tracks_update_assign(stream, B, topk, T, d_rec.data_ptr(), 1.0, None, ctypes.byref(p), 0, states[1].data_ptr(),
                                                  ids[1].data_ptr(), ws.data_ptr()), 'tracks_update')
        torch.cuda.synchronize()
        assert ids[0].cpu().numpy().tobytes() == ids[1].cpu().numpy().tobytes()
        assert states[0].cpu().numpy().tobytes() == states[1].cpu().numpy().tobytes()
    assert int(states[0][0, 0].item()) >= 4 and bool((ids[0] != 0).any())


def test_the_evaluator_entry_gives_the_tracker_match_on_the_same_gains(dev):
    """One solver text (csrc/assign_wave.h) behind both entry points: the match rtm3d_tracks_update_assign(assign = 1) stores equals
    rtm3d_mot_assign on w = affinity - thresh read back from the tracker's own workspace, exact ties included; integers, exactly.
    Both cases have T, topk <= 64, so the evaluator runs its one-column-per-lane form against the tracker's four-column one; the
    evaluator's own four-column form is compared with scipy in tests/test_gpu_mot_eval.py, not with the tracker here."""
    lib = _lib.load()
    for name in ('exact_ties', 'chain_dist'):
        case = ar.fixed(name)[0]
        B, topk, T = case['frames'][0].shape[0], case['topk'], case['T']
        p = track.TrackParams(**case['params']).to_c()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        state = torch.zeros(B, ref.HEADER + ref.SLOT * T, dtype=torch.float64, device=dev)
        ids = torch.zeros(B, topk, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.rtm3d_tracks_workspace_bytes(B, topk, T)), dtype=torch.uint8, device=dev)
        assert len(case['frames']) == 2                                       # the births, then the frame that is matched
        for rec in case['frames']:
            before = state.cpu().numpy()[:, ref.HEADER:].reshape(B, T, ref.SLOT).copy()
            d_rec = torch.from_numpy(rec).to(dev)
            _lib.check(lib.rtm3d_tracks_update_assign(stream, B, topk, T, d_rec.data_ptr(), case['dt'], None, ctypes.byref(p), 1,
                                                      state.data_ptr(), ids.data_ptr(), ws.data_ptr()), 'tracks_update_assign')
            torch.cuda.synchronize()
        aff = ws.view(torch.float64).reshape(B, T, topk)
        w = torch.where(aff > -np.inf, aff - case['params']['thresh'], torch.zeros_like(aff))
        match = mot_eval.assign(w, np.full(B, T), np.full(B, topk)).cpu().numpy()
        after = state.cpu().numpy()[:, ref.HEADER:].reshape(B, T, ref.SLOT)
        live = before[..., 0] != 0
        assert live.sum() == {'exact_ties': 2, 'chain_dist': 2 * ar.CHAIN}[name] and int((w > 0).sum()) > live.sum()
        assert np.array_equal(after[..., 0][live], before[..., 0][live])      # still the same tracks: field 6 is this frame's match
        assert np.array_equal(match[live], after[..., 6][live].astype(np.int64)), name
        assert (match[live] >= 0).all() and (match[~live] == -1).all()


def test_engine_detect_with_an_optimal_tracker(dev, tmp_path, monkeypatch):
    """The fixture and the raised acceptance bar of tests/test_gpu_track.py's engine test (random regression weights keep no box
    at the product's bar); centre distance, which any finite box supports."""
    from rtm3d_amd import model_utils
    monkeypatch.setattr(model_utils, 'FUN_ACCEPT', 1e6)
    monkeypatch.setattr(engine, 'FUN_ACCEPT', 1e6)
    g = load_golden('e2e_dla34_small.npz')
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    cfg = rtm3d_amd.kitti_config(bb)
    m = rtm3d_amd.create_model(cfg).to(dev).eval()
    m.load_state_dict(weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']), heat_gain=float(g['heat_gain'])))
    path = str(tmp_path / 'small.rtm3d')
    m.save_engine(path, B, H, W)
    x = weights.synth_images(B, H, W, seed=int(g['img_seed']))
    K = np.tile(g['K'], (B, 1))
    eng = engine.Engine(path, dev)
    plain = eng.detect(x.to(dev), K).clone()
    host = plain.cpu().numpy()
    kept = host[..., 31] == 2
    finite = kept & np.isfinite(host[..., 24:31]).all(-1)
    assert int(kept.sum()) > 0 and int(finite.sum()) >= 4, (kept.sum(), finite.sum())
    trk = track.Tracker(B, 128, track.TrackParams(metric='dist', thresh=-0.5, min_hits=3), dev, assignment='optimal')
    seen = []
    for n in range(2):
        rec, ids = eng.detect(x.to(dev), K, tracker=trk)
        torch.cuda.synchronize()
        assert torch.equal(rec, plain) and ids.dtype == torch.int32 and tuple(ids.shape) == tuple(plain.shape[:2])
        seen.append(ids.cpu().numpy())
    assert not any(s[~kept].any() for s in seen) and all((s[kept] != 0).all() for s in seen)
    assert (seen[0][finite] > 0).all() and np.array_equal(seen[1][finite], seen[0][finite])      # the ids persist
    hits = trk.tracks()['hits'].cpu().numpy()
    tid = trk.tracks()['id'].cpu().numpy()
    for b in range(B):
        for k in np.flatnonzero(finite[b]):
            row = np.flatnonzero(tid[b] == seen[1][b][k])
            assert len(row) == 1 and hits[b, row[0]] == 2, (b, k)
    eng.close()
