"""GPU: rtm3d_tracks_update (csrc/track.hip) against the numpy yardstick tests/track_ref.py over the generated sequences of
tests/track_cases.py, frame by frame: ids, classes, ages, hits, misses, slots and counters EQUAL, filtered states and covariances
within 1e-9 (both sides fp64 without contraction; the bar of tests/test_gpu_box_overlap.py for the same arithmetic).  Every
sequence's decision margin is asserted first (>= 1e-6 in every frame, on the yardstick's own numbers).  Then: reset of one
stream, determinism, the records stay untouched, Engine.detect / detect_frames with a tracker, the C example.

Measured on an MI355X (the figure each case prints; copied to profiles/track.txt): 0 in four sequences, 1.78e-15 in the one with
ego motion."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine, track   # noqa: E402
from tests import track_ref as ref                   # noqa: E402
from tests import track_cases as tc                  # noqa: E402
from tests.util import load_golden                   # noqa: E402

CASES = tc.cases()
TOL = 1e-9
EXACT = [0, 1, 2, 3, 4, 5, 6, 22, 23]                 # id, class, age, hits, misses, score, record slot, the two zero fields
FLOAT = list(range(7, 22))                            # h w l X Y Z ry vx vy vz, Ppp Ppv Pvv, var ry, var dim


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def tracker_for(case, dev):
    B = case['frames'][0].shape[0]
    return track.Tracker(B, case['T'], track.TrackParams(**case['params']), dev)


def run_device(case, dev, frames=None):
    """[(ids, table)] per frame as numpy, and the tracker."""
    trk = tracker_for(case, dev)
    out = []
    for f, rec in enumerate(case['frames'][:frames]):
        d_rec = torch.from_numpy(rec).to(dev)
        ego = None if case['egos'] is None else torch.from_numpy(case['egos'][f]).to(dev)
        ids = trk.update(d_rec, dt=case['dt'], ego=ego)
        torch.cuda.synchronize()
        assert d_rec.cpu().numpy().tobytes() == rec.tobytes()                 # the records are read only
        out.append((ids.cpu().numpy(), trk.state.cpu().numpy().copy()))
    return out, trk


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_sequences_equal_the_yardstick(dev, case):
    want = tc.reference(case)
    assert len(want) == 12 and min(float(w[2].min()) for w in want) >= tc.MARGIN
    got, _ = run_device(case, dev)
    B, T = case['frames'][0].shape[0], case['T']
    worst = 0.0
    for f, ((ids, table), (w_ids, w_table, _)) in enumerate(zip(got, want)):
        assert np.array_equal(ids, w_ids), (case['name'], f, np.argwhere(ids != w_ids)[:8].tolist())
        assert np.array_equal(table[:, :ref.HEADER], w_table[:, :ref.HEADER]), (case['name'], f, table[:, :3], w_table[:, :3])
        g = table[:, ref.HEADER:].reshape(B, T, ref.SLOT)
        w = w_table[:, ref.HEADER:].reshape(B, T, ref.SLOT)
        assert np.array_equal(g[..., EXACT], w[..., EXACT]), (case['name'], f)
        err = float(np.abs(g[..., FLOAT] - w[..., FLOAT]).max())
        worst = max(worst, err)
        assert err <= TOL, (case['name'], f, err)
    print('%s: largest disagreement of a filtered state or covariance over 12 frames %.3g (bar %g)' % (case['name'], worst, TOL))


def test_two_runs_are_bit_identical(dev):
    case = CASES[0]
    a, _ = run_device(case, dev, 6)
    b, _ = run_device(case, dev, 6)
    for (ia, ta), (ib, tb) in zip(a, b):
        assert ia.tobytes() == ib.tobytes() and ta.tobytes() == tb.tobytes()


def test_reset_of_one_stream_leaves_the_others_bit_identical(dev):
    case = [c for c in CASES if c['name'] == 'three_streams_classes'][0]
    out, trk = run_device(case, dev, 5)
    before = trk.state.clone()
    assert bool(trk.tracks()['live'][0].any())
    trk.reset([0])
    torch.cuda.synchronize()
    assert torch.equal(trk.state[1], before[1]) and torch.equal(trk.state[2], before[2]) and not trk.state[0].any()
    t = trk.tracks()
    assert not t['live'][0].any() and t['box'].shape == (3, case['T'], 7) and t['cov'].shape == (3, case['T'], 3)
    # the emptied stream starts again at id 1 (confirmed: its frame counter is 1), the others go on as the yardstick does
    ids = trk.update(torch.from_numpy(case['frames'][5]).to(dev)).cpu().numpy()
    n = len(ref.detections(case['frames'][5][0], case['params']['min_score']))
    assert n > 0 and sorted(ids[0][ids[0] != 0].tolist()) == list(range(1, n + 1))
    want = tc.reference(case)[5][0]
    assert np.array_equal(ids[1], want[1]) and np.array_equal(ids[2], want[2])
    trk.reset()
    torch.cuda.synchronize()
    assert not trk.state.any()


def test_python_refusals(dev):
    trk = track.Tracker(2, 8, device=dev)
    rec = torch.zeros(2, 7, 32, device=dev)
    with pytest.raises(RuntimeError, match='no CPU path'):
        trk.update(rec.cpu())
    with pytest.raises(ValueError, match='rec must be'):
        trk.update(rec[:1])
    with pytest.raises(ValueError, match='rec must be'):
        trk.update(rec.double())
    with pytest.raises(RuntimeError, match='no CPU path'):
        trk.update(rec, ego=torch.zeros(2, 12, dtype=torch.float64))
    with pytest.raises(ValueError, match='ego must be'):
        trk.update(rec, ego=torch.zeros(2, 9, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match='dt'):
        trk.update(rec, dt=0.0)
    with pytest.raises(RuntimeError, match='topk 257'):
        trk.update(torch.zeros(2, 257, 32, device=dev))
    with pytest.raises(ValueError, match='capacity'):
        track.Tracker(1, 257, device=dev)
    torch.cuda.synchronize()
    assert not trk.state.any()


def test_engine_detect_with_a_tracker_and_the_c_example(dev, tmp_path, monkeypatch):
    """The regression weights of the fixture are random, so the solver's residual keeps none of its boxes at the product's bar; as
    in tests/test_gpu_box_overlap.py the bar is raised for this model (pack_records reads model_utils.FUN_ACCEPT, save_engine writes
    engine.FUN_ACCEPT into the file, so the C example sees it too), which turns every solved slot into a kept one.  Not every such
    box is a valid one (positive finite sizes): the detect part matches on centre distance, which any finite box supports, and the
    ids are asserted to be non-zero, persistent and confirmed on a non-empty set; the detect_frames part runs the default 3D IoU
    the C example runs, where the valid boxes persist and the others are born again every frame - in both programs alike."""
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
    assert isinstance(plain, torch.Tensor)
    trk = track.Tracker(B, 128, track.TrackParams(metric='dist', thresh=-0.5, min_hits=3), dev)
    host = plain.cpu().numpy()
    kept = host[..., 31] == 2
    finite = kept & np.isfinite(host[..., 24:31]).all(-1)
    print('Engine.detect with a tracker: %d kept boxes in %d images, %d of them finite' % (int(kept.sum()), B, int(finite.sum())))
    assert int(finite.sum()) >= 4 and all(int(finite[b].sum()) >= 1 for b in range(B)), (kept.sum(), finite.sum())
    seen = []
    for n in range(3):
        rec, ids = eng.detect(x.to(dev), K, tracker=trk)
        torch.cuda.synchronize()
        assert torch.equal(rec, plain) and ids.dtype == torch.int32 and tuple(ids.shape) == tuple(plain.shape[:2])
        seen.append(ids.cpu().numpy())
    assert not any(s[~kept].any() for s in seen) and all((s[kept] != 0).all() for s in seen)
    # the same finite boxes keep their ids over the three calls, one id each, and are confirmed on the third
    assert (seen[0][finite] > 0).all() and np.array_equal(seen[1][finite], seen[0][finite]) and np.array_equal(seen[2][finite], seen[0][finite])
    for b in range(B):
        first = seen[0][b][kept[b]]
        assert sorted(first.tolist()) == list(range(1, int(kept[b].sum()) + 1))           # frame 1: births in slot order
        assert len(set(seen[2][b][finite[b]].tolist())) == int(finite[b].sum())
    t = trk.tracks()
    tid, hits, slot = t['id'].cpu().numpy(), t['hits'].cpu().numpy(), t['slot'].cpu().numpy()
    for b in range(B):
        for k in np.flatnonzero(finite[b]):
            row = np.flatnonzero(tid[b] == seen[2][b][k])
            assert len(row) == 1 and hits[b, row[0]] == 3 and slot[b, row[0]] == k, (b, k)

    # camera frames: detect_frames with a tracker, and the C example on the same three frame files
    mean, std = cfg.DATASET.MEAN, cfg.DATASET.STD
    v = (x.numpy().astype(np.float64) * np.asarray(std, np.float64).reshape(1, 3, 1, 1) + np.asarray(mean, np.float64).reshape(1, 3, 1, 1)) * 255.0
    full = np.ascontiguousarray(np.clip(np.round(v), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
    frames = [full[0], np.ascontiguousarray(full[1][9:110, 20:243])]
    eng.set_frame_params(mean, std, None)
    imgs = [torch.from_numpy(f).to(dev) for f in frames]
    plain_f = eng.detect_frames(imgs, K).clone()
    host_f = plain_f.cpu().numpy()
    kept_f = host_f[..., 31] == 2
    valid_f = kept_f & np.isfinite(host_f[..., 24:31]).all(-1) & (host_f[..., 24:27] > 0).all(-1)
    print('Engine.detect_frames with a tracker: %d kept boxes, %d of them valid' % (int(kept_f.sum()), int(valid_f.sum())))
    assert int(kept_f.sum()) >= 4 and int(valid_f.sum()) >= 1, (kept_f.sum(), valid_f.sum())
    trk2 = track.Tracker(B, 128, None, dev)
    want = []
    for n in range(3):
        rec, rows, ids = eng.detect_frames(imgs, K, kitti=True, tracker=trk2)
        torch.cuda.synchronize()
        assert torch.equal(rec, plain_f) and tuple(rows.shape) == (B, plain_f.shape[1], 16)
        want.append(ids.cpu().numpy())
    assert all((w[kept_f] != 0).all() and not w[~kept_f].any() for w in want)
    # a valid box overlaps itself with 3D IoU 1: unless another valid box competes for it, it keeps its id
    stay = valid_f & (want[1] == want[0]) & (want[2] == want[0])
    print('Engine.detect_frames with a tracker: %d valid boxes keep their id over three frames' % int(stay.sum()))
    assert int(stay.sum()) >= 1 and (want[2][stay] > 0).all()
    eng.close()
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_track_frames')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rtm3d_amd', 'csrc'), 'example'], check=True)
    files = []
    for n in range(3):
        fin = str(tmp_path / ('frames%d.bin' % n))
        with open(fin, 'wb') as f:
            f.write(struct.pack('<i', B))
            for fr in frames:
                f.write(struct.pack('<ii', fr.shape[0], fr.shape[1]))
                f.write(fr.tobytes())
            f.write(K.astype('<f8').tobytes())
            f.write(np.asarray(mean, '<f4').tobytes() + np.asarray(std, '<f4').tobytes())
            f.write(struct.pack('<i', 0))
        files.append(fin)
    f_ids = str(tmp_path / 'ids.i32')
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, path, f_ids] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(f_ids, '<i4').reshape(3, B, -1)
    assert np.count_nonzero(got) >= 3 * 4 and np.array_equal(got, np.stack(want)), r.stdout
