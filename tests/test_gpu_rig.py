"""GPU: rtm3d_rig_fuse / rtm3d_rig_scatter_ids (csrc/rig.hip) against the numpy yardstick tests/rig_ref.py over the generated
cases of tests/rig_cases.py: the map, the cluster table, the counters, classes, scores, flags and zero fields EQUAL, the fused
boxes within 1e-9 (both sides fp64 without contraction, the device's sin / cos / atan2 against libm's: the bar of
tests/test_gpu_track.py for the same arithmetic), the fp32 boxes of the records the rounding of the device's own fp64 boxes bit
for bit.  Every case's decision margin is asserted first (>= 1e-6, on the yardstick's own numbers).  Then: the records stay
untouched, determinism, R = 2 against two calls of R = 1, the id scatter, and Engine.detect_frames_rig with a tracker next to
the C example.

Measured on an MI355X (the figure each case prints; copied to profiles/rig.txt): between 5.55e-17 and 4.44e-16 in the six cases."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                          # noqa: E402
from rtm3d_amd import _lib, weights, engine, track, rig   # noqa: E402
from tests import rig_ref as ref                          # noqa: E402
from tests import rig_cases as rc                         # noqa: E402
from tests.util import load_golden                        # noqa: E402

CASES = rc.cases()
TOL = 1e-9
BY_NAME = {c['name']: c for c in CASES}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def rig_for(case, dev, rigs=None):
    ext = case['ext'].reshape(case['R'], case['C'], 3, 4)
    if rigs is not None:
        ext = ext[rigs]
    return rig.Rig(ext, R=ext.shape[0], cap=case['cap'], params=rig.RigParams(**case['params']), device=dev)


def run_device(case, dev, rigs=None):
    """The outputs of one call as numpy arrays (dict, the yardstick's names)."""
    C = case['C']
    rec = case['rec'] if rigs is None else np.concatenate([case['rec'][r * C:(r + 1) * C] for r in rigs])
    d_rec = torch.from_numpy(rec).to(dev)
    f = rig_for(case, dev, rigs).fuse(d_rec)
    torch.cuda.synchronize()
    assert d_rec.cpu().numpy().tobytes() == rec.tobytes()                     # the records are read only
    return dict(out=f.records.cpu().numpy(), box=f.box.cpu().numpy(), info=f.info.cpu().numpy(), map=f.map.cpu().numpy(), n=f.n.cpu().numpy())


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ('out', 'box', 'info', 'map', 'n'))


def equals_the_yardstick(case, got, want):
    """The comparison rule of the rig fusion (shared with tests/test_gpu_rig_regimes.py): asserts it, prints and returns the
    largest disagreement of a fused box component."""
    assert want['margin'] >= rc.MARGIN
    assert np.array_equal(got['n'], want['n']), (case['name'], got['n'], want['n'])
    assert np.array_equal(got['map'], want['map']), (case['name'], np.argwhere(got['map'] != want['map'])[:8].tolist())
    assert np.array_equal(got['info'], want['info']), (case['name'], np.argwhere(got['info'] != want['info'])[:8].tolist())
    assert got['out'][..., :24].tobytes() == want['out'][..., :24].tobytes() and np.array_equal(got['out'][..., 31], want['out'][..., 31])
    fin = np.isfinite(want['box'])
    assert np.array_equal(np.isfinite(got['box']), fin) and np.array_equal(got['box'][~fin], want['box'][~fin], equal_nan=True)
    err = float(np.abs(got['box'][fin] - want['box'][fin]).max()) if fin.any() else 0.0
    print('%s: largest disagreement of a fused box component %.3g (bar %g), %d clusters, %d dropped'
          % (case['name'], err, TOL, int(got['n'][:, 0].sum()), int(got['n'][:, 1].sum())))
    assert err <= TOL, (case['name'], err)
    with np.errstate(invalid='ignore', over='ignore'):
        own = got['box'].astype(np.float32)
    assert np.array_equal(got['out'][..., 24:31].view(np.uint32), own.view(np.uint32)), case['name']
    return err


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_cases_equal_the_yardstick(dev, case):
    equals_the_yardstick(case, run_device(case, dev), rc.reference(case))


def test_two_runs_are_bit_identical(dev):
    for name in ('six_cameras_two_rigs', 'sixteen_cameras_overflow'):
        assert same_bytes(run_device(BY_NAME[name], dev), run_device(BY_NAME[name], dev)), name


def test_two_rigs_equal_two_calls_of_one(dev):
    case = BY_NAME['six_cameras_two_rigs']
    both = run_device(case, dev)
    for r in range(2):
        one = run_device(case, dev, [r])
        C = case['C']
        part = dict(out=both['out'][r:r + 1], box=both['box'][r:r + 1], info=both['info'][r:r + 1], map=both['map'][r * C:(r + 1) * C],
                    n=both['n'][r:r + 1])
        assert same_bytes(one, part), r


def test_a_dirty_workspace_and_dirty_outputs_change_nothing(dev):
    """Every output and every word of the workspace that is read is rewritten by the call: a second call of the same Rig (its
    workspace full of the first call's, then of another case's) gives the first call's bytes."""
    case = BY_NAME['three_rigs_own_extrinsics']
    rg = rig_for(case, dev)
    d_rec = torch.from_numpy(case['rec']).to(dev)
    a = rg.fuse(d_rec)
    rg._ws.fill_(0xff)
    b = rg.fuse(d_rec)
    torch.cuda.synchronize()
    for x, y in ((a.records, b.records), (a.box, b.box), (a.info, b.info), (a.map, b.map), (a.n, b.n)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert np.array_equal(b.map.cpu().numpy(), rc.reference(case)['map'])


def test_scatter_ids_against_numpy_indexing(dev):
    case = BY_NAME['sixteen_cameras_overflow']
    rg = rig_for(case, dev)
    f = rg.fuse(torch.from_numpy(case['rec']).to(dev))
    m = f.map.cpu().numpy()
    assert (m == -1).any() and (m == -2).any() and (m >= 0).any()
    rng = np.random.Generator(np.random.PCG64(5))
    ids_rig = rng.integers(-400, 400, (case['R'], case['cap'])).astype(np.int32)          # tentative ids are negative
    assert (ids_rig < 0).any()
    got = rg.camera_ids(torch.from_numpy(ids_rig).to(dev), f).cpu().numpy()
    r_of = np.arange(m.shape[0])[:, None] // case['C']
    want = np.where(m >= 0, ids_rig[r_of, np.clip(m, 0, None)], 0).astype(np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(want, ref.scatter_ids(m, ids_rig, case['R'], case['C']))
    assert (got < 0).any() and (got > 0).any() and not got[m < 0].any()


def test_python_refusals(dev):
    case = BY_NAME['two_cameras_ties_and_flip']
    rg = rig_for(case, dev)
    rec = torch.from_numpy(case['rec']).to(dev)
    with pytest.raises(RuntimeError, match='no CPU path'):
        rg.fuse(rec.cpu())
    with pytest.raises(ValueError, match='rec must be'):
        rg.fuse(rec[:1])
    with pytest.raises(ValueError, match='rec must be'):
        rg.fuse(rec.double())
    with pytest.raises(ValueError, match='topk 257'):
        rg.fuse(torch.zeros(2, 257, 32, device=dev))
    f = rg.fuse(rec)
    with pytest.raises(ValueError, match='ids_rig must be'):
        rg.camera_ids(torch.zeros(1, case['cap'] + 1, dtype=torch.int32, device=dev), f)
    with pytest.raises(RuntimeError, match='no CPU path'):
        rg.camera_ids(torch.zeros(1, case['cap'], dtype=torch.int32), f)
    with pytest.raises(ValueError, match='C \\* topk'):
        rig.Rig(np.stack([rig.mount(0.0)] * 16), device=dev).fuse(torch.zeros(16, 129, 32, device=dev))
    torch.cuda.synchronize()


def test_engine_detect_frames_rig_with_a_tracker_and_the_c_example(dev, tmp_path, monkeypatch):
    """One frame fed as the two cameras of a rig with identical extrinsics, cross_only on, BEV IoU with a bar of 0.9: a valid box
    and its twin in the other camera overlap with IoU 1, nothing else reaches the bar.  Structural invariants that hold exactly
    by the rule, not decision parity on real detections: every cluster of a valid box has the camera mask 0b11, two members and a
    representative from camera 0 (the tie rule); and with a tracker, over three steps, the twins carry one non-zero id.  The
    regression weights of the fixture are random (tests/test_gpu_track.py: FUN_ACCEPT is raised so that its boxes are kept), and
    some kept boxes are not valid ones (a size that is not positive or not finite): by the rule such a box overlaps nothing, its
    own twin included, and is a cluster of one - asserted as such."""
    from rtm3d_amd import model_utils
    monkeypatch.setattr(model_utils, 'FUN_ACCEPT', 1e6)
    monkeypatch.setattr(engine, 'FUN_ACCEPT', 1e6)
    g = load_golden('e2e_dla34_small.npz')
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    assert B == 2
    cfg = rtm3d_amd.kitti_config(bb)
    m = rtm3d_amd.create_model(cfg).to(dev).eval()
    m.load_state_dict(weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']), heat_gain=float(g['heat_gain'])))
    path = str(tmp_path / 'small.rtm3d')
    m.save_engine(path, B, H, W)
    x = weights.synth_images(B, H, W, seed=int(g['img_seed']))
    K = np.tile(g['K'], (B, 1))
    mean, std = cfg.DATASET.MEAN, cfg.DATASET.STD
    v = (x.numpy().astype(np.float64) * np.asarray(std, np.float64).reshape(1, 3, 1, 1) + np.asarray(mean, np.float64).reshape(1, 3, 1, 1)) * 255.0
    full = np.ascontiguousarray(np.clip(np.round(v), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
    frames = [full[0], full[0]]                                   # the same frame from both cameras
    eng = engine.Engine(path, dev)
    eng.set_frame_params(mean, std, None)
    imgs = [torch.from_numpy(f).to(dev) for f in frames]
    topk = eng.info['topk']
    ext = np.stack([rig.mount(0.3, t=(1.0, 0.0, 2.0))] * 2)
    rg = rig.Rig(ext, params=rig.RigParams(metric='bev', thresh=0.9, cross_only=True), device=dev)
    plain = eng.detect_frames(imgs, K).clone()
    rec, fused = eng.detect_frames_rig(imgs, K, rg)
    torch.cuda.synchronize()
    assert torch.equal(rec, plain) and torch.equal(rec[0], rec[1])
    host = rec.cpu().numpy()
    kept = host[..., 31] == 2
    valid = kept & np.isfinite(host[..., 24:31]).all(-1) & (host[..., 24:27] > 0).all(-1)
    n, info, mp = fused.n.cpu().numpy(), fused.info.cpu().numpy()[0], fused.map.cpu().numpy()
    print('detect_frames_rig: %d kept boxes per camera, %d of them valid, %d clusters' % (int(kept[0].sum()), int(valid[0].sum()), int(n[0, 0])))
    assert int(valid[0].sum()) >= 1 and n[0, 1] == 0 and fused.records.shape == (1, min(256, 2 * topk), 32)
    assert n[0, 0] == int(valid[0].sum()) + 2 * int((kept[0] & ~valid[0]).sum())
    for s in range(int(n[0, 0])):
        cam, slot, members, mask = info[s]
        if valid[cam, slot]:
            assert (cam, members, mask) == (0, 2, 0b11) and mp[0, slot] == s and mp[1, slot] == s, (s, info[s])
        else:
            assert members == 1 and mask == 1 << cam and mp[cam, slot] == s, (s, info[s])
    assert ((mp >= 0) == kept).all()

    # with a tracker: three steps, the twins carry one non-zero id; wrong sizes raise before anything runs
    with pytest.raises(ValueError, match='streams'):
        eng.detect_frames_rig(imgs, K, rg, tracker=track.Tracker(2, 8, device=dev))
    with pytest.raises(ValueError, match='cameras'):
        eng.detect_frames_rig(imgs, K, rig.Rig(np.stack([rig.mount(0.0)] * 3), device=dev))
    trk = track.Tracker(1, 256, None, dev)
    for step in range(3):
        rec, rows, fused, ids_rig, ids_cam = eng.detect_frames_rig(imgs, K, rg, kitti=True, tracker=trk)
        torch.cuda.synchronize()
        assert tuple(rows.shape) == (2, topk, 16) and tuple(ids_rig.shape) == (1, fused.records.shape[1]) and tuple(ids_cam.shape) == (2, topk)
        ic = ids_cam.cpu().numpy()
        assert (ic[0][valid[0]] != 0).all() and np.array_equal(ic[0][valid[0]], ic[1][valid[0]]) and not ic[~kept].any() and (ic[kept] != 0).all()
        assert len(set(ic[0][valid[0]].tolist())) == int(valid[0].sum())
    assert (ic[0][valid[0]] > 0).all()                           # matched three times in a row: confirmed

    # the C example on the same three steps, default parameters on both sides
    rg2 = rig.Rig(ext, device=dev)
    trk2 = track.Tracker(1, 128, None, dev)
    want = []
    for step in range(3):
        rec, fused, ids_rig, ids_cam = eng.detect_frames_rig(imgs, K, rg2, tracker=trk2)
        torch.cuda.synchronize()
        want.append((fused.n.cpu().numpy(), fused.box.cpu().numpy(), ids_rig.cpu().numpy(), ids_cam.cpu().numpy()))
    eng.close()
    cap = min(256, 2 * topk)
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_rig_frames')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rtm3d_amd', 'csrc'), 'example'], check=True)
    files = []
    for step in range(3):
        fin = str(tmp_path / ('frames%d.bin' % step))
        with open(fin, 'wb') as f:
            f.write(struct.pack('<i', B))
            for fr in frames:
                f.write(struct.pack('<ii', fr.shape[0], fr.shape[1]))
                f.write(fr.tobytes())
            f.write(K.astype('<f8').tobytes())
            f.write(np.asarray(mean, '<f4').tobytes() + np.asarray(std, '<f4').tobytes())
            f.write(struct.pack('<i', 0))
        files.append(fin)
    f_ext, f_out = str(tmp_path / 'ext.f64'), str(tmp_path / 'out.bin')
    ext.astype('<f8').tofile(f_ext)
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, path, f_ext, f_out] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    raw = open(f_out, 'rb').read()
    per = 8 + cap * 56 + cap * 4 + 2 * topk * 4
    assert len(raw) == 3 * per
    for step in range(3):
        blk = raw[step * per:(step + 1) * per]
        n_c = np.frombuffer(blk[:8], '<i4')
        box_c = np.frombuffer(blk[8:8 + cap * 56], '<f8').reshape(cap, 7)
        rig_c = np.frombuffer(blk[8 + cap * 56:8 + cap * 60], '<i4')
        cam_c = np.frombuffer(blk[8 + cap * 60:], '<i4').reshape(2, topk)
        w_n, w_box, w_rig, w_cam = want[step]
        assert np.array_equal(n_c, w_n[0]) and box_c.tobytes() == w_box[0].tobytes(), (step, r.stdout)
        assert np.array_equal(rig_c, w_rig[0]) and np.array_equal(cam_c, w_cam), (step, r.stdout)
    assert r.stdout.count('  id ') == sum(int(w[0][0, 0]) for w in want) and np.count_nonzero(want[2][3]) >= 2
