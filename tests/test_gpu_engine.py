"""GPU: engine files loaded by the C loader run the launches of the Python path - logits torch.equal to Model.forward_logits
(graph replay on and off) for the reference-run fixture shapes, detect records equal to the non-pipelined Python step and
matching the reference's detections, the plain C example (a child process without Python) writes the same records, and two
engines of different shapes interleave in one process."""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine          # noqa: E402
from rtm3d_amd import distributed as rdist           # noqa: E402
from rtm3d_amd.model_utils import decode3d_slots     # noqa: E402
from tests.util import load_golden, dets_from_golden  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_RTOL, VERT_TOL_PX = 0.010, 0.25          # the bars of tests/test_gpu_parity.py
HM_RTOL = 0.0055


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def fixture_model(fname, head_precision='fp16'):
    g = load_golden(fname)
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    nconv = int(g['header_num_conv']) if 'header_num_conv' in g else 2
    cfg = rtm3d_amd.kitti_config(bb)
    cfg.MODEL.HEADER_NUM_CONV = nconv
    m = rtm3d_amd.create_model(cfg, head_precision=head_precision).to('cuda:0').eval()
    m.load_state_dict(weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']),
                                               heat_gain=float(g['heat_gain']), header_num_conv=nconv))
    x = weights.synth_images(B, H, W, seed=int(g['img_seed']))
    return g, m, x


def python_step(m, x, K):
    """The non-pipelined Python detect step: forward -> decode2d -> decode3d_slots -> pack_records on one stream."""
    det = m.decode2d(m.forward_logits(x))
    boxes = decode3d_slots(det, K, m.config.DETECTOR.dim_ref, (0.0, -0.5, 20.0))
    return rdist.pack_records(det.n, det.cls, det.score, det.mproj, det.verts, det.bbox, det.topk, boxes)


@pytest.mark.parametrize('fname,prec', [('e2e_dla34_small.npz', 'fp16'), ('e2e_resnet18_small.npz', 'fp16'), ('e2e_resnet34_small.npz', 'fp16'),
                                        ('e2e_dla34_kitti416.npz', 'fp16'), ('e2e_dla34_small_nc1.npz', 'fp16'),
                                        ('e2e_dla34_small_nc3.npz', 'fp16'), ('e2e_dla34_small.npz', 'mxfp8')])
def test_engine_logits_equal_model_logits(dev, tmp_path, fname, prec):
    g, m, x = fixture_model(fname, prec)
    B, _, H, W = x.shape
    path = str(tmp_path / 'e.rtm3d')
    m.save_engine(path, B, H, W)
    x = x.to(dev)
    eng = engine.Engine(path, dev)
    assert eng.info['use_graph'] == 1 and eng.info['head_precision'] == (1 if prec == 'mxfp8' else 0)
    for graph in (True, False):
        m.use_graph = graph
        m._drop_plans()
        eng.set_graph(graph)
        want = m.forward_logits(x)
        for _ in range(2):                         # the second call of graph mode replays the captured graph
            got = eng.forward_logits(x)
            torch.cuda.synchronize()
            for a, b in zip(got, want):
                assert torch.equal(a, b), (fname, prec, graph)
    eng.close()


def test_engine_detect_matches_python_step_and_reference(dev, tmp_path):
    fname = 'e2e_dla34_small.npz'
    g, m, x = fixture_model(fname)
    B, _, H, W = x.shape
    path = str(tmp_path / 'e.rtm3d')
    m.save_engine(path, B, H, W)
    x = x.to(dev)
    K = torch.as_tensor(np.tile(g['K'], (B, 1)), dtype=torch.float64, device=dev)
    eng = engine.Engine(path, dev)
    rec = eng.detect(x, K).clone()
    rec2 = eng.detect(x, K).clone()
    want = python_step(m, x, K)
    torch.cuda.synchronize()
    assert torch.equal(rec, want) and torch.equal(rec2, want)
    rec = rec.cpu().numpy()
    assert (rec[..., 31] >= 1).sum() >= 12 * B                # (random regression weights: the solver keeps few boxes, if any)
    # the reference's detections (bars of test_gpu_parity.py::test_forward_logits_vs_reference_golden)
    tol = HM_RTOL * max(1.0, np.abs(g['logits_main_kf']).max())
    thr_logit = float(np.log(0.4 / 0.6))
    checked, vmax = 0, 0.0
    for b in range(B):
        live = rec[b][rec[b, :, 31] >= 1]
        got = {(int(r[0]), int(r[2] // 4), int(r[3] // 4)): r[4:20].reshape(8, 2) for r in live}
        if g['det_n'][b] == 0:
            continue
        rc, rs, rm, rv, _ = dets_from_golden(g, 'det_', b)
        margin = np.abs(np.log(rs.astype(np.float64) / (1.0 - rs.astype(np.float64))) - thr_logit)
        for c, s, mp, v, ok in zip(rc, rs, rm, rv, margin > tol):
            if not ok:
                continue
            key = (int(c), int(mp[0] // 4), int(mp[1] // 4))
            assert key in got, (key, s)
            vmax = max(vmax, float(np.abs(got[key] - v).max()))
            checked += 1
    assert vmax < VERT_TOL_PX, vmax
    assert checked >= 12 * B, checked
    eng.close()


def test_c_example_writes_the_records_of_the_python_step(dev, tmp_path):
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_detect')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(REPO, 'rtm3d_amd', 'csrc'), 'example'], check=True)
    g, m, x = fixture_model('e2e_dla34_small.npz')
    B, _, H, W = x.shape
    K = np.ascontiguousarray(np.tile(g['K'], (B, 1)), np.float64)
    paths = {k: str(tmp_path / k) for k in ('engine', 'images', 'K', 'records')}
    m.save_engine(paths['engine'], B, H, W)
    x.numpy().astype('<f4').tofile(paths['images'])
    K.astype('<f8').tofile(paths['K'])
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, paths['engine'], paths['images'], paths['K'], paths['records'], '0'],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith('engine_detect: DLA-34 %dx3x%dx%d' % (B, H, W)), r.stdout
    want = python_step(m, x.to(dev), torch.as_tensor(K, device=dev)).cpu().numpy()
    got = open(paths['records'], 'rb').read()
    assert got == want.astype('<f4').tobytes()
    assert (want[..., 31] >= 1).sum() > 0


def test_two_engines_interleave_bit_identically(dev, tmp_path):
    cfg = rtm3d_amd.kitti_config('DLA-34')
    m = rtm3d_amd.create_model(cfg).to('cuda:0').eval()
    m.load_state_dict(weights.synth_state_dict('DLA-34', 5, 'trained'))
    shapes = [(1, 64, 128), (2, 96, 160)]
    engs, xs, wants = [], [], []
    for i, (B, H, W) in enumerate(shapes):
        p = str(tmp_path / ('e%d.rtm3d' % i))
        m.save_engine(p, B, H, W)
        engs.append(engine.Engine(p, dev))
        xs.append(weights.synth_images(B, H, W, seed=20 + i).to(dev))
        wants.append(m.forward_logits(xs[-1]))
    K = [torch.as_tensor(np.tile(weights.synth_intrinsics(), (B, 1)), device=dev) for B, _, _ in shapes]
    recs = [None, None]
    for step in range(3):
        for i in (0, 1) if step % 2 == 0 else (1, 0):
            got = engs[i].forward_logits(xs[i])
            r = engs[i].detect(xs[i], K[i]).clone()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(got, wants[i])), (step, i)
            if recs[i] is None:
                recs[i] = r
            assert torch.equal(r, recs[i]), (step, i)
    for e in engs:
        e.close()
