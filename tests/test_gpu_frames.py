"""GPU: the camera-frame path - rtm3d_frames_adjust_k and rtm3d_records_to_camera against the numpy statements of the same
bookkeeping (bit for bit; the KITTI rows at the bar of test_project_boxes_device_vs_reference_vectors), and
Engine.detect_frames, the plain C example and Detect3DPipeline.submit_uint8(camera_K=True) against the Python path that
already exists (preprocess_batch -> forward_logits(preloaded) -> decode2d -> decode3d_slots -> pack_records -> numpy)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine, preprocess  # noqa: E402
from rtm3d_amd import distributed as rdist           # noqa: E402
from rtm3d_amd import kitti_results as kr            # noqa: E402
from rtm3d_amd.model import Detections               # noqa: E402
from rtm3d_amd.model_utils import Boxes3D, decode3d_slots, FUN_ACCEPT  # noqa: E402
from rtm3d_amd.pipeline import Detect3DPipeline      # noqa: E402
from tests.util import load_golden                   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LOC = (0.0, -0.5, 20.0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------------------------------- numpy references
def geoms(specs, size):
    """[(h, w, resize_to or None)] -> one ctypes array of FrameGeom on the (H, W) canvas (each through rtm3d_frame_geometry,
    itself pinned by tests/test_frames_cpu.py)."""
    out = (_lib.FrameGeom * len(specs))()
    for i, (h, w, r) in enumerate(specs):
        g = preprocess.frame_geometry([(h, w)], size, r)[0]
        out[i] = _lib.FrameGeom(g.h, g.w, g.rh, g.rw, g.pad_w, g.pad_h)
    return out


def K_net_numpy(K_cam, geom):
    return np.concatenate([preprocess.adjust_K(preprocess.resize_K(K_cam[b], (g.h, g.w), (g.rh, g.rw)), g.pad_w, g.pad_h)
                           for b, g in enumerate(geom)])


def to_camera_numpy(rec, geom):
    """The issue's formula on (B, topk, 32) canvas records: float64, one rounding to float32."""
    out = rec.copy()
    for b, g in enumerate(geom):
        live = rec[b, :, 31] >= 1
        v = rec[b][:, 2:24].astype(np.float64)
        v[:, 0::2] = (v[:, 0::2] - g.pad_w) * (np.float64(g.w) / np.float64(g.rw))
        v[:, 1::2] = (v[:, 1::2] - g.pad_h) * (np.float64(g.h) / np.float64(g.rh))
        out[b][live, 2:24] = v.astype(np.float32)[live]
    return out


def kitti_rows_numpy(rec, x, fun, status, K_cam, geom):
    """(B, topk, 16) rows from kitti_results.kitti_label_values on the fp64 solver outputs, and the same without clipping."""
    B, topk = rec.shape[:2]
    rows, unclipped = np.zeros((B, topk, 16)), np.zeros((B, topk, 16))
    x, fun, status = x.reshape(B, topk, 8), fun.reshape(B, topk), status.reshape(B, topk)
    for b, g in enumerate(geom):
        kept = (rec[b, :, 31] >= 1) & (status[b] >= 0) & (fun[b] < FUN_ACCEPT)
        xs = x[b][kept]
        params = {'class': rec[b][kept, 0].astype(np.int64), 'Ry': np.arctan2(xs[:, 0], xs[:, 1]), 'dimension': xs[:, [3, 4, 2]],
                  'location': xs[:, 5:8], 'K': np.tile(K_cam[b], (kept.sum(), 1)), 'score': rec[b][kept, 1].astype(np.float64)}
        for dst, size in ((rows, (g.w, g.h)), (unclipped, None)):
            dst[b][kept, :14] = kr.kitti_label_values(params, image_size=size)
            dst[b][kept, 14] = 2.0
    return rows, unclipped


# ------------------------------------------------------------------------------------------------ 1. adjust_K
RAGGED = [(128, 256, None),      # identity: the divide / multiply pair still runs
          (300, 1000, 256),      # width-limited Resize
          (100, 201, None),      # no Resize, padding on both axes
          (101, 223, None),      # odd differences: both pads truncate
          (500, 300, 128)]       # height-limited Resize


def test_frames_adjust_K_equals_numpy(dev):
    rng = np.random.Generator(np.random.PCG64(11))
    for specs in (RAGGED, [RAGGED[i % 5] for i in range(70)]):          # 70 images: two by-value chunks (64 + 6)
        geom = geoms(specs, (128, 256))
        B = len(specs)
        K = np.tile(weights.synth_intrinsics(), (B, 1)) * rng.uniform(0.5, 1.5, (B, 9))
        K[:, 6:] = rng.uniform(-1, 1, (B, 3))                          # row 2 is copied whatever it holds
        got = preprocess.adjust_K_device(torch.as_tensor(K, device=dev), geom)
        np.testing.assert_array_equal(got.cpu().numpy(), K_net_numpy(K, geom))
    with pytest.raises(ValueError):
        preprocess.adjust_K_device(torch.as_tensor(K[:3], device=dev), geom)


# ------------------------------------------------------------------------------------------------ 2. records_to_camera
@pytest.fixture(scope='module')
def solved(dev):
    """The objects of decode3d_cases.npz as the slots of two images with different geometries, solved and packed once."""
    g = load_golden('decode3d_cases.npz')
    topk, B, size = len(g['clses']), 2, (384, 1280)
    # image 0: a 300 x 1000 frame fed as it is (the projected rectangles of the fixture reach beyond it: clipping is active);
    # image 1: a 200 x 640 frame resized to 375 x 1200 (scale 1.875, pads 40 and 4)
    geom = geoms([(300, 1000, None), (200, 640, 1200)], size)
    # cameras whose canvas intrinsics are (up to rounding) the fixture's K
    K_cam = np.zeros((B, 9))
    for b, q in enumerate(geom):
        k = g['K'].copy()
        k[2] -= q.pad_w; k[5] -= q.pad_h
        k[:3] *= q.w / q.rw; k[3:6] *= q.h / q.rh
        K_cam[b] = k
    K_cam_d = torch.as_tensor(K_cam, device=dev)
    K_net = preprocess.adjust_K_device(K_cam_d, geom)
    det = Detections(B, topk, dev)
    n = [topk, topk - 14]                                               # the last 14 slots of image 1 are empty
    det.n.copy_(torch.tensor(n, dtype=torch.int32))
    rng = np.random.Generator(np.random.PCG64(3))
    uv = np.tile(g['uv'].astype(np.float32), (B, 1, 1))
    det.cls.copy_(torch.from_numpy(np.tile(g['clses'], B)))
    det.score.copy_(torch.from_numpy(rng.uniform(0.4, 1.0, B * topk).astype(np.float32)))
    det.verts.copy_(torch.from_numpy(uv))
    det.mproj.copy_(torch.from_numpy(uv.mean(1)))
    det.bbox.copy_(torch.from_numpy(np.concatenate([uv.min(1), uv.max(1)], 1)))
    boxes = decode3d_slots(det, K_net, g['dim_ref'], g['ref_loc'])
    rec = rdist.pack_records(det.n, det.cls, det.score, det.mproj, det.verts, det.bbox, topk, boxes)
    torch.cuda.synchronize()
    return {'geom': geom, 'K_cam': K_cam, 'K_cam_d': K_cam_d, 'boxes': boxes, 'rec': rec, 'n': n, 'topk': topk, 'B': B}


def test_records_to_camera_on_solver_fixtures(dev, solved):
    s = solved
    geom, B, topk = s['geom'], s['B'], s['topk']
    canvas = s['rec'].cpu().numpy()
    x, fun, status = (t.cpu().numpy() for t in (s['boxes'].x, s['boxes'].fun, s['boxes'].status))
    got, rows = preprocess.records_to_camera(s['rec'].clone(), geom, K_camera=s['K_cam_d'], boxes=s['boxes'], kitti=True)
    plain = preprocess.records_to_camera(s['rec'].clone(), geom)                       # without the KITTI rows
    torch.cuda.synchronize()
    assert torch.equal(got, plain)
    got, rows = got.cpu().numpy(), rows.cpu().numpy()
    flag = canvas[..., 31]
    assert (flag == 2).sum() >= 8, (flag == 2).sum()
    assert (flag[1, s['n'][1]:] == 0).all() and (flag[1, :s['n'][1]] >= 1).all() and (flag[0] >= 1).all()
    # 2D fields: the formula in float64, one rounding; everything else untouched; empty slots all zero
    np.testing.assert_array_equal(got[..., 2:24], to_camera_numpy(canvas, geom)[..., 2:24])
    np.testing.assert_array_equal(got[..., :2], canvas[..., :2])
    np.testing.assert_array_equal(got[..., 24:], canvas[..., 24:])
    assert not got[flag == 0].any()
    assert (got[..., 2:24] != canvas[..., 2:24])[flag >= 1].any(axis=-1).all()          # every live slot did move
    # KITTI rows: kitti_label_values on the same fp64 solver outputs, the bar of the device's projection test
    want, unclipped = kitti_rows_numpy(canvas, x, fun, status, s['K_cam'], geom)
    kept = flag == 2
    np.testing.assert_array_equal(kept, want[..., 14] == 2)
    np.testing.assert_allclose(rows[kept], want[kept], rtol=1e-9, atol=1e-7)
    assert not rows[~kept].any()
    assert (rows[kept][:, 15] == 0).all() and (rows[kept][:, 14] == 2).all()
    assert (want[0][kept[0], 2:6] != unclipped[0][kept[0], 2:6]).any(), 'the clipping of image 0 was meant to be active'
    g0, g1 = geom[0], geom[1]
    for b, q in ((0, g0), (1, g1)):
        r = rows[b][kept[b]]
        assert (r[:, [2, 4]] >= 0).all() and (r[:, [2, 4]] <= q.w - 1).all() and (r[:, [3, 5]] >= 0).all() and (r[:, [3, 5]] <= q.h - 1).all()


def test_records_to_camera_over_two_chunks(dev):
    """66 images (64 + 2 by-value chunks) of 4 slots with made-up records and solver outputs: every chunk offset is right."""
    rng = np.random.Generator(np.random.PCG64(17))
    B, topk = 66, 4
    geom = geoms([RAGGED[i % 5] for i in range(B)], (128, 256))
    rec = rng.uniform(0, 256, (B, topk, 32)).astype(np.float32)
    rec[..., 0] = rng.integers(0, 3, (B, topk))
    rec[..., 31] = rng.integers(0, 3, (B, topk))
    rec[rec[..., 31] == 0] = 0
    bx = Boxes3D(B * topk, dev)
    x = np.concatenate([rng.uniform(-1, 1, (B * topk, 2)), rng.uniform(1, 4, (B * topk, 3)), rng.uniform(-8, 8, (B * topk, 1)),
                        rng.uniform(0.5, 2, (B * topk, 1)), rng.uniform(8, 60, (B * topk, 1))], 1)
    flag = rec[..., 31].reshape(-1)
    fun = np.where(flag == 2, 0.01, 5.0)
    status = np.where(flag >= 1, 0, -1).astype(np.int32)
    bx.x.copy_(torch.from_numpy(x)); bx.fun.copy_(torch.from_numpy(fun)); bx.status.copy_(torch.from_numpy(status))
    K_cam = np.tile(weights.synth_intrinsics(), (B, 1)) * rng.uniform(0.9, 1.1, (B, 1))
    K_cam[:, 6:] = (0, 0, 1)
    got, rows = preprocess.records_to_camera(torch.from_numpy(rec).to(dev), geom, K_camera=torch.as_tensor(K_cam, device=dev), boxes=bx,
                                             kitti=True)
    np.testing.assert_array_equal(got.cpu().numpy(), to_camera_numpy(rec, geom))
    want, _ = kitti_rows_numpy(rec, x, fun, status, K_cam, geom)
    assert (want[..., 14] == 2).sum() >= B
    np.testing.assert_allclose(rows.cpu().numpy(), want, rtol=1e-9, atol=1e-7)
    assert not rows.cpu().numpy()[rec[..., 31] != 2].any()


# ------------------------------------------------------------------------------------------------ 3. Engine.detect_frames
def uint8_frames(x, mean, std):
    """Invert the normalisation of synth_images: (B, 3, H, W) fp32 -> (B, H, W, 3) uint8."""
    m, s = np.asarray(mean, np.float64).reshape(1, 3, 1, 1), np.asarray(std, np.float64).reshape(1, 3, 1, 1)
    v = np.clip(np.round((x.numpy().astype(np.float64) * s + m) * 255.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(v.transpose(0, 2, 3, 1))


@pytest.fixture(scope='module')
def small(dev, tmp_path_factory):
    """The model of e2e_dla34_small.npz, its engine file, two sets of ragged frames and - per set - what the Python path
    that exists today makes of them (computed once, shared by the engine, C example and pipeline tests)."""
    g = load_golden('e2e_dla34_small.npz')
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    cfg = rtm3d_amd.kitti_config(bb)
    m = rtm3d_amd.create_model(cfg).to('cuda:0').eval()
    m.load_state_dict(weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']),
                                               heat_gain=float(g['heat_gain'])))
    path = str(tmp_path_factory.mktemp('frames') / 'small.rtm3d')
    m.save_engine(path, B, H, W)
    mean, std = cfg.DATASET.MEAN, cfg.DATASET.STD
    full = uint8_frames(weights.synth_images(B, H, W, seed=int(g['img_seed'])), mean, std)
    assert B == 2
    sets = {
        # one frame equal to the canvas, one narrower and shorter (odd pads), fed at their own size
        'pad': (None, [full[0], np.ascontiguousarray(full[1][9:110, 20:243])]),
        # Resize to W: frames 2x and 3x the size of what the network is to see, every pixel repeated (bilinear resampling of
        # white noise itself would smooth the heat map empty; of repeated pixels it gives the pixels back): 256 x 512 ->
        # 128 x 256 and 354 x 768 -> 118 x 256 (pad_h 5)
        'resize': (W, [np.ascontiguousarray(full[0].repeat(2, 0).repeat(2, 1)),
                       np.ascontiguousarray(full[1][5:123].repeat(3, 0).repeat(3, 1))]),
    }
    K_cam = np.tile(g['K'], (B, 1)) * np.array([[1.0], [1.03]])
    K_cam[:, 6:] = (0, 0, 1)
    out = {'model': m, 'engine': path, 'mean': mean, 'std': std, 'B': B, 'H': H, 'W': W, 'K_cam': K_cam, 'sets': {}}
    for name, (resize_to, frames) in sets.items():
        imgs = [torch.from_numpy(f).to(dev) for f in frames]
        _, pads, rhw = preprocess.preprocess_batch(imgs, (H, W), mean, std, resize_to=resize_to, model=m)
        logits = m.forward_logits(None, preloaded=(B, H, W))
        det = m.decode2d(logits)
        geom = preprocess.frame_geometry([f.shape[:2] for f in frames], (H, W), resize_to)
        assert [(q.pad_w, q.pad_h) for q in geom] == list(pads) and [(q.rh, q.rw) for q in geom] == list(rhw)
        K_net = K_net_numpy(K_cam, geom)
        boxes = decode3d_slots(det, torch.as_tensor(K_net, device=dev), cfg.DETECTOR.dim_ref, REF_LOC)
        canvas = rdist.pack_records(det.n, det.cls, det.score, det.mproj, det.verts, det.bbox, det.topk, boxes)
        _, rows = preprocess.records_to_camera(canvas.clone(), geom, K_camera=torch.as_tensor(K_cam, device=dev), boxes=boxes, kitti=True)
        torch.cuda.synchronize()
        canvas = canvas.cpu().numpy()
        want = to_camera_numpy(canvas, geom)
        live = (want[..., 31] >= 1).sum(1)
        print('frames set %s: live slots per image %s, kept %d' % (name, live.tolist(), int((want[..., 31] == 2).sum())))
        assert (live >= 1).all(), (name, live)
        out['sets'][name] = {'resize_to': resize_to, 'frames': frames, 'imgs': imgs, 'geom': geom, 'K_net': K_net, 'canvas': canvas,
                             'want': want, 'rows': rows.cpu().numpy()}
    return out


@pytest.mark.parametrize('name', ['pad', 'resize'])
def test_engine_detect_frames_equals_the_python_path(dev, small, name):
    s = small['sets'][name]
    want = torch.from_numpy(s['want']).to(dev)
    K = torch.as_tensor(small['K_cam'], device=dev)
    eng = engine.Engine(small['engine'], dev)
    with pytest.raises(RuntimeError, match='set_frame_params'):
        eng.detect_frames(s['imgs'], K)
    eng.set_frame_params(small['mean'], small['std'], s['resize_to'])
    assert eng.info['use_graph'] == 1
    for graph in (True, False):
        eng.set_graph(graph)
        for _ in range(2):                         # the second call of graph mode replays the captured graph
            rec, rows = eng.detect_frames(s['imgs'], K, kitti=True)
            torch.cuda.synchronize()
            assert torch.equal(rec, want), (name, graph)
            assert np.array_equal(rows.cpu().numpy(), s['rows']), (name, graph)
        assert torch.equal(eng.detect_frames(s['imgs'], K), want)
    c, h, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert eng.lib.rtm3d_ctx_graph_stats(eng.ctx, ctypes.byref(c), ctypes.byref(h), ctypes.byref(e)) == 0
    assert c.value == 1 and h.value >= 2, (c.value, h.value)        # one capture keyed by the workspace, then replays
    # the fp32 entry is still there beside it, and still refuses a missing batch
    assert eng.lib.rtm3d_engine_detect(eng.ctx, None, None, ctypes.c_void_p(K.data_ptr()), ctypes.c_void_p(rec.data_ptr()),
                                       ctypes.c_void_p(eng.workspace.data_ptr())) != 0
    assert eng.lib.rtm3d_last_error().decode() == 'engine_detect: null argument'
    # a frame that does not fit is refused by name before anything is launched
    big = torch.zeros(small['H'] + 1, 8, 3, dtype=torch.uint8, device=dev)
    if s['resize_to'] is None:
        with pytest.raises(RuntimeError, match=r'frame 1 \(129x8'):
            eng.detect_frames([s['imgs'][0], big], K)
    with pytest.raises(RuntimeError, match='already set'):
        eng.set_frame_params(small['mean'], small['std'], s['resize_to'])
    eng.close()


def test_frames_entries_refuse_a_context_that_is_not_an_engine(dev):
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.rtm3d_ctx_create(0, ctypes.byref(ctx)) == 0
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    hw = (ctypes.c_int * 2)(8, 8)
    ptrs = (ctypes.c_void_p * 1)(buf.data_ptr())
    assert lib.rtm3d_engine_detect_frames(ctx, None, ptrs, hw, p, p, None, p) != 0
    assert lib.rtm3d_last_error().decode() == 'engine_detect_frames: the context was not made by rtm3d_engine_load'
    params = _lib.FrameParams((ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(1, 1, 1), 0)
    assert lib.rtm3d_engine_set_frame_params(ctx, ctypes.byref(params)) != 0
    assert lib.rtm3d_engine_frames_workspace_bytes(ctx) == 0
    lib.rtm3d_ctx_destroy(ctx)


# ------------------------------------------------------------------------------------------------ 4. the C example
@pytest.mark.parametrize('name', ['pad', 'resize'])
def test_c_example_writes_the_records_and_rows_of_detect_frames(dev, small, tmp_path, name):
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_detect_frames')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(REPO, 'rtm3d_amd', 'csrc'), 'example'], check=True)
    s = small['sets'][name]
    B = small['B']
    paths = {k: str(tmp_path / k) for k in ('frames', 'records', 'kitti')}
    with open(paths['frames'], 'wb') as f:
        f.write(struct.pack('<i', B))
        for fr in s['frames']:
            f.write(struct.pack('<ii', fr.shape[0], fr.shape[1]))
            f.write(fr.tobytes())
        f.write(small['K_cam'].astype('<f8').tobytes())
        f.write(np.asarray(small['mean'], '<f4').tobytes() + np.asarray(small['std'], '<f4').tobytes())
        f.write(struct.pack('<i', s['resize_to'] or 0))
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, small['engine'], paths['frames'], paths['records'], paths['kitti'], '0'],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith('engine_detect_frames: DLA-34 %d frames on a %dx%d canvas' % (B, small['H'], small['W'])), r.stdout
    assert open(paths['records'], 'rb').read() == s['want'].astype('<f4').tobytes()
    assert open(paths['kitti'], 'rb').read() == s['rows'].astype('<f8').tobytes()
    assert (s['want'][..., 31] >= 1).sum() > 0


# ------------------------------------------------------------------------------------------------ 5. the pipeline
@pytest.mark.parametrize('name', ['pad', 'resize'])
def test_pipeline_submit_uint8_camera_K(dev, small, name):
    s = small['sets'][name]
    m, B, size = small['model'], small['B'], (small['H'], small['W'])
    K_cam = torch.as_tensor(small['K_cam'], device=dev)
    pipe = Detect3DPipeline(m, B, dev, gather=False)
    for _ in range(pipe.depth + 1):                                      # every slot, and one of them twice
        i = pipe.submit_uint8(s['imgs'], K_cam, size, resize_to=s['resize_to'], camera_K=True)
        assert np.array_equal(pipe.results(i, copy=True).cpu().numpy(), s['want'])
    # the default is today's behaviour: K with the bookkeeping in, records in canvas pixels
    i = pipe.submit_uint8(s['imgs'], torch.as_tensor(s['K_net'], device=dev), size, resize_to=s['resize_to'])
    assert np.array_equal(pipe.results(i, copy=True).cpu().numpy(), s['canvas'])
    pipe.drain()
