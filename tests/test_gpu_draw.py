"""GPU: rtm3d_records_draw (csrc/draw.hip) against the numpy yardstick tests/draw_ref.py, BYTE FOR BYTE, on the case tables of
tests/draw_cases.py (their input conditions are asserted in tests/test_draw_cpu.py); the refusals; Engine.detect_frames(draw=)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine          # noqa: E402
from rtm3d_amd import draw as rdraw                  # noqa: E402
from tests import draw_ref as ref                    # noqa: E402
from tests import draw_cases as dc                   # noqa: E402
from tests.util import load_golden                   # noqa: E402

CASES = dc.cases()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def run_device(dev, case, imgs, bev, check_classes=True):
    d_imgs = [torch.from_numpy(i).to(dev) for i in imgs]
    d_bev = None if bev is None else torch.from_numpy(bev).to(dev)
    K = None if case['K'] is None else torch.as_tensor(case['K'], device=dev)
    out = rdraw.draw_records(d_imgs, torch.from_numpy(case['rec']).to(dev), K, rdraw.DrawParams(**case['params']), d_bev,
                             check_classes=check_classes)
    torch.cuda.synchronize()
    assert (out is None) == (d_bev is None) and (out is None or out.data_ptr() == d_bev.data_ptr())
    return [i.cpu().numpy() for i in d_imgs], None if d_bev is None else d_bev.cpu().numpy()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_records_draw_equals_the_yardstick(dev, case):
    imgs, bev = dc.backgrounds(case)
    want, want_bev = [i.copy() for i in imgs], None if bev is None else bev.copy()
    ref.draw(want, case['rec'], case['K'], want_bev, **case['params'])
    got, got_bev = run_device(dev, case, imgs, bev)
    for b, (g, w) in enumerate(zip(got, want)):
        diff = (g != w).any(2)
        print('%s frame %d: %d pixels painted, %d differ' % (case['name'], b, int((w != imgs[b]).any(2).sum()), int(diff.sum())))
        assert np.array_equal(g, w), (case['name'], b, np.argwhere(diff)[:8].tolist())
    if bev is not None:
        diff = (got_bev != want_bev).any(3)
        print('%s panels: %d pixels painted, %d differ' % (case['name'], int((want_bev != bev).any(3).sum()), int(diff.sum())))
        assert np.array_equal(got_bev, want_bev), (case['name'], np.argwhere(diff)[:8].tolist())
    if case['name'] == 'empty':
        assert all(np.array_equal(g, i) for g, i in zip(got, imgs)) and np.array_equal(got_bev, bev)


def test_frames_on_odd_addresses_and_a_class_outside_the_table_on_the_device(dev):
    """Frames that start 1, 2, 3 bytes off a dword boundary (views into one buffer): the byte-store path, and no byte outside
    the frames changes.  A slot whose class lies outside the table is not drawn by the kernel (it cannot report it)."""
    case = [c for c in CASES if c['name'] == 'ragged'][0]
    rec = case['rec'].copy()
    rec[0, 1, 0] = 3.0                                   # a table of three colours
    rec[1, 0, 0] = -1.0
    case = dict(case, rec=rec)
    imgs, bev = dc.backgrounds(case)
    want, want_bev = [i.copy() for i in imgs], bev.copy()
    ref.draw(want, rec, case['K'], want_bev, **case['params'])
    for off in (1, 2, 3):
        sizes = [i.size for i in imgs]
        buf = torch.full((off + sizes[0] + 5 + sizes[1] + 8,), 0xA5, dtype=torch.uint8, device=dev)
        o1 = off + sizes[0] + 5
        views = [buf[off:off + sizes[0]].view(imgs[0].shape), buf[o1:o1 + sizes[1]].view(imgs[1].shape)]
        for v, i in zip(views, imgs):
            v.copy_(torch.from_numpy(i).to(dev))
        rdraw.draw_records(views, torch.from_numpy(rec).to(dev), torch.as_tensor(case['K'], device=dev), rdraw.DrawParams(**case['params']),
                           torch.from_numpy(bev).to(dev), check_classes=False)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + sizes[0]].reshape(imgs[0].shape), want[0]), off
        assert np.array_equal(host[o1:o1 + sizes[1]].reshape(imgs[1].shape), want[1]), off
        assert (host[:off] == 0xA5).all() and (host[off + sizes[0]:o1] == 0xA5).all() and (host[o1 + sizes[1]:] == 0xA5).all(), off


def test_more_frames_than_one_launch_holds(dev):
    """B = 66 > 64 frames per launch: the second chunk's records, intrinsics and panels are offset correctly."""
    case = [c for c in CASES if c['name'] == 'ragged'][0]
    B = 66
    big = dict(case, hw=[case['hw'][b % 2] for b in range(B)], rec=np.ascontiguousarray(np.tile(case['rec'], (B // 2, 1, 1))),
               K=np.tile(case['K'], (B // 2, 1)))
    big['rec'][65, 0, 2:4] += 7.0                       # the last frame is not a copy of frame 1
    imgs, bev = dc.backgrounds(big)
    want, want_bev = [i.copy() for i in imgs], bev.copy()
    ref.draw(want[62:], big['rec'][62:], big['K'][62:], want_bev[62:], **big['params'])
    got, got_bev = run_device(dev, big, imgs, bev)
    for b in range(62, B):
        assert np.array_equal(got[b], want[b]), b
    assert np.array_equal(got_bev[62:], want_bev[62:])


def test_refusals(dev):
    lib = _lib.load()
    case = [c for c in CASES if c['name'] == 'tiny'][0]
    rec = torch.from_numpy(case['rec']).to(dev)
    img = torch.zeros(37, 53, 3, dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * 1)(img.data_ptr())

    def call(p, hw=(37, 53), K=None, bev=None):
        rc = lib.rtm3d_records_draw(None, 1, 3, rec.data_ptr(), ptrs, (ctypes.c_int * 2)(*hw), K, ctypes.byref(p), bev)
        return rc, lib.rtm3d_last_error().decode()

    p = _lib.DrawParamsC()
    assert lib.rtm3d_draw_default_params(ctypes.byref(p)) == 0
    assert (p.layers, p.source, p.min_flag, p.thickness, p.radius, p.face_alpha, p.ncls) == (15, 0, 1, 1, 5, 77, 16)
    assert call(p)[0] == 0
    torch.cuda.synchronize()
    painted = img.clone()
    assert painted.any()
    rc, msg = call(p, hw=(37, 8193))                     # a side of 8193: the error names the frame
    assert rc != 0 and 'frame 0' in msg and '8193' in msg, msg
    rc, msg = call(p, hw=(8193, 53))
    assert rc != 0 and 'frame 0' in msg, msg
    p.source = 1                                         # source 1 with a NULL K
    rc, msg = call(p)
    assert rc != 0 and 'd_K_camera' in msg, msg
    p.source, p.layers = 0, 15 | rdraw.BEV               # the bird's-eye layer with a NULL panel
    p.bev_h, p.bev_w, p.bev_m_per_px = 40, 40, 0.5
    rc, msg = call(p)
    assert rc != 0 and 'd_bev' in msg, msg
    p.layers = 15
    for ncls in (0, 17):                                 # a table outside the 16 classes the library holds
        p.ncls = ncls
        rc, msg = call(p)
        assert rc != 0 and 'classes' in msg, msg
    p.ncls = 16
    for field, bad in (('thickness', 0), ('thickness', 16), ('face_alpha', 257), ('min_flag', 0), ('layers', 0), ('layers', 32), ('radius', -1)):
        q = _lib.DrawParamsC.from_buffer_copy(p)
        setattr(q, field, bad)
        rc, msg = call(q)
        assert rc != 0 and field in msg, (field, msg)
    torch.cuda.synchronize()
    assert torch.equal(img, painted)                     # the refused calls painted nothing


def test_refusals_leave_the_frame_alone_and_python_checks_classes(dev):
    case = [c for c in CASES if c['name'] == 'tiny'][0]
    imgs, _ = dc.backgrounds(case)
    d = [torch.from_numpy(imgs[0]).to(dev)]
    rec = torch.from_numpy(case['rec']).to(dev)
    with pytest.raises(ValueError, match='class outside the colour table'):          # classes 0, 1, 2 and a table of two
        rdraw.draw_records(d, rec, None, rdraw.DrawParams(colors=dc.COLORS[:2]))
    with pytest.raises(RuntimeError, match='frame 0'):
        rdraw.draw_records([torch.zeros(1, 8193, 3, dtype=torch.uint8, device=dev)], rec, None, rdraw.DrawParams(colors=dc.COLORS))
    with pytest.raises(RuntimeError, match='d_K_camera'):
        rdraw.draw_records(d, rec, None, rdraw.DrawParams(source=1, colors=dc.COLORS))
    torch.cuda.synchronize()
    assert np.array_equal(d[0].cpu().numpy(), imgs[0])


def test_to_ppm(tmp_path):
    a = np.arange(2 * 5 * 3, dtype=np.uint8).reshape(2, 5, 3)
    rdraw.to_ppm(str(tmp_path / 'a.ppm'), a)
    assert open(str(tmp_path / 'a.ppm'), 'rb').read() == b'P6\n5 2\n255\n' + a.tobytes()


def test_engine_detect_frames_draw(dev, tmp_path):
    """Engine.detect_frames(..., draw=params) = detect_frames followed by draw_records; draw=None leaves the frames untouched."""
    g = load_golden('e2e_dla34_small.npz')
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    cfg = rtm3d_amd.kitti_config(bb)
    m = rtm3d_amd.create_model(cfg).to(dev).eval()
    m.load_state_dict(weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']), heat_gain=float(g['heat_gain'])))
    path = str(tmp_path / 'small.rtm3d')
    m.save_engine(path, B, H, W)
    mean, std = cfg.DATASET.MEAN, cfg.DATASET.STD
    x = weights.synth_images(B, H, W, seed=int(g['img_seed'])).numpy().astype(np.float64)
    v = (x * np.asarray(std, np.float64).reshape(1, 3, 1, 1) + np.asarray(mean, np.float64).reshape(1, 3, 1, 1)) * 255.0
    full = np.ascontiguousarray(np.clip(np.round(v), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
    frames = [full[0], np.ascontiguousarray(full[1][9:110, 20:243])]
    K = np.tile(g['K'], (B, 1))
    eng = engine.Engine(path, dev)
    eng.set_frame_params(mean, std, None)
    imgs = [torch.from_numpy(f).to(dev) for f in frames]
    rec = eng.detect_frames(imgs, K)                                    # draw=None
    torch.cuda.synchronize()
    assert all(np.array_equal(i.cpu().numpy(), f) for i, f in zip(imgs, frames))
    assert int((rec[..., 31] >= 1).sum()) >= 2
    params = rdraw.DrawParams(layers=rdraw.FRAME_LAYERS | rdraw.BEV, thickness=2, bev_hw=(60, 80), bev_m_per_px=0.5)
    two = [i.clone() for i in imgs]
    panels_two = rdraw.draw_records(two, rec, K, params)
    one = [i.clone() for i in imgs]
    rec_one, panels_one = eng.detect_frames(one, K, draw=params)
    torch.cuda.synchronize()
    assert torch.equal(rec_one, rec) and torch.equal(panels_one, panels_two)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    assert any(not torch.equal(a, b) for a, b in zip(one, imgs))        # something was painted
    # and it is what the yardstick paints from those records
    want = [f.copy() for f in frames]
    ref.draw(want, rec.cpu().numpy(), K, np.zeros((B, 60, 80, 3), np.uint8), layers=params.layers, thickness=2, colors=params.colors,
             bev_hw=(60, 80), bev_m_per_px=0.5)
    assert all(np.array_equal(a.cpu().numpy(), w) for a, w in zip(one, want))
    # the C example: the same engine and frames; its two PPM files are what draw_records paints with the example's parameters
    cp = rdraw.DrawParams(layers=rdraw.FRAME_LAYERS | rdraw.BEV, thickness=2, bev_hw=(400, 400), bev_m_per_px=0.2)
    c_imgs = [i.clone() for i in imgs]
    c_panels = rdraw.draw_records(c_imgs, rec, K, cp)
    torch.cuda.synchronize()
    eng.close()
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_draw_frames')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rtm3d_amd', 'csrc'), 'example'], check=True)
    fin, f_ppm, p_ppm = [str(tmp_path / n) for n in ('frames.bin', 'frame.ppm', 'panel.ppm')]
    with open(fin, 'wb') as f:
        f.write(struct.pack('<i', B))
        for fr in frames:
            f.write(struct.pack('<ii', fr.shape[0], fr.shape[1]))
            f.write(fr.tobytes())
        f.write(K.astype('<f8').tobytes())
        f.write(np.asarray(mean, '<f4').tobytes() + np.asarray(std, '<f4').tobytes())
        f.write(struct.pack('<i', 0))
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, path, fin, f_ppm, p_ppm, '0'], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith('engine_draw_frames: DLA-34 %d frames' % B), r.stdout
    assert open(f_ppm, 'rb').read() == b'P6\n%d %d\n255\n' % (W, H) + c_imgs[0].cpu().numpy().tobytes()
    assert open(p_ppm, 'rb').read() == b'P6\n400 400\n255\n' + c_panels[0].cpu().numpy().tobytes()
