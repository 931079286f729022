"""GPU: rtm3d_records_draw_tracks (csrc/draw_tracks.hip) against the numpy yardstick tests/draw_tracks_ref.py, BYTE FOR BYTE, on
the case tables of tests/draw_tracks_cases.py (their input conditions are asserted in tests/test_draw_tracks_cpu.py); against
rtm3d_records_draw where the two must agree; the refusals; Engine.detect_frames(draw=TrackDrawParams, tracker=); the C example."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine, track   # noqa: E402
from rtm3d_amd import draw as rdraw                  # noqa: E402
from tests import draw_cases as dc                   # noqa: E402
from tests import draw_tracks_ref as ref             # noqa: E402
from tests import draw_tracks_cases as tc            # noqa: E402
from tests.util import load_golden                   # noqa: E402

CASES = tc.cases()
BASE_CASES = dc.cases()
BY = {c['name']: c for c in CASES}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def tracker_of(dev, state):
    """A Tracker whose table is the hand-made one."""
    if state is None:
        return None
    T = (state.shape[1] - ref.HEADER) // ref.SLOT
    trk = track.Tracker(state.shape[0], T, None, dev)
    trk.state.copy_(torch.from_numpy(state))
    return trk


def run_device(dev, case, imgs, bev, check_classes=True):
    d_imgs = [torch.from_numpy(i).to(dev) for i in imgs]
    d_bev = None if bev is None else torch.from_numpy(bev).to(dev)
    K = None if case['K'] is None else torch.as_tensor(case['K'], device=dev)
    out = rdraw.draw_tracks(d_imgs, torch.from_numpy(case['rec']).to(dev), torch.from_numpy(case['ids']).to(dev), K,
                            rdraw.TrackDrawParams(**case['params']), tracker_of(dev, case['state']), d_bev, check_classes=check_classes)
    torch.cuda.synchronize()
    assert (out is None) == (d_bev is None) and (out is None or out.data_ptr() == d_bev.data_ptr())
    return [i.cpu().numpy() for i in d_imgs], None if d_bev is None else d_bev.cpu().numpy()


def compare(name, got, got_bev, want, want_bev):
    for b, (g, w) in enumerate(zip(got, want)):
        diff = (g != w).any(2)
        assert np.array_equal(g, w), (name, 'frame', b, int(diff.sum()), np.argwhere(diff)[:8].tolist())
    if want_bev is not None:
        diff = (got_bev != want_bev).any(3)
        assert np.array_equal(got_bev, want_bev), (name, 'panels', int(diff.sum()), np.argwhere(diff)[:8].tolist())


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_draw_tracks_equals_the_yardstick(dev, case):
    imgs, bev = tc.backgrounds(case)
    want, want_bev = [i.copy() for i in imgs], None if bev is None else bev.copy()
    stats = ref.draw(want, case['rec'], case['ids'], case['K'], want_bev, case['state'], **case['params'])
    got, got_bev = run_device(dev, case, imgs, bev)
    print(case['name'], {k: v for k, v in stats.items() if v})
    compare(case['name'], got, got_bev, want, want_bev)


@pytest.mark.parametrize('case', BASE_CASES, ids=[c['name'] for c in BASE_CASES])
def test_all_ids_zero_and_no_new_layer_equals_records_draw(dev, case):
    imgs, bev = dc.backgrounds(case)
    rec = torch.from_numpy(case['rec']).to(dev)
    K = None if case['K'] is None else torch.as_tensor(case['K'], device=dev)
    a = [torch.from_numpy(i).to(dev) for i in imgs]
    a_bev = None if bev is None else torch.from_numpy(bev).to(dev)
    rdraw.draw_records(a, rec, K, rdraw.DrawParams(**case['params']), a_bev)
    b = [torch.from_numpy(i).to(dev) for i in imgs]
    b_bev = None if bev is None else torch.from_numpy(bev).to(dev)
    ids = torch.zeros(case['rec'].shape[:2], dtype=torch.int32, device=dev)
    rdraw.draw_tracks(b, rec, ids, K, rdraw.TrackDrawParams(palette=tc.PALETTE3, names=tc.NAMES, **case['params']), None, b_bev)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and (bev is None or torch.equal(a_bev, b_bev))
    if case['name'] != 'empty':
        assert any(not np.array_equal(x.cpu().numpy(), i) for x, i in zip(a, imgs)) or not np.array_equal(a_bev.cpu().numpy(), bev)


def test_frames_on_odd_addresses_and_a_class_outside_the_table_on_the_device(dev):
    """Frames that start 1, 2, 3 bytes off a dword boundary (views into one buffer): the byte-store path under labels, and no byte
    outside the frames changes.  A slot whose class lies outside the table is not drawn by the kernel, its label included."""
    case = BY['ids_mix']
    rec = case['rec'].copy()
    rec[0, 1, 0] = 3.0                                   # a table of three colours
    rec[1, 1, 0] = -1.0
    case = dict(case, rec=rec)
    imgs, bev = tc.backgrounds(case)
    want, want_bev = [i.copy() for i in imgs], bev.copy()
    ref.draw(want, rec, case['ids'], case['K'], want_bev, None, **case['params'])
    full = [i.copy() for i in imgs]
    ref.draw(full, BY['ids_mix']['rec'], case['ids'], case['K'], bev.copy(), None, **case['params'])
    assert any(not np.array_equal(a, b) for a, b in zip(want, full))        # the two slots did paint something before
    for off in (1, 2, 3):
        sizes = [i.size for i in imgs]
        buf = torch.full((off + sizes[0] + 5 + sizes[1] + 8,), 0xA5, dtype=torch.uint8, device=dev)
        o1 = off + sizes[0] + 5
        views = [buf[off:off + sizes[0]].view(imgs[0].shape), buf[o1:o1 + sizes[1]].view(imgs[1].shape)]
        for v, i in zip(views, imgs):
            v.copy_(torch.from_numpy(i).to(dev))
        d_bev = torch.from_numpy(bev).to(dev)
        rdraw.draw_tracks(views, torch.from_numpy(rec).to(dev), torch.from_numpy(case['ids']).to(dev), torch.as_tensor(case['K'], device=dev),
                          rdraw.TrackDrawParams(**case['params']), None, d_bev, check_classes=False)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + sizes[0]].reshape(imgs[0].shape), want[0]), off
        assert np.array_equal(host[o1:o1 + sizes[1]].reshape(imgs[1].shape), want[1]), off
        assert (host[:off] == 0xA5).all() and (host[off + sizes[0]:o1] == 0xA5).all() and (host[o1 + sizes[1]:] == 0xA5).all(), off
        assert np.array_equal(d_bev.cpu().numpy(), want_bev)
    with pytest.raises(ValueError, match='class outside the colour table'):
        rdraw.draw_tracks([torch.from_numpy(i).to(dev) for i in imgs], torch.from_numpy(rec).to(dev), torch.from_numpy(case['ids']).to(dev),
                          torch.as_tensor(case['K'], device=dev), rdraw.TrackDrawParams(**case['params']))


def test_more_frames_than_one_launch_holds(dev):
    """B = 66 > 64 frames per launch: the second chunk's records, ids, tables and panels are offset correctly; the last frame's
    ids and table differ from the tiled ones."""
    case = BY['track_panel']
    B = 66
    p = dict(case['params'], layers=ref.BOX2D | ref.LABEL | ref.TRACK_BEV, label_fields=3)
    big = dict(case, hw=[case['hw'][b % 2] for b in range(B)], rec=np.ascontiguousarray(np.tile(case['rec'], (B // 2, 1, 1))),
               ids=np.ascontiguousarray(np.tile(case['ids'], (B // 2, 1))), state=np.ascontiguousarray(np.tile(case['state'], (B // 2, 1))), params=p)
    big['ids'][65] = (31, 7)
    big['state'][65] = case['state'][0]
    imgs, bev = tc.backgrounds(big)
    want, want_bev = [i.copy() for i in imgs], bev.copy()
    ref.draw(want[62:], big['rec'][62:], big['ids'][62:], None, want_bev[62:], big['state'][62:], **p)
    got, got_bev = run_device(dev, big, imgs, bev)
    compare('B66', got[62:], got_bev[62:], want[62:], want_bev[62:])
    assert not np.array_equal(got[65], got[63]) and not np.array_equal(got_bev[65], got_bev[63])


def test_without_a_fade_untouched_panel_tiles_keep_their_bytes(dev):
    """bev_fade 256: a panel of a guard pattern keeps it in every tile nothing touches (the yardstick says which those are)."""
    case = BY['track_panel']
    imgs, bev = tc.backgrounds(case)
    bev[...] = 0xA5
    want_bev = bev.copy()
    ref.draw([i.copy() for i in imgs], case['rec'], case['ids'], None, want_bev, case['state'], **case['params'])
    _, got_bev = run_device(dev, case, imgs, bev)
    assert np.array_equal(got_bev, want_bev)
    tiles = (want_bev != 0xA5).any(3).reshape(2, 5, 14, 4, 50)           # 70 x 200 is not tile-exact: count over 14 x 50 blocks
    assert (got_bev[:, :16, :64] == 0xA5).all() and 0 < tiles.any((2, 4)).sum() < 40


REFUSALS = [('npal', 0), ('npal', 33), ('font_scale', 0), ('font_scale', 5), ('label_fields', -1), ('label_fields', 16), ('bev_fade', -1),
            ('bev_fade', 257), ('vel_horizon', -0.5), ('vel_horizon', float('nan')), ('vel_horizon', float('inf'))]


def test_refusals_paint_nothing(dev):
    lib = _lib.load()
    case = BY['track_panel']
    rec = torch.from_numpy(case['rec'][:1]).to(dev)
    ids = torch.from_numpy(case['ids'][:1]).to(dev)
    trk = tracker_of(dev, case['state'][:1])
    img = torch.zeros(37, 53, 3, dtype=torch.uint8, device=dev)
    panel = torch.zeros(1, 70, 200, 3, dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * 1)(img.data_ptr())
    good = rdraw.TrackDrawParams(**dict(case['params'], layers=ref.BOX2D | ref.LABEL | ref.TRACK_BEV)).to_c()

    def call(q, hw=(37, 53), K=None, d_ids=ids.data_ptr(), T=5, state=trk.state.data_ptr(), bev=panel.data_ptr(), topk=2):
        rc = lib.rtm3d_records_draw_tracks(None, 1, topk, rec.data_ptr(), d_ids, T, state, ptrs, (ctypes.c_int * 2)(*hw), K, ctypes.byref(q), bev)
        return rc, lib.rtm3d_last_error().decode()

    assert call(good)[0] == 0
    torch.cuda.synchronize()
    painted, painted_panel = img.clone(), panel.clone()
    assert painted.any() and painted_panel.any()
    for field, bad in REFUSALS:
        q = _lib.DrawTracksParamsC.from_buffer_copy(good)
        setattr(q, field, bad)
        rc, msg = call(q)
        assert rc != 0 and field in msg, (field, bad, msg)
    # the refusals of rtm3d_records_draw, in its words
    for field, bad in (('thickness', 0), ('thickness', 16), ('face_alpha', 257), ('min_flag', 0), ('layers', 0), ('layers', 128), ('radius', -1),
                       ('ncls', 0), ('ncls', 17)):
        q = _lib.DrawTracksParamsC.from_buffer_copy(good)
        setattr(q.base, field, bad)
        rc, msg = call(q)
        assert rc != 0 and ('classes' if field == 'ncls' else field) in msg, (field, msg)
    rc, msg = call(good, hw=(37, 8193))
    assert rc != 0 and 'frame 0' in msg and '8193' in msg, msg
    q = _lib.DrawTracksParamsC.from_buffer_copy(good)
    q.base.source = 1
    rc, msg = call(q)
    assert rc != 0 and 'd_K_camera' in msg, msg
    q = _lib.DrawTracksParamsC.from_buffer_copy(good)
    q.base.layers |= rdraw.BEV                              # both panel bits
    rc, msg = call(q)
    assert rc != 0 and 'RTM3D_DRAW_BEV' in msg and 'RTM3D_DRAW_TRACK_BEV' in msg, msg
    q = _lib.DrawTracksParamsC.from_buffer_copy(good)
    q.label_fields = 0                                      # the label layer with nothing to write
    rc, msg = call(q)
    assert rc != 0 and 'label_fields' in msg, msg
    for kw, word in ((dict(d_ids=None), 'd_ids'), (dict(state=None), 'd_state'), (dict(bev=None), 'd_bev'), (dict(T=0), 'T 0'), (dict(T=257), 'T 257'),
                     (dict(topk=0), 'topk')):
        rc, msg = call(good, **kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert lib.rtm3d_records_draw_tracks(None, 1, 2, rec.data_ptr(), ids.data_ptr(), 5, trk.state.data_ptr(), ptrs, (ctypes.c_int * 2)(37, 53), None, None,
                                         panel.data_ptr()) != 0
    # without the track panel neither the table nor T is looked at
    q = _lib.DrawTracksParamsC.from_buffer_copy(good)
    q.base.layers = ref.BOX2D | ref.LABEL
    assert call(q, state=None, T=0, bev=None)[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(img, painted) and torch.equal(panel, painted_panel)      # the refused calls painted nothing (the last repaints the same)
    # Python: TRACK_BEV without a tracker, ids of the wrong shape
    with pytest.raises(ValueError, match='tracker'):
        rdraw.draw_tracks([img], rec, ids, None, rdraw.TrackDrawParams(**case['params']))
    with pytest.raises(ValueError, match='ids'):
        rdraw.draw_tracks([img], rec, ids[:, :1].contiguous(), None, rdraw.TrackDrawParams(layers=rdraw.BOX2D))


def test_engine_detect_frames_draws_tracks_and_the_c_example(dev, tmp_path, monkeypatch):
    """Engine.detect_frames(draw=TrackDrawParams, tracker=) over three consecutive steps = detect_frames + Tracker.update +
    draw_tracks done separately = the yardstick on those records, ids and table; the C example's PPMs are what draw_tracks paints
    with the example's parameters.  (The acceptance bar is raised as in tests/test_gpu_track.py: the fixture's weights are random.)"""
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
    mean, std = cfg.DATASET.MEAN, cfg.DATASET.STD
    x = weights.synth_images(B, H, W, seed=int(g['img_seed'])).numpy().astype(np.float64)
    v = (x * np.asarray(std, np.float64).reshape(1, 3, 1, 1) + np.asarray(mean, np.float64).reshape(1, 3, 1, 1)) * 255.0
    full = np.ascontiguousarray(np.clip(np.round(v), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
    frames = [full[0], np.ascontiguousarray(full[1][9:110, 20:243])]
    K = np.tile(g['K'], (B, 1))
    eng = engine.Engine(path, dev)
    eng.set_frame_params(mean, std, None)
    # the example's parameters
    params = rdraw.TrackDrawParams(layers=rdraw.FRAME_LAYERS | rdraw.LABEL | rdraw.TRACK_BEV, thickness=2, bev_hw=(400, 400), bev_m_per_px=0.2,
                                   label_fields=7, font_scale=2, bev_fade=200, names=['Car', 'Pedestr', 'Cyclist'])
    with pytest.raises(ValueError, match='tracker'):
        eng.detect_frames([torch.from_numpy(f).to(dev) for f in frames], K, draw=params)
    trk_a, trk_b = track.Tracker(B, 128, None, dev), track.Tracker(B, 128, None, dev)
    panels_b = torch.zeros(B, 400, 400, 3, dtype=torch.uint8, device=dev)
    want_bev = np.zeros((B, 400, 400, 3), np.uint8)
    c_frames, c_panels, labelled = [], [], 0
    for step in range(3):
        one = [torch.from_numpy(f).to(dev) for f in frames]
        rec_a, panels_a, ids_a = eng.detect_frames(one, K, draw=params, tracker=trk_a)
        two = [torch.from_numpy(f).to(dev) for f in frames]
        rec_b, ids_b = eng.detect_frames(two, K, tracker=trk_b)
        assert rdraw.draw_tracks(two, rec_b, ids_b, K, params, trk_b, panels_b, check_classes=False) is panels_b
        torch.cuda.synchronize()
        assert torch.equal(rec_a, rec_b) and torch.equal(ids_a, ids_b) and torch.equal(trk_a.state, trk_b.state)
        assert all(torch.equal(p, q) for p, q in zip(one, two))
        assert any(not np.array_equal(p.cpu().numpy(), f) for p, f in zip(one, frames))          # something was painted
        # the engine paints NEW panels every step (no trail); draw_tracks on the caller's panels keeps the trail, like the example
        fresh = np.zeros((B, 400, 400, 3), np.uint8)
        want = [f.copy() for f in frames]
        kw = dict(layers=params.layers, thickness=2, colors=params.colors, bev_hw=(400, 400), bev_m_per_px=0.2, label_fields=7, font_scale=2,
                  bev_fade=200, names=[b'Car', b'Pedestr', b'Cyclist'], palette=[tuple(c) for c in params.to_c().palette][:32])
        stats = ref.draw(want, rec_a.cpu().numpy(), ids_a.cpu().numpy(), K, fresh, trk_a.state.cpu().numpy(), **kw)
        ref.draw([f.copy() for f in frames], rec_a.cpu().numpy(), ids_a.cpu().numpy(), K, want_bev, trk_a.state.cpu().numpy(), **kw)
        labelled += stats['label_glyph']
        compare('engine step %d' % step, [p.cpu().numpy() for p in one], panels_a.cpu().numpy(), want, fresh)
        assert np.array_equal(panels_b.cpu().numpy(), want_bev), step
        assert stats['track_box'] > 0 and stats['track_text'] > 0
        c_frames.append(two[0].cpu().numpy())
        c_panels.append(panels_b[0].cpu().numpy().copy())
    assert labelled > 0
    eng.close()
    # the C example on the same three frame files
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_track_draw_frames')
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
    prefix = str(tmp_path / 'out')
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, path, prefix] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    for n in range(3):
        assert open('%s%d_frame.ppm' % (prefix, n), 'rb').read() == b'P6\n%d %d\n255\n' % (W, H) + c_frames[n].tobytes(), n
        assert open('%s%d_panel.ppm' % (prefix, n), 'rb').read() == b'P6\n400 400\n255\n' + c_panels[n].tobytes(), n
