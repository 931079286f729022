"""GPU: rtm3d_frames_convert (csrc/frames_convert.hip) against the numpy restatement tests/pixfmt_ref.py, BYTE FOR BYTE, over
the case table of tests/pixfmt_cases.py - formats, sizes on either side of every boundary of the thread mapping, pitches,
odd base addresses, batches of mixed frames - with 64 guard bytes around every destination; the refusals through the launcher;
Engine.detect_frames_src against Engine.detect_frames; the C example."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine, pixfmt  # noqa: E402
from rtm3d_amd import draw as rdraw                  # noqa: E402
from tests import pixfmt_cases as cases              # noqa: E402
from tests import pixfmt_ref as ref                  # noqa: E402
from tests.util import load_golden                   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_BYTE = 64, 0xA5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------------------------------- helpers
def upload(src, dev, offset=0):
    """A source dict of pixfmt_ref on the device: every plane in an allocation of its own, `offset` bytes into it (torch
    allocations are 512-byte aligned, so the offset is the address modulo 4 / 8) -> pixfmt.FrameSource over 1-D tensors."""
    planes = []
    for p in src['planes']:
        buf = torch.empty(offset + len(p), dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        buf[offset:].copy_(torch.from_numpy(p))
        planes.append(buf[offset:])
    return pixfmt.FrameSource(planes, src['format'], size=(src['h'], src['w']), pitches=src['pitches'], matrix=src['matrix'],
                              range=src['range'])


class Guarded(object):
    """Destinations with GUARD bytes of 0xA5 before and after each, `offset` bytes into their allocations."""

    def __init__(self, srcs, dev, offset=0):
        self.bufs, self.out = [], []
        for s in srcs:
            n = s['h'] * s['w'] * 3
            buf = torch.full((offset + GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
            self.bufs.append((buf, offset + GUARD, n))
            self.out.append(buf[offset + GUARD:offset + GUARD + n].view(s['h'], s['w'], 3))

    def guards_intact(self):
        return all(bool((b[:at] == GUARD_BYTE).all()) and bool((b[at + n:] == GUARD_BYTE).all()) for b, at, n in self.bufs)

    def untouched(self):
        return all(bool((b == GUARD_BYTE).all()) for b, _, _ in self.bufs)


def run_and_compare(srcs, dev, order, src_offset=0, dst_offset=0):
    """All of `srcs` in ONE rtm3d_frames_convert call (chunks of 32 inside); every frame against the reference."""
    g = Guarded(srcs, dev, dst_offset)
    got = pixfmt.convert([upload(s, dev, src_offset) for s in srcs], order, out=g.out)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, g.out))
    for i, s in enumerate(srcs):
        want = ref.convert(s, order)
        assert torch.equal(got[i].cpu(), torch.from_numpy(want)), \
            (i, s['format'], s['h'], s['w'], s['pitches'], s['matrix'], s['range'], order, src_offset, dst_offset)
    assert g.guards_intact()
    return got


# ---------------------------------------------------------------------------------------------------- 1. formats x sizes
@pytest.mark.parametrize('fmt', ref.FORMATS)
def test_format_sweep(dev, fmt):
    """Every size of the table, both destination orders, every matrix x range of a YUV format."""
    rng = np.random.Generator(np.random.PCG64(ref.FORMAT_ID[fmt]))
    for order in ('rgb', 'bgr'):
        srcs = [cases.build_source(fmt, h, w, rng, 0, m, r) for (m, r) in cases.variants(fmt) for (h, w) in cases.SIZES]
        run_and_compare(srcs, dev, order)


def test_saturated_and_anchor_samples(dev):
    """Random bytes seldom clamp on all three channels: frames of the extreme and the anchor samples of every table."""
    vals8, vals10 = [0, 1, 15, 16, 17, 127, 128, 129, 235, 236, 240, 254, 255], [0, 63, 64, 65, 511, 512, 513, 940, 960, 1022, 1023]
    srcs = []
    for m, r in cases.MATRIX_RANGE:
        Y, U, V = [a.reshape(-1) for a in np.meshgrid(vals8, vals8, vals8, indexing='ij')]
        n = len(Y)                                                              # one pixel pair per triple: w = 2 n, h = 1
        yuyv = np.stack([Y, U, Y, V], 1).astype(np.uint8).reshape(-1)
        srcs.append({'format': 'yuyv', 'h': 1, 'w': 2 * n, 'planes': [yuyv], 'pitches': [4 * n], 'matrix': m, 'range': r})
        Y, U, V = [a.reshape(-1) for a in np.meshgrid(vals10, vals10, vals10, indexing='ij')]
        n = len(Y)
        s16 = lambda a: (np.asarray(a, np.uint16) << 6).astype('<u2').view(np.uint8)
        srcs.append({'format': 'p010', 'h': 1, 'w': 2 * n, 'planes': [s16(np.repeat(Y, 2)), s16(np.stack([U, V], 1).reshape(-1))],
                     'pitches': [4 * n, 4 * n], 'matrix': m, 'range': r})
    got = run_and_compare(srcs, dev, 'rgb')
    lim = got[0].cpu().numpy().reshape(-1, 3)
    assert (lim == 0).all(1).any() and (lim == 255).all(1).any()


# ---------------------------------------------------------------------------------------------------- 2. pitches
@pytest.mark.parametrize('fmt', ref.FORMATS)
def test_pitch_sweep(dev, fmt):
    rng = np.random.Generator(np.random.PCG64(100 + ref.FORMAT_ID[fmt]))
    m, r = cases.variants(fmt)[-1]
    srcs = [cases.build_source(fmt, h, w, rng, extra, m, r) for extra in cases.pitch_steps(fmt)
            for (h, w) in cases.SMALL + cases.WIDE + cases.RUN_EDGES]
    run_and_compare(srcs, dev, 'rgb')


# ---------------------------------------------------------------------------------------------------- 3. addresses
@pytest.mark.parametrize('fmt', ref.FORMATS)
def test_address_sweep(dev, fmt):
    """Plane and destination bases at byte offsets 0, 1, 3 (P010 planes: 0, 2) into their allocations, at the least pitch and
    one byte (P010: two) above it: the same bytes come out wherever they lie.  Then the destination alone at offsets 2 and 4."""
    rng = np.random.Generator(np.random.PCG64(200 + ref.FORMAT_ID[fmt]))
    m, r = cases.variants(fmt)[0]
    srcs = [cases.build_source(fmt, h, w, rng, extra, m, r) for extra in cases.pitch_steps(fmt)[:2]
            for (h, w) in cases.WIDE + [(3, 5), (2, 129), (3, 17)]]
    first = None
    for so in cases.base_offsets(fmt):
        for do in (0, 1, 3):
            got = [t.cpu() for t in run_and_compare(srcs, dev, 'bgr', so, do)]
            first = first or got
            assert all(torch.equal(a, b) for a, b in zip(first, got))
    # destination bases 2 modulo 4 and 4 modulo 8, on rows of whole runs and rows that end in a partial one (cases.STORE_SIZES)
    srcs = [cases.build_source(fmt, h, w, rng, 0, m, r) for (h, w) in cases.STORE_SIZES]
    first = [t.cpu() for t in run_and_compare(srcs, dev, 'bgr')]
    for do in cases.STORE_OFFSETS:
        assert all(torch.equal(a, b.cpu()) for a, b in zip(first, run_and_compare(srcs, dev, 'bgr', 0, do)))


# ---------------------------------------------------------------------------------------------------- 4. batches
def test_batches_of_mixed_frames(dev):
    """B = 1, and B = 2 x 32 + 6 with formats, sizes, pitches, matrices mixed within one call: every frame as on its own."""
    rng = np.random.Generator(np.random.PCG64(7))
    sizes = cases.SMALL + cases.RUN_EDGES + cases.WIDE + cases.BLOCK_EDGES[:2]
    srcs = []
    for i in range(2 * cases.CHUNK + 6):
        fmt = ref.FORMATS[(i * 7 + 3) % len(ref.FORMATS)]
        h, w = sizes[(i * 7 + 1) % len(sizes)]
        m, r = cases.variants(fmt)[i % len(cases.variants(fmt))]
        srcs.append(cases.build_source(fmt, h, w, rng, cases.pitch_steps(fmt)[i % 3], m, r))
    assert len({s['format'] for s in srcs[:32]}) == len(ref.FORMATS) and len({(s['h'], s['w']) for s in srcs[:32]}) > 8
    many = [t.cpu() for t in run_and_compare(srcs, dev, 'rgb')]
    for i in (0, 31, 32, 63, 64, len(srcs) - 1):                     # the ends of every chunk, each as a call of its own
        assert torch.equal(run_and_compare([srcs[i]], dev, 'rgb')[0].cpu(), many[i])


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_destination_untouched(dev):
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(9))
    srcs = [cases.build_source('nv12', 6, 10, rng), cases.build_source('p010', 5, 7, rng), cases.build_source('bgra32', 3, 3, rng)]
    up = [upload(s, dev) for s in srcs]
    g = Guarded(srcs, dev)
    dst = (ctypes.c_void_p * 3)(*[o.data_ptr() for o in g.out])
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def refused(arr, word, dst=dst, order=0):
        assert lib.rtm3d_frames_convert(stream, 3, arr, dst, order) != 0, word
        assert word in lib.rtm3d_last_error().decode(), (lib.rtm3d_last_error().decode(), word)
        torch.cuda.synchronize()
        assert g.untouched(), word

    # the LAST frame is the bad one: nothing of the good ones in front of it may have been launched
    a = pixfmt.c_sources(up); a[2].format = 11
    refused(a, 'frame 2 has the unknown format 11')
    a = pixfmt.c_sources(up); a[2].reserved = 5
    refused(a, 'frame 2: reserved = 5')
    a = pixfmt.c_sources(up); a[1].matrix = 9
    refused(a, 'frame 1: unknown matrix 9')
    a = pixfmt.c_sources(up); a[1].range = 2
    refused(a, 'range 2')
    a = pixfmt.c_sources(up); a[0].plane[1] = None
    refused(a, 'frame 0: plane 1 is a NULL')
    refused(pixfmt.c_sources(up), 'frame 2: the destination is a NULL', dst=(ctypes.c_void_p * 3)(dst[0], dst[1], None))
    a = pixfmt.c_sources(up); a[2].w = 0
    refused(a, 'frame 2 is 3 x 0')
    a = pixfmt.c_sources(up); a[2].h = 16385
    refused(a, 'frame 2 is 16385 x 3')
    a = pixfmt.c_sources(up); a[2].pitch[0] = 11
    refused(a, 'frame 2: pitch 11 of plane 0 is below')
    a = pixfmt.c_sources(up); a[1].pitch[1] = 17
    refused(a, 'frame 1: plane 1 of a P010 surface has an odd')
    a = pixfmt.c_sources(up); a[1].plane[0] = a[1].plane[0] + 1
    refused(a, 'frame 1: plane 0 of a P010 surface has an odd')
    refused(pixfmt.c_sources(up), 'dst_order 2', order=2)
    # Python: a destination of the wrong shape, a plane too small for its rows, a missing pitch
    with pytest.raises(ValueError, match='destination'):
        pixfmt.convert(up, out=[o[:, :-1] for o in g.out])
    with pytest.raises(ValueError, match='holds'):
        pixfmt.FrameSource([up[0].planes[0][:-1], up[0].planes[1]], 'nv12', size=(6, 10), pitches=[10, 10])
    with pytest.raises(ValueError, match='pitches'):
        pixfmt.FrameSource(up[0].planes, 'nv12', size=(6, 10))
    with pytest.raises(ValueError, match='order'):
        pixfmt.convert(up, 'gbr', out=g.out)
    assert g.untouched()
    # and the same call, unbroken, does write
    pixfmt.convert(up, out=g.out)
    torch.cuda.synchronize()
    assert g.guards_intact() and all(torch.equal(o.cpu(), torch.from_numpy(ref.convert(s))) for o, s in zip(g.out, srcs))


def test_frame_source_reads_geometry_from_tensor_views(dev):
    """2-D and 3-D plane tensors carry their own pitch: views into a pitched surface, a crop of a larger BGRA frame."""
    rng = np.random.Generator(np.random.PCG64(21))
    h, w, pitch = 9, 21, 256
    surf = torch.from_numpy(rng.integers(0, 256, (h + (h + 1) // 2, pitch), dtype=np.uint8)).to(dev)       # NV12 as a decoder lays it out
    s = pixfmt.FrameSource.nv12(surf[:h, :w], surf[h:, :2 * ((w + 1) // 2)], matrix='bt709', range='full')
    assert (s.h, s.w, s.pitches) == (h, w, [pitch, pitch])
    flat = surf.cpu().numpy().reshape(-1)
    want = ref.convert({'format': 'nv12', 'h': h, 'w': w, 'planes': [flat, flat[h * pitch:]], 'pitches': [pitch, pitch], 'matrix': 'bt709',
                        'range': 'full'})
    assert torch.equal(pixfmt.convert([s])[0].cpu(), torch.from_numpy(want))
    big = torch.from_numpy(rng.integers(0, 256, (12, 30, 4), dtype=np.uint8)).to(dev)
    crop = big[2:9, 5:16]                                                                                  # 7 x 11, pitch 120
    s = pixfmt.FrameSource.packed(crop, 'bgra')
    assert (s.h, s.w, s.pitches) == (7, 11, [120])
    assert torch.equal(pixfmt.convert([s], 'rgb')[0], crop[:, :, [2, 1, 0]].contiguous())
    assert torch.equal(pixfmt.convert([s], 'bgr')[0], crop[:, :, :3].contiguous())
    p16 = torch.from_numpy(rng.integers(0, 65536, (6, 8), dtype=np.uint16)).to(dev)                        # P010 from uint16 tensors
    s = pixfmt.FrameSource.p010(p16[:4], p16[4:])
    assert (s.h, s.w, s.pitches) == (4, 8, [16, 16])
    raw = p16.cpu().numpy().astype('<u2').view(np.uint8).reshape(-1)
    want = ref.convert({'format': 'p010', 'h': 4, 'w': 8, 'planes': [raw, raw[64:]], 'pitches': [16, 16], 'matrix': 'bt601', 'range': 'limited'})
    assert torch.equal(pixfmt.convert([s])[0].cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError, match='contiguous'):
        pixfmt.FrameSource.gray(big[:, :, 0])


# ---------------------------------------------------------------------------------------------------- 6. the engine
def rgb_to_nv12(rgb):
    """(h, w, 3) uint8 -> Y (h, w), CbCr (ch, 2 cw) uint8: BT.601 limited range in float, chroma of the top-left pixel of each 2 x 2
    block.  Only a way to make NV12 frames with the content of the fixture's frames; nothing is compared against it."""
    f = rgb.astype(np.float64)
    y = 16 + (65.481 * f[..., 0] + 128.553 * f[..., 1] + 24.966 * f[..., 2]) / 255
    cb = 128 + (-37.797 * f[..., 0] - 74.203 * f[..., 1] + 112.0 * f[..., 2]) / 255
    cr = 128 + (112.0 * f[..., 0] - 93.786 * f[..., 1] - 18.214 * f[..., 2]) / 255
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return q(y), np.ascontiguousarray(np.stack([q(cb[::2, ::2]), q(cr[::2, ::2])], -1).reshape((rgb.shape[0] + 1) // 2, -1))


@pytest.fixture(scope='module')
def small(dev, tmp_path_factory):
    """The small synthetic engine of tests/test_gpu_frames.py (128 x 256 canvas, batch 2) and its ragged frames, as RGB tensors
    and as NV12 surfaces at a pitch of 256.  (The acceptance bar of the 3D solver is raised as in tests/test_gpu_track.py: the
    fixture's weights are random, and the KITTI rows are to hold something.)"""
    from rtm3d_amd import model_utils
    from tests.test_gpu_frames import uint8_frames
    g = load_golden('e2e_dla34_small.npz')
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    cfg = rtm3d_amd.kitti_config(bb)
    m = rtm3d_amd.create_model(cfg).to('cuda:0').eval()
    m.load_state_dict(weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']),
                                               heat_gain=float(g['heat_gain'])))
    path = str(tmp_path_factory.mktemp('pixfmt') / 'small.rtm3d')
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(model_utils, 'FUN_ACCEPT', 1e6)
        mp.setattr(engine, 'FUN_ACCEPT', 1e6)
        m.save_engine(path, B, H, W)
    full = uint8_frames(weights.synth_images(B, H, W, seed=int(g['img_seed'])), cfg.DATASET.MEAN, cfg.DATASET.STD)
    frames = [full[0], np.ascontiguousarray(full[1][9:110, 20:243])]              # the canvas itself, and 101 x 223 (odd both ways)
    K = np.tile(g['K'], (B, 1)) * np.array([[1.0], [1.03]])
    K[:, 6:] = (0, 0, 1)
    nv12 = []
    for f in frames:
        h, w = f.shape[:2]
        y, c = rgb_to_nv12(f)
        surf = np.full((h + c.shape[0], 256), 0x5A, np.uint8)
        surf[:h, :w] = y
        surf[h:, :c.shape[1]] = c
        nv12.append({'format': 'nv12', 'h': h, 'w': w, 'planes': [surf.reshape(-1), surf.reshape(-1)[h * 256:]], 'pitches': [256, 256],
                     'matrix': 'bt601', 'range': 'limited', 'file': y.tobytes() + c.tobytes()})
    eng = engine.Engine(path, dev)
    eng.set_frame_params(cfg.DATASET.MEAN, cfg.DATASET.STD, None)
    yield {'engine': eng, 'path': path, 'frames': frames, 'nv12': nv12, 'K': K, 'mean': cfg.DATASET.MEAN, 'std': cfg.DATASET.STD, 'B': B}
    eng.close()


def test_engine_rgb24_sources_equal_detect_frames(dev, small):
    eng, K = small['engine'], small['K']
    imgs = [torch.from_numpy(f).to(dev) for f in small['frames']]
    want_rec, want_rows = eng.detect_frames(imgs, K, kitti=True)
    want_rec, want_rows = want_rec.clone(), want_rows.clone()
    assert int((want_rec[..., 31] >= 1).sum()) > 0
    for _ in range(2):                                                       # the second call replays the captured graph
        rec, rows = eng.detect_frames_src([pixfmt.FrameSource.packed(i, 'rgb') for i in imgs], K, kitti=True)
        torch.cuda.synchronize()
        assert torch.equal(rec, want_rec) and torch.equal(rows, want_rows)
    assert all(torch.equal(p, i) for p, i in zip(eng.last_packed, imgs))
    # BGR rows read as BGR and written B G R are the same bytes again; the caller's own buffers are used when given
    mine = [torch.empty_like(i) for i in imgs]
    rec = eng.detect_frames_src([pixfmt.FrameSource.packed(i, 'bgr') for i in imgs], K, order='bgr', packed=mine)
    assert torch.equal(rec, want_rec) and eng.last_packed[0] is mine[0] and all(torch.equal(p, i) for p, i in zip(mine, imgs))
    with pytest.raises(ValueError, match='batches of 2'):
        eng.detect_frames_src([pixfmt.FrameSource.packed(imgs[0], 'rgb')], K)
    # a source the conversion refuses, and one the canvas cannot hold: by name, before anything is launched
    mine[0].fill_(7)
    bad = pixfmt.c_sources([pixfmt.FrameSource.packed(i, 'rgb') for i in imgs])
    bad[1].reserved = 1
    ptrs = (ctypes.c_void_p * 2)(*[p.data_ptr() for p in mine])
    args = (ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), bad, ptrs, 0, ctypes.c_void_p(torch.as_tensor(K, device=dev).data_ptr()),
            ctypes.c_void_p(rec.data_ptr()), None, ctypes.c_void_p(eng.frames_workspace.data_ptr()))
    assert eng.lib.rtm3d_engine_detect_frames_src(eng.ctx, *args) != 0 and 'frame 1: reserved = 1' in eng.lib.rtm3d_last_error().decode()
    big = torch.zeros(129, 8, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match=r'frame 1 \(129x8'):
        eng.detect_frames_src([pixfmt.FrameSource.packed(imgs[0], 'rgb'), pixfmt.FrameSource.packed(big, 'rgb')], K,
                              packed=[mine[0], torch.empty_like(big)])
    torch.cuda.synchronize()
    assert bool((mine[0] == 7).all())


def test_engine_nv12_sources_and_draw(dev, small):
    eng, K = small['engine'], small['K']
    conv = [ref.convert(s) for s in small['nv12']]
    want_rec, want_rows = eng.detect_frames([torch.from_numpy(c).to(dev) for c in conv], K, kitti=True)
    want_rec, want_rows = want_rec.clone(), want_rows.clone()
    live = int((want_rec[..., 31] >= 1).sum())
    print('NV12 frames: %d live slots, %d kept' % (live, int((want_rec[..., 31] == 2).sum())))
    assert live > 0 and int((want_rows[..., 14] == 2).sum()) > 0
    srcs = [upload(s, dev) for s in small['nv12']]
    rec, rows = eng.detect_frames_src(srcs, K, kitti=True)
    torch.cuda.synchronize()
    assert torch.equal(rec, want_rec) and torch.equal(rows, want_rows)
    assert all(torch.equal(p.cpu(), torch.from_numpy(c)) for p, c in zip(eng.last_packed, conv))
    # draw= paints into the packed frames: the same bytes as draw_records on the reference's conversion
    params = rdraw.DrawParams(thickness=2)
    rec2 = eng.detect_frames_src(srcs, K, draw=params)
    painted = [torch.from_numpy(c).to(dev) for c in conv]
    rdraw.draw_records(painted, want_rec, torch.as_tensor(K, device=dev), params, check_classes=False)
    torch.cuda.synchronize()
    assert torch.equal(rec2, want_rec)
    assert all(torch.equal(p, q) for p, q in zip(eng.last_packed, painted))
    assert any(not np.array_equal(p.cpu().numpy(), c) for p, c in zip(painted, conv))                  # something was painted
    # the BGR order is the other three-byte order of the same conversion
    eng.detect_frames_src(srcs, K, order='bgr')
    assert all(torch.equal(p.cpu(), torch.from_numpy(np.ascontiguousarray(c[:, :, ::-1]))) for p, c in zip(eng.last_packed, conv))


def test_c_example_prints_the_rows_of_the_python_path(dev, small, tmp_path):
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_detect_nv12')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(REPO, 'rtm3d_amd', 'csrc'), 'example'], check=True)
    eng, K, B = small['engine'], small['K'], small['B']
    # the example takes one size for all its files: the first frame's NV12 file, once per frame of the batch
    s = small['nv12'][0]
    conv = torch.from_numpy(ref.convert(s)).to(dev)
    rec, rows = eng.detect_frames([conv, conv.clone()], K, kitti=True)
    rec, rows = rec.cpu().numpy(), rows.cpu().numpy()
    frame, params = str(tmp_path / 'frame.nv12'), str(tmp_path / 'params.bin')
    with open(frame, 'wb') as f:
        f.write(s['file'])
    with open(params, 'wb') as f:
        f.write(K.astype('<f8').tobytes() + np.asarray(small['mean'], '<f4').tobytes() + np.asarray(small['std'], '<f4').tobytes())
        f.write(struct.pack('<4i', 0, 0, 0, 0))
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, small['path'], params, str(s['w']), str(s['h'])] + [frame] * B,
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().split('\n')
    assert lines[0] == 'engine_detect_nv12: DLA-34 %d NV12 frames of %dx%d (pitch 256) on a 128x256 canvas' % (B, s['h'], s['w']), lines[0]
    live = np.argwhere(rec[..., 31] >= 1)
    kept = int((rows[..., 14] == 2).sum())
    assert lines[-1] == 'engine_detect_nv12: %d detections, %d KITTI rows' % (len(live), kept) and len(lines) == len(live) + 2
    assert len(live) > 0 and kept > 0
    for line, (b, i) in zip(lines[1:-1], live):
        head, _, tail = line.partition(' | ')
        v = head.split()
        assert (int(v[0]), int(v[1]), int(v[2])) == (b, i, int(rec[b, i, 0]))
        assert np.array_equal(np.array([float(x) for x in v[3:]], np.float32), rec[b, i, [1, 20, 21, 22, 23]])
        assert bool(tail) == (rows[b, i, 14] == 2)
        if tail:
            assert np.array_equal(np.array([float(x) for x in tail.split()]), rows[b, i])
