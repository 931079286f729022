"""GPU: the device stage of the JPEG frames (csrc/jpeg.hip: rtm3d_frames_jpeg_idct) from synthetic coefficient buffers against
the numpy restatement tests/jpeg_ref.py, BYTE FOR BYTE - every mode, every kind of coefficients of tests/jpeg_cases.py (zero, DC
only, single extreme AC terms, picture-sized, the two wrap regimes), small sizes and sizes on either side of every tile boundary
(read from the launcher's plan), mixed chunks, 33 frames, odd destination addresses, both byte orders, 64 guard bytes around
every destination; then the whole chain, jpeg.decode on the fixture streams against libjpeg-turbo's stored pixels, its
refusals, and Engine.detect_frames_jpeg against Engine.detect_frames."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, jpeg                     # noqa: E402
from tests import jpeg_cases as cases                # noqa: E402
from tests import jpeg_ref as ref                    # noqa: E402
from tests.test_gpu_lens import small                # noqa: E402,F401  (the small engine fixture, built once for this module)

GUARD, GUARD_BYTE = 64, 0xA5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def tile():
    return cases.tile()


# ---------------------------------------------------------------------------------------------------- helpers
class Guarded(object):
    """Destinations of (h, w) frames with GUARD bytes of 0xA5 before and after each, `offset` bytes into their allocations."""

    def __init__(self, sizes, dev, offset=0):
        self.bufs, self.out = [], []
        for h, w in sizes:
            n = h * w * 3
            buf = torch.full((offset + GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
            self.bufs.append((buf, offset + GUARD, n))
            self.out.append(buf[offset + GUARD:offset + GUARD + n].view(h, w, 3))

    def guards_intact(self):
        return all(bool((b[:at] == GUARD_BYTE).all()) and bool((b[at + n:] == GUARD_BYTE).all()) for b, at, n in self.bufs)

    def untouched(self):
        return all(bool((b == GUARD_BYTE).all()) for b, _, _ in self.bufs)


def run_and_compare(frames, dev, order='rgb', dst_offset=0):
    """frames = [(coefficient buffer as numpy int16, h, w, mode)], all in ONE rtm3d_frames_jpeg_idct call (chunks of 32 inside);
    every frame against the reference, every guard byte in place."""
    g = Guarded([(f[1], f[2]) for f in frames], dev, dst_offset)
    up = [(torch.from_numpy(np.ascontiguousarray(buf)).to(dev), h, w, mode) for buf, h, w, mode in frames]
    assert all(u[0].data_ptr() % 16 == 0 for u in up)
    got = jpeg.idct(up, order, out=g.out)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, g.out))
    for i, (buf, h, w, mode) in enumerate(frames):
        want = ref.decode_coef(buf, h, w, mode, order)
        assert torch.equal(got[i].cpu(), torch.from_numpy(want)), (i, h, w, ref.MODE_NAMES[mode], order, dst_offset)
    assert g.guards_intact()


# ---------------------------------------------------------------------------------------------------- 1. the device stage
@pytest.mark.parametrize('mode', cases.MODES, ids=[ref.MODE_NAMES[m] for m in cases.MODES])
def test_small_sizes_every_kind(dev, mode):
    """Sizes 1 x 1 ... 17 x 33 x every kind of coefficients, one call (two chunks: 40 frames)."""
    rng = np.random.Generator(np.random.PCG64(10 + mode))
    frames = [(cases.coef_buffer(kind, h, w, mode, rng), h, w, mode) for kind in cases.KINDS for h, w in cases.SMALL_SIZES]
    assert len(frames) == 40
    run_and_compare(frames, dev)


@pytest.mark.parametrize('mode', cases.MODES, ids=[ref.MODE_NAMES[m] for m in cases.MODES])
def test_tile_edges(dev, tile, mode):
    """tile - 1, tile, tile + 1 in both directions and a frame of 3 x 3 tiles: pictures-sized coefficients and the 16-bit wrap
    regime; the halo blocks of the subsampled modes are exactly what differs between these sizes."""
    tw, th = tile[:2]
    assert (tw, th) == (cases.TILE_W, cases.TILE_H)
    rng = np.random.Generator(np.random.PCG64(20 + mode))
    frames = [(cases.coef_buffer(kind, h, w, mode, rng), h, w, mode) for kind in ('image', 'wrap16') for h, w in cases.edge_sizes(tw, th)]
    run_and_compare(frames, dev)


def test_mixed_chunk_of_33_frames(dev, tile):
    """33 frames of every mode and of sizes from 1 x 1 to more than a tile, in one call: two chunks, the second of one frame."""
    tw, th = tile[:2]
    rng = np.random.Generator(np.random.PCG64(30))
    sizes = cases.SMALL_SIZES + [(th + 1, 17), (9, tw + 1), (th + 9, tw + 17)]
    frames = []
    for i in range(33):
        h, w = sizes[i % len(sizes)]
        mode = cases.MODES[(i + i // 4) % 4]
        frames.append((cases.coef_buffer(cases.KINDS[5 + i % 3], h, w, mode, rng), h, w, mode))
    assert len(jpeg.plan([(0x1000, h, w, m) for _, h, w, m in frames])) == 2
    run_and_compare(frames, dev)


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_odd_destination_addresses_and_byte_orders(dev, tile, offset):
    tw, th = tile[:2]
    rng = np.random.Generator(np.random.PCG64(40 + offset))
    frames = [(cases.coef_buffer('image', h, w, mode, rng), h, w, mode) for mode in cases.MODES for h, w in ((9, 17), (17, 33), (th + 1, tw + 3))]
    for order in ('rgb', 'bgr'):
        run_and_compare(frames, dev, order, dst_offset=offset)


def test_a_frame_of_the_benchmark_size(dev):
    """375 x 1242 in 4:2:0: 60 tiles of a frame, the width no multiple of anything."""
    rng = np.random.Generator(np.random.PCG64(50))
    run_and_compare([(cases.coef_buffer('image', 375, 1242, ref.YUV420, rng), 375, 1242, ref.YUV420)], dev, 'bgr')


def test_device_stage_refuses_through_the_launcher(dev):
    rng = np.random.Generator(np.random.PCG64(60))
    buf = torch.from_numpy(cases.coef_buffer('image', 9, 17, ref.YUV420, rng)).to(dev)
    g = Guarded([(9, 17), (9, 17)], dev)
    with pytest.raises(RuntimeError, match='frame 1 has the unknown mode 7'):
        jpeg.idct([(buf, 9, 17, ref.YUV420), (buf, 9, 17, 7)], out=g.out)
    with pytest.raises(RuntimeError, match='frame 1: the coefficient buffer is not 16-byte aligned'):
        jpeg.idct([(buf, 9, 17, ref.YUV420), (buf[4:], 9, 17, ref.GREY)], out=g.out)
    with pytest.raises(ValueError, match='destination'):
        jpeg.idct([(buf, 9, 17, ref.YUV420)], out=[g.out[0][:8]])
    torch.cuda.synchronize()
    assert g.untouched()


# ---------------------------------------------------------------------------------------------------- 2. the whole chain
def test_chain_equals_libjpeg_on_every_fixture(dev):
    """jpeg.decode on all fixture streams in one call (two chunks) against the pixels libjpeg-turbo decoded them to; then again
    at once, in the other byte order and into the caller's buffers: the second staging set, while the first is in flight."""
    fx = cases.fixtures()
    names = cases.decodable()
    assert len(names) > 32
    datas = [fx[n][0] for n in names]
    got = jpeg.decode(datas)
    g = Guarded([fx[n][1].shape[:2] for n in names], dev, offset=1)
    again = jpeg.decode([np.frombuffer(d, np.uint8) for d in datas], order='bgr', out=g.out, threads=3)
    third = jpeg.decode(datas[:5], threads=1)
    torch.cuda.synchronize()
    for i, n in enumerate(names):
        want = fx[n][1]
        assert tuple(got[i].shape) == want.shape and torch.equal(got[i].cpu(), torch.from_numpy(want)), n
        assert torch.equal(again[i].cpu(), torch.from_numpy(np.ascontiguousarray(want[:, :, ::-1]))), n
    assert all(torch.equal(third[i], got[i]) for i in range(5)) and g.guards_intact()


def test_one_bad_stream_refuses_the_batch(dev):
    fx = cases.fixtures()
    good = [fx[n][0] for n in ('9x17_420_q90', '17x33_444_q90', '16x16_grey_q90')]
    sizes = [(9, 17), (17, 33), (16, 16)]
    for bad, at, word in ((fx[cases.PROGRESSIVE][0], 1, 'progressive'), (good[1][:-30], 1, 'ends before the last MCU'),
                          (cases.patch(good[2], cases.sof_offset(good[2]) + 4, [12]), 2, '12-bit')):
        datas = list(good)
        datas[at] = bad
        g = Guarded(sizes, dev)
        with pytest.raises(RuntimeError, match='frames_jpeg: frame %d: .*%s' % (at, word)):
            jpeg.decode(datas, out=g.out)
        torch.cuda.synchronize()
        assert g.untouched()
    # a destination of the wrong size is refused by the binding, one that is too small by the library
    g = Guarded(sizes, dev)
    with pytest.raises(ValueError, match='destination'):
        jpeg.decode(good, out=[g.out[0], g.out[1], g.out[2][:8]])
    arrs, ptrs, nbytes = jpeg._streams(good)
    s, cap = jpeg.staging(dev, jpeg.workspace_bytes(good))
    short = (ctypes.c_size_t * 3)(9 * 17 * 3, 17 * 33 * 3 - 1, 16 * 16 * 3)
    rc = _lib.load().rtm3d_frames_jpeg(_lib.stream_ptr(dev), 3, ptrs, nbytes, s.host.data_ptr(), s.dev.data_ptr(), cap, _lib.ptr_array(g.out), short, 0, 0)
    assert rc == 1 and 'frame 1: the destination holds 1682 bytes' in _lib.load().rtm3d_last_error().decode()
    torch.cuda.synchronize()
    assert g.untouched()
    assert all(torch.equal(a.cpu(), torch.from_numpy(fx[n][1])) for a, n in zip(jpeg.decode(good), ('9x17_420_q90', '17x33_444_q90', '16x16_grey_q90')))


# ---------------------------------------------------------------------------------------------------- 3. the engine
def test_engine_jpeg_streams_equal_detect_frames(dev, small):
    eng, K = small['engine'], small['K']
    fx = cases.fixtures()
    names = ['72x136_420_q90', '37x53_444_q90']
    datas = [fx[n][0] for n in names]
    packed = jpeg.decode(datas)
    assert all(torch.equal(p.cpu(), torch.from_numpy(fx[n][1])) for p, n in zip(packed, names))
    want_rec, want_rows = eng.detect_frames(packed, K, kitti=True)
    want_rec, want_rows = want_rec.clone(), want_rows.clone()
    for _ in range(2):                                                       # the second call replays the captured graph
        rec, rows = eng.detect_frames_jpeg(datas, K, kitti=True)
        torch.cuda.synchronize()
        assert torch.equal(rec, want_rec) and torch.equal(rows, want_rows)
    assert all(torch.equal(p, q) for p, q in zip(eng.last_packed, packed))
    # the caller's own buffers are used when given; B G R is the other byte order of the same frames
    mine = [torch.empty(72, 136, 3, dtype=torch.uint8, device=dev), torch.empty(37, 53, 3, dtype=torch.uint8, device=dev)]
    eng.detect_frames_jpeg(datas, K, order='bgr', packed=mine)
    assert eng.last_packed[0] is mine[0]
    assert all(torch.equal(p.cpu(), torch.from_numpy(np.ascontiguousarray(fx[n][1][:, :, ::-1]))) for p, n in zip(mine, names))
    with pytest.raises(ValueError, match='batches of 2'):
        eng.detect_frames_jpeg(datas[:1], K)
    # a stream that is refused, and a frame the canvas cannot hold: by name, before anything is launched
    mine[0].fill_(7)
    with pytest.raises(RuntimeError, match='progressive'):
        eng.detect_frames_jpeg([datas[0], fx[cases.PROGRESSIVE][0]], K, packed=[mine[0], torch.empty(16, 16, 3, dtype=torch.uint8, device=dev)])
    tall = cases.patch(datas[1], cases.sof_offset(datas[1]) + 5, [0, 129])         # the header says 129 rows; the canvas has 128
    with pytest.raises(RuntimeError, match=r'frame 1 \(129x53'):
        eng.detect_frames_jpeg([datas[0], tall], K, packed=[mine[0], torch.empty(129, 53, 3, dtype=torch.uint8, device=dev)])
    torch.cuda.synchronize()
    assert bool((mine[0] == 7).all())


def test_c_example(dev, small, tmp_path):
    """examples/engine_detect_jpeg.c on two fixture streams written out as files: the records of Engine.detect_frames_jpeg."""
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_detect_jpeg')
    assert os.path.exists(exe), 'build() makes the examples'
    eng, K = small['engine'], small['K']
    fx = cases.fixtures()
    names = ['72x136_420_q90', '37x53_444_q90']
    files = []
    for n in names:
        files.append(str(tmp_path / (n + '.jpg')))
        with open(files[-1], 'wb') as f:
            f.write(fx[n][0])
    assert [bytes(b) for b in jpeg.read_files(files)] == [fx[n][0] for n in names]
    params = str(tmp_path / 'params.bin')
    with open(params, 'wb') as f:
        f.write(np.asarray(K, np.float64).tobytes() + struct.pack('<3f3f2i', *(list(small['mean']) + list(small['std']) + [0, 0])))
    rec, rows = eng.detect_frames_jpeg(jpeg.read_files(files), K, kitti=True)
    torch.cuda.synchronize()
    rec, rows = rec.cpu().numpy().reshape(-1, 32), rows.cpu().numpy().reshape(-1, 16)
    r = subprocess.run([exe, small['path'], params] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split('\n')
    live = [i for i in range(len(rec)) if rec[i, 31] >= 1]
    kept = sum(1 for i in live if rows[i, 14] == 2.0)
    assert lines[0].startswith('engine_detect_jpeg: DLA-34 2 JPEG frames')
    assert lines[-1] == 'engine_detect_jpeg: %d detections, %d KITTI rows' % (len(live), kept) and len(lines) == len(live) + 2
    topk = rec.shape[0] // 2
    for line, i in zip(lines[1:-1], live):
        head = line.split(' |')[0].split()
        assert [int(head[0]), int(head[1]), int(head[2])] == [i // topk, i % topk, int(rec[i, 0])]
        assert np.array_equal(np.array([float(v) for v in head[3:]], np.float32), rec[i, [1, 20, 21, 22, 23]])
        if rows[i, 14] == 2.0:
            assert np.array_equal(np.array([float(v) for v in line.split(' |')[1].split()]), rows[i])
