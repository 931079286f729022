"""GPU: the device stage of the JPEG encoding (csrc/jpeg_enc.hip: rtm3d_frames_jpeg_fdct) against the numpy restatement
tests/jpeg_enc_ref.py, BIT FOR BIT over the WHOLE coefficient buffer (tables, real blocks, zero padding blocks) with guard words
around it - every mode x the small sizes, sizes on either side of every tile boundary, a mixed chunk of 33 frames, source
addresses offset by 1, 2, 3 bytes in both byte orders, the forward DCT's extremes, one 384 x 1280 frame, custom tables; then
the chain, jpeg.encode against libjpeg-turbo's stored streams, the round trip through jpeg.decode, the split Encoder, the
refusal of a batch, the bird's-eye panels and the C example."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, jpeg                     # noqa: E402
from rtm3d_amd import draw as rdraw                  # noqa: E402
from tests import jpeg_enc_cases as cases            # noqa: E402
from tests import jpeg_enc_ref as enc                # noqa: E402
from tests import jpeg_ref as ref                    # noqa: E402
from tests.test_gpu_lens import small                # noqa: E402,F401  (the small engine fixture, built once for this module)

GUARD, GUARD_WORD = 64, 0x5A5A                       # int16 before and after every coefficient buffer


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def upload(img, dev, offset=0):
    """The picture on the device, `offset` bytes into its allocation (any byte address is a legal source)."""
    buf = torch.empty(offset + img.size, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + img.size].view(img.shape)
    view.copy_(torch.from_numpy(np.array(img, order='C')))
    assert view.data_ptr() % 4 == offset % 4
    return view


def run_and_compare(frames, dev, tables=None, quality=90, order='rgb', offset=0):
    """frames = [(picture (h, w, 3) uint8, mode)], all in ONE rtm3d_frames_jpeg_fdct call (chunks of 32 inside); every whole
    buffer against the reference, every guard word in place.  `order`: the byte order of the uploaded pixels."""
    luma, chroma = jpeg._tables(quality, tables)
    srcs, bufs, arr = [], [], []
    for img, mode in frames:
        h, w = img.shape[:2]
        n = ref.layout(h, w, mode)['count']
        srcs.append(upload(img if order == 'rgb' else img[:, :, ::-1], dev, offset))
        buf = torch.full((GUARD + n + GUARD,), GUARD_WORD, dtype=torch.int16, device=dev)
        assert buf.data_ptr() % 16 == 0
        bufs.append((buf, n))
        arr.append((srcs[-1], buf[GUARD:GUARD + n], h, w, mode))
    _lib.check(_lib.load().rtm3d_frames_jpeg_fdct(_lib.stream_ptr(dev), len(arr), jpeg.c_enc_frames(arr), luma.ctypes.data, chroma.ctypes.data,
                                                  jpeg._order(order)), 'frames_jpeg_fdct')
    torch.cuda.synchronize()
    for i, ((img, mode), (buf, n)) in enumerate(zip(frames, bufs)):
        got = buf.cpu().numpy()
        want = enc.coef_buffer(img, mode, (luma, chroma))
        assert (got[:GUARD] == GUARD_WORD).all() and (got[GUARD + n:] == GUARD_WORD).all(), (i, img.shape, mode)
        assert np.array_equal(got[GUARD:GUARD + n], want), (i, img.shape, ref.MODE_NAMES[mode], order, offset,
                                                           np.flatnonzero(got[GUARD:GUARD + n] != want)[:8])


# ---------------------------------------------------------------------------------------------------- the device stage
@pytest.mark.parametrize('mode', cases.MODES, ids=[ref.MODE_NAMES[m] for m in cases.MODES])
def test_small_sizes(dev, mode):
    run_and_compare([(cases.picture(h, w, 100 + i), mode) for i, (h, w) in enumerate(cases.SMALL_SIZES)], dev)


@pytest.mark.parametrize('mode', cases.MODES, ids=[ref.MODE_NAMES[m] for m in cases.MODES])
def test_tile_edges(dev, mode):
    p = jpeg.fdct_plan([(0, 0, 8, 8, mode)])[0]
    assert (p.tile_w, p.tile_h) == (cases.TILE_W, cases.TILE_H)
    run_and_compare([(cases.picture(h, w, 200 + i), mode) for i, (h, w) in enumerate(cases.edge_sizes(p.tile_w, p.tile_h))], dev)


def test_mixed_chunk_of_33(dev):
    """Frames of different sizes and modes in one call; frame 32 starts the second chunk."""
    sizes = cases.SMALL_SIZES + [(65, 129), (63, 127), (40, 20), (2, 300)]
    frames = [(cases.picture(*sizes[i % len(sizes)], 300 + i), cases.MODES[(i + i // 4) % 4]) for i in range(33)]
    assert len(jpeg.fdct_plan([(0, 0, f.shape[0], f.shape[1], m) for f, m in frames])) == 2
    run_and_compare(frames, dev)


@pytest.mark.parametrize('order', ['rgb', 'bgr'])
@pytest.mark.parametrize('offset', [1, 2, 3])
def test_source_addresses_and_byte_orders(dev, offset, order):
    frames = [(cases.picture(h, w, 400 + i), cases.MODES[i % 4]) for i, (h, w) in enumerate([(9, 17), (16, 16), (37, 53), (65, 129), (20, 40)])]
    run_and_compare(frames, dev, order=order, offset=offset)


def test_extremes_of_the_forward_dct(dev):
    """All 0, all 255 and a checkerboard of 0 / 255 - the largest DC and the largest AC terms the transform can produce - at
    quality 100 (tables of 1), where nothing is rounded away."""
    h, w = 24, 40
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    pics = [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), np.repeat(board[:, :, None], 3, axis=2),
            np.stack([board, 255 - board, board], axis=2)]
    for q in (100, 50):
        run_and_compare([(p, m) for p in pics for m in cases.MODES], dev, quality=q)
    # the largest DC terms there are: -128 * 8 and 127 * 8 at a table entry of 1
    tables = enc.quality_tables(100)
    assert enc.coef_buffer(pics[0], ref.GREY, tables)[192] == -1024 and enc.coef_buffer(pics[1], ref.GREY, tables)[192] == 1016
    assert np.abs(enc.coef_buffer(pics[2], ref.GREY, tables)[192:].astype(np.int64)).max() > 800      # the checkerboard's corner term


def test_one_full_frame(dev):
    for mode in (ref.YUV420, ref.YUV444):
        run_and_compare([(cases.picture(384, 1280, 500), mode)], dev)


def test_custom_tables(dev):
    ones, full = np.ones(64, np.uint16), np.full(64, 255, np.uint16)
    ramp = (1 + np.arange(64) * 4).astype(np.uint16)
    for tables in ((ones, ones), (full, full), (ramp, ramp[::-1].copy())):
        run_and_compare([(cases.picture(37, 53, 600), m) for m in cases.MODES], dev, tables=tables)


def test_idct_reads_an_encoder_buffer(dev):
    """The buffer is the decoder's: rtm3d_frames_jpeg_idct of the device stage's output is the reference's decode of it."""
    img = cases.picture(37, 53, 700)
    for mode in cases.MODES:
        coef = jpeg.fdct([upload(img, dev)], ref.MODE_NAMES[mode], quality=75)
        out = jpeg.idct([(coef[0], 37, 53, mode)])
        torch.cuda.synchronize()
        want = ref.decode_coef(enc.coef_buffer(img, mode, enc.quality_tables(75)), 37, 53, mode)
        assert np.array_equal(out[0].cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- the chain
def test_chain_equals_libjpeg_on_every_fixture(dev):
    """jpeg.encode writes the very bytes libjpeg-turbo wrote, for all 92 fixture streams (batched by their parameters)."""
    groups = {}
    for name in cases.names():
        img, h, w, mode, q, ri, stream = cases.case(name)
        groups.setdefault((mode, q, ri), []).append((name, img, stream))
    n = 0
    for (mode, q, ri), items in groups.items():
        got = jpeg.encode([upload(img, dev) for _, img, _ in items], quality=q, mode=ref.MODE_NAMES[mode], restart=ri)
        for (name, _, stream), g in zip(items, got):
            assert g == stream, name
            n += 1
    assert n == 92


def test_decode_of_encode(dev):
    imgs = [cases.picture(h, w, 800 + i) for i, (h, w) in enumerate([(37, 53), (72, 136), (20, 40)])]
    for mode in cases.MODES:
        for order in ('rgb', 'bgr'):
            streams = jpeg.encode([upload(i if order == 'rgb' else i[:, :, ::-1], dev) for i in imgs], quality=75, mode=ref.MODE_NAMES[mode], order=order, restart=2)
            back = jpeg.decode(streams, order=order)
            torch.cuda.synchronize()
            for img, s, b in zip(imgs, streams, back):
                assert s == enc.encode(img, mode, 75, 2)
                assert np.array_equal(b.cpu().numpy(), ref.decode(s, order))


def test_split_encoder_over_three_batches(dev):
    """Encoder.submit / collect give the bytes of encode; three batches through two staging sets, two of them in flight at once."""
    batches = [[upload(cases.picture(h, w, 900 + 10 * b + i), dev) for i, (h, w) in enumerate(sizes)]
               for b, sizes in enumerate([[(37, 53), (72, 136)], [(65, 129), (9, 17), (20, 40)], [(16, 16)]])]
    want = [jpeg.encode(b, quality=80, mode='422', restart=3, threads=2) for b in batches]
    e = jpeg.Encoder(quality=80, mode='422', restart=3, threads=1)
    e.submit(batches[0])
    e.submit(batches[1])
    with pytest.raises(RuntimeError, match='two batches are pending'):
        e.submit(batches[2])
    got = [e.collect()]
    e.submit(batches[2])
    got += [e.collect(), e.collect()]
    assert got == want
    with pytest.raises(RuntimeError, match='nothing was submitted'):
        e.collect()


def test_one_bad_frame_refuses_the_batch(dev):
    """Nothing is launched: the coefficient memory of the staging set stays as it was."""
    good = upload(cases.picture(16, 16, 1000), dev)
    jpeg.encode([good, good])
    jpeg.encode([good, good])                                               # (both staging sets exist now, large enough for what follows)
    sets = jpeg._enc_sets[str(good.device)][0]
    for s in sets:
        s.dev.fill_(GUARD_WORD)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='frame 1: a frame of 16385 x 1'):
        jpeg.encode([good, torch.zeros(16385, 1, 3, dtype=torch.uint8, device=dev)])
    bad = np.ones(64, np.uint16)
    bad[3] = 0
    with pytest.raises(RuntimeError, match='entry 3 of the chroma table is 0'):
        jpeg.encode([good, good], tables=(np.ones(64, np.uint16), bad))
    with pytest.raises(RuntimeError, match='restart interval of 70000'):
        jpeg.encode([good], restart=70000)
    with pytest.raises(ValueError, match='contiguous uint8'):
        jpeg.encode([good, good.cpu()])
    torch.cuda.synchronize()
    assert all(bool((s.dev == GUARD_WORD).all()) for s in sets)


def test_panels_and_to_jpeg(dev, small, tmp_path):
    """The bird's-eye panels of draw_records - one (B, h, w, 3) tensor - and a painted frame encode; draw.to_jpeg writes the file."""
    eng, K = small['engine'], small['K']
    imgs = [torch.from_numpy(f).to(dev) for f in small['frames']]
    rec = eng.detect_frames(imgs, K)
    params = rdraw.DrawParams(layers=rdraw.FRAME_LAYERS | rdraw.BEV, thickness=2, bev_hw=(60, 80), bev_m_per_px=0.5)
    panels = rdraw.draw_records(imgs, rec, K, params)
    torch.cuda.synchronize()
    assert panels.shape == (2, 60, 80, 3) and bool(panels.any())
    streams = jpeg.encode(panels)
    assert [s for s in streams] == [enc.encode(p, ref.YUV420, 90) for p in panels.cpu().numpy()]
    rdraw.to_jpeg(str(tmp_path / 'f.jpg'), imgs[1], quality=85)
    assert open(str(tmp_path / 'f.jpg'), 'rb').read() == enc.encode(imgs[1].cpu().numpy(), ref.YUV420, 85)
    jpeg.write_files([str(tmp_path / 'p0.jpg'), str(tmp_path / 'p1.jpg')], streams)
    assert jpeg.read_files([str(tmp_path / 'p1.jpg')]) == [streams[1]]


def test_c_example(dev, small, tmp_path):
    """examples/engine_draw_jpeg.c on the small engine: its .jpg files are jpeg.encode of the frames and panels that draw_records
    paints with the example's parameters, byte for byte."""
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_draw_jpeg')
    assert os.path.exists(exe), 'build() makes the examples'
    eng, K, frames = small['engine'], small['K'], small['frames']
    imgs = [torch.from_numpy(f).to(dev) for f in frames]
    rec = eng.detect_frames(imgs, K)
    cp = rdraw.DrawParams(layers=rdraw.FRAME_LAYERS | rdraw.BEV, thickness=2, bev_hw=(400, 400), bev_m_per_px=0.2)
    panels = rdraw.draw_records(imgs, rec, K, cp)
    torch.cuda.synchronize()
    want_frames, want_panels = jpeg.encode(imgs), jpeg.encode(panels)
    fin = str(tmp_path / 'frames.bin')
    with open(fin, 'wb') as f:
        f.write(struct.pack('<i', len(frames)))
        for fr in frames:
            f.write(struct.pack('<ii', fr.shape[0], fr.shape[1]))
            f.write(fr.tobytes())
        f.write(np.asarray(K, '<f8').tobytes())
        f.write(np.asarray(small['mean'], '<f4').tobytes() + np.asarray(small['std'], '<f4').tobytes())
        f.write(struct.pack('<i', 0))
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, small['path'], fin, str(tmp_path / 'frame'), str(tmp_path / 'panel'), '0'], capture_output=True,
                       text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith('engine_draw_jpeg: DLA-34 2 frames'), r.stdout
    for b in range(2):
        assert open(str(tmp_path / ('frame%d.jpg' % b)), 'rb').read() == want_frames[b], b
        assert open(str(tmp_path / ('panel%d.jpg' % b)), 'rb').read() == want_panels[b], b
