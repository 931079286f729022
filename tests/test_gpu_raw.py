"""GPU: rtm3d_frames_demosaic (csrc/demosaic.hip) against the numpy restatement tests/raw_ref.py, BYTE FOR BYTE, over the case
table of tests/raw_cases.py - layouts and bit depths, patterns, both methods, sizes on either side of every boundary of the tile
(read from the launcher's plan), pitches, odd base addresses, chosen sample values, tone tables, batches of mixed frames - with
64 guard bytes around every destination; the refusals through the launcher; Engine.detect_frames_raw against
Engine.detect_frames; the C example."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, raw                      # noqa: E402
from rtm3d_amd import draw as rdraw                  # noqa: E402
from tests import raw_cases as cases                 # noqa: E402
from tests import raw_ref as ref                     # noqa: E402
from tests.test_gpu_lens import small                # noqa: E402,F401  (the small engine fixture, built once for this module)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
def upload(src, dev, offset=0, shared=None):
    """A source dict of raw_ref on the device: the plane in an allocation of its own, `offset` bytes into it (torch allocations
    are 512-byte aligned, so the offset is the address modulo 4) -> raw.RawSource over a 1-D tensor.  `shared`: a cache
    id(array) -> device tensor, so that frames that share a plane or a tone table share it on the device too."""
    shared = {} if shared is None else shared
    p = src['plane']
    if id(p) not in shared:
        buf = torch.empty(offset + len(p), dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        buf[offset:].copy_(torch.from_numpy(p))
        shared[id(p)] = buf[offset:]
    tone = None
    if src['tone'] is not None:
        if id(src['tone']) not in shared:
            shared[id(src['tone'])] = torch.from_numpy(np.asarray(src['tone'], np.uint8)).to(dev)
        tone = shared[id(src['tone'])]
    s = raw.RawSource(shared[id(p)], src['layout'], src['pattern'], bits=src['bits'], size=(src['h'], src['w']), pitch=src['pitch'], tone=tone)
    s.black, s.gain, s.ccm = list(src['black']), list(src['gain']), list(src['ccm'])        # the Q10 integers themselves
    return s


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


def run_and_compare(srcs, dev, method, order, src_offset=0, dst_offset=0, want=None):
    """All of `srcs` in ONE rtm3d_frames_demosaic call (chunks of 32 inside); every frame against the reference (`want`: the
    reference frames in R G B order where the caller has them already)."""
    g = Guarded(srcs, dev, dst_offset)
    shared = {}
    got = raw.demosaic([upload(s, dev, src_offset, shared) for s in srcs], method, order, out=g.out)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, g.out))
    for i, s in enumerate(srcs):
        w = ref.demosaic(s, method) if want is None else want[i]
        w = w if order == 'rgb' else np.ascontiguousarray(w[:, :, ::-1])
        assert torch.equal(got[i].cpu(), torch.from_numpy(w)), \
            (i, s['layout'], s['bits'], s['pattern'], s['h'], s['w'], s['pitch'], method, order, src_offset, dst_offset)
    assert g.guards_intact()
    return got


# ---------------------------------------------------------------------------------------------------- 1. layouts x patterns x sizes
@pytest.mark.parametrize('layout,bits', cases.LAYOUT_BITS)
def test_layout_sweep(dev, tile, layout, bits):
    """Every size of the table x the four patterns in ONE call per method and byte order (a chunk mixes sizes and patterns);
    random bytes, a camera's black levels and gains, every third frame with a colour matrix."""
    TW, TH = tile[:2]
    rng = np.random.Generator(np.random.PCG64(ref.LAYOUT_BITS.index((layout, bits))))
    srcs = [cases.random_source(layout, bits, p, h, w, rng, ccm=(cases.CCM_NEGATIVE if (i + j) % 3 == 0 else None), **cases.camera_params(bits, rng))
            for i, p in enumerate(cases.PATTERNS) for j, (h, w) in enumerate(cases.sizes(TW, TH))]
    assert len(srcs) == 44
    for method in cases.METHODS:
        want = [ref.demosaic(s, method) for s in srcs]
        for order in ('rgb', 'bgr'):
            run_and_compare(srcs, dev, method, order, want=want)


# ---------------------------------------------------------------------------------------------------- 2. chosen values
@pytest.mark.parametrize('layout,bits', cases.LAYOUT_BITS)
def test_chosen_values(dev, tile, layout, bits):
    """All zero, all M, the checkerboard of 0 and M (both clamps of the 5 x 5 filters), a black level above some samples, gain
    16384, colour matrices with negative entries and entries at +-8192: every pattern, frames smaller than and across a tile."""
    TW, TH = tile[:2]
    rng = np.random.Generator(np.random.PCG64(50 + ref.LAYOUT_BITS.index((layout, bits))))
    srcs = [cases.value_source(kind, layout, bits, p, h, w, rng) for kind in cases.VALUE_KINDS for p in cases.PATTERNS
            for (h, w) in ((3, 3), (4, 5), (TH + 1, TW + 1))]
    for method in cases.METHODS:
        got = run_and_compare(srcs, dev, method, 'rgb')
        by_kind = {k: [g.cpu().numpy() for g in got[i * 12:(i + 1) * 12]] for i, k in enumerate(cases.VALUE_KINDS)}       # 4 patterns x 3 sizes each
        assert all((g == 0).all() for g in by_kind['zero']) and all((g == 255).all() for g in by_kind['full'])
        assert all(g.min() == 0 and g.max() == 255 for g in by_kind['checker'])


# ---------------------------------------------------------------------------------------------------- 3. addresses and pitches
@pytest.mark.parametrize('layout,bits', cases.ONE_PER_LAYOUT)
def test_address_and_pitch_sweep(dev, tile, layout, bits):
    """Plane bases at byte offsets 0..3 (uint16: 0, 2), destinations at 0..3, the least pitch and least + 7 (uint16: + 6), both
    byte orders: the same bytes come out wherever they lie.  (5, 24) is a row of three whole runs, (3, 21) ends in a partial one
    and walks the destination addresses through every residue."""
    TW, TH = tile[:2]
    rng = np.random.Generator(np.random.PCG64(100 + ref.LAYOUT_ID[layout]))
    srcs = [cases.random_source(layout, bits, cases.PATTERNS[i % 4], h, w, rng, extra, **cases.camera_params(bits, rng))
            for extra in cases.pitch_steps(layout) for i, (h, w) in enumerate([(3, 3), (4, 5), (5, 24), (3, 21), (TH + 1, TW + 1), (5, 2 * TW + 3)])]
    for method in cases.METHODS:
        want = [ref.demosaic(s, method) for s in srcs]
        for so in cases.base_offsets(layout):
            for do in (0, 1, 2, 3):
                run_and_compare(srcs, dev, method, 'bgr' if (so + do) % 2 else 'rgb', so, do, want=want)


# ---------------------------------------------------------------------------------------------------- 4. tone tables
@pytest.mark.parametrize('layout,bits', [('u8', 8), ('mipi10', 10), ('u16_msb', 10), ('mipi12', 12), ('u16', 12), ('u16', 16), ('u16_msb', 16)])
def test_tone_tables(dev, tile, layout, bits):
    """A random-permutation table at 8, 10, 12 and 16 bits (an index error cannot hide), NULL against the 'linear' table, and the
    table at addresses that are no multiple of 16."""
    TW, TH = tile[:2]
    rng = np.random.Generator(np.random.PCG64(150 + bits))
    perm = cases.permutation_tone(rng)
    lin = raw.tone_table('linear').numpy()
    shapes = [(3, 3), (4, 5), (TH + 1, TW + 1)]
    for method in cases.METHODS:
        srcs = [cases.random_source(layout, bits, p, h, w, rng, tone=perm, ccm=(cases.CCM_NEGATIVE if i % 2 else None)) for i, p in enumerate(cases.PATTERNS)
                for (h, w) in shapes]
        got = run_and_compare(srcs, dev, method, 'rgb')
        null = [dict(s, tone=None) for s in srcs]
        linear = [dict(s, tone=lin) for s in srcs]
        a, b = run_and_compare(null, dev, method, 'rgb'), run_and_compare(linear, dev, method, 'rgb')
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert not any(torch.equal(x, y) for x, y in zip(a, got))                                          # the table was read
        # the table is plain data at any byte address: 1 and 8 bytes into an allocation (the kernel stages it 16 bytes at a time)
        for off in (1, 8):
            buf = torch.empty(off + 4096, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[off:].copy_(torch.from_numpy(perm))
            ups = [upload(s, dev) for s in srcs]
            for u in ups:
                u.tone = buf[off:]
            g = Guarded(srcs, dev)
            raw.demosaic(ups, method, 'rgb', out=g.out)
            torch.cuda.synchronize()
            assert g.guards_intact() and all(torch.equal(x, y) for x, y in zip(g.out, got))


# ---------------------------------------------------------------------------------------------------- 5. batches
def test_batches_of_mixed_frames(dev, tile):
    """B = 1, and B = 2 x 32 + 3 = 67 with layouts, bit depths, patterns, sizes, pitches and parameters mixed within one call,
    some frames sharing a plane and a tone table: every frame as on its own."""
    TW, TH = tile[:2]
    rng = np.random.Generator(np.random.PCG64(7))
    sizes = cases.sizes(TW, TH)
    perm = cases.permutation_tone(rng)
    srcs = []
    for i in range(2 * cases.CHUNK + 3):
        layout, bits = cases.LAYOUT_BITS[(i * 7 + 3) % len(cases.LAYOUT_BITS)]
        h, w = sizes[(i * 5 + 1) % len(sizes)]
        srcs.append(cases.random_source(layout, bits, cases.PATTERNS[(i * 3) % 4], h, w, rng, cases.pitch_steps(layout)[i % 2],
                                        tone=perm if i % 3 == 0 else None, ccm=cases.CCM_NEGATIVE if i % 4 == 1 else None, **cases.camera_params(bits, rng)))
    # frames that share ONE plane (and, every third, ONE table) on the device with a frame of another chunk, read as another pattern
    # with other parameters
    for i, j in ((5, 36), (37, 4), (66, 0), (65, 64)):
        srcs[i] = dict(srcs[j], pattern=cases.PATTERNS[(i + 1) % 4], gain=[1024 + 10 * i] * 4, tone=perm if i % 2 else None)
        assert srcs[i]['plane'] is srcs[j]['plane']
    assert len(srcs) == 67 and len({(s['layout'], s['bits']) for s in srcs[:32]}) == len(cases.LAYOUT_BITS) and len({(s['h'], s['w']) for s in srcs[:32]}) > 8
    for method in cases.METHODS:
        want = [ref.demosaic(s, method) for s in srcs]
        run_and_compare(srcs, dev, method, 'rgb', want=want)
        for i in (0, 31, 32, 63, 64, 66):                                  # the ends of every chunk, each as a call of its own
            run_and_compare([srcs[i]], dev, method, 'rgb', want=[want[i]])


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_destination_untouched(dev):
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(9))
    srcs = [cases.random_source('mipi10', 10, 'rggb', 6, 10, rng), cases.random_source('u16', 12, 'gbrg', 5, 7, rng),
            cases.random_source('u8', 8, 'bggr', 3, 3, rng)]
    up = [upload(s, dev) for s in srcs]
    g = Guarded(srcs, dev)
    dst = (ctypes.c_void_p * 3)(*[o.data_ptr() for o in g.out])
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def refused(arr, word, dst=dst, method=0, order=0):
        assert lib.rtm3d_frames_demosaic(stream, 3, arr, dst, method, order) != 0, word
        assert word in lib.rtm3d_last_error().decode(), (lib.rtm3d_last_error().decode(), word)
        torch.cuda.synchronize()
        assert g.untouched(), word

    # the LAST frame is the bad one where it can be: nothing of the good ones in front of it may have been launched
    a = raw.c_sources(up); a[2].layout = 5
    refused(a, 'frame 2 has the unknown layout 5')
    a = raw.c_sources(up); a[2].pattern = 4
    refused(a, 'frame 2 has the unknown pattern 4')
    refused(raw.c_sources(up), 'method 2', method=2)
    refused(raw.c_sources(up), 'dst_order 2', order=2)
    a = raw.c_sources(up); a[2].bits = 10
    refused(a, 'frame 2: layout 0 does not take 10 bits')
    a = raw.c_sources(up); a[1].bits = 9
    refused(a, 'frame 1: layout 1 does not take 9 bits')
    a = raw.c_sources(up); a[2].reserved = 5
    refused(a, 'frame 2: reserved = 5')
    a = raw.c_sources(up); a[2].pad = -1
    refused(a, 'frame 2: pad = -1')
    a = raw.c_sources(up); a[2].plane = None
    refused(a, 'frame 2: the plane is a NULL')
    refused(raw.c_sources(up), 'frame 2: the destination is a NULL', dst=(ctypes.c_void_p * 3)(dst[0], dst[1], None))
    a = raw.c_sources(up); a[2].w = 1
    refused(a, 'frame 2 is 3 x 1')
    a = raw.c_sources(up); a[2].h = 16385
    refused(a, 'frame 2 is 16385 x 3')
    a = raw.c_sources(up); a[0].pitch = 14
    refused(a, 'frame 0: pitch 14 is below')
    a = raw.c_sources(up); a[1].pitch = 15
    refused(a, 'frame 1: a uint16 plane has an odd')
    a = raw.c_sources(up); a[1].plane = a[1].plane + 1
    refused(a, 'frame 1: a uint16 plane has an odd')
    a = raw.c_sources(up); a[2].black[1] = 256
    refused(a, 'frame 2: black[1] = 256')
    a = raw.c_sources(up); a[2].gain[3] = 16385
    refused(a, 'frame 2: gain[3] = 16385')
    a = raw.c_sources(up); a[2].ccm[4] = -8193
    refused(a, 'frame 2: ccm[4] = -8193')
    # Python: a destination of the wrong shape, a plane too small for its rows, a missing pitch, unknown names
    with pytest.raises(ValueError, match='destination'):
        raw.demosaic(up, out=[o[:, :-1] for o in g.out])
    with pytest.raises(ValueError, match='holds'):
        raw.RawSource(up[0].plane[:-1], 'mipi10', 'rggb', size=(6, 10), pitch=15)
    with pytest.raises(ValueError, match='pitch'):
        raw.RawSource(up[0].plane, 'mipi10', 'rggb', size=(6, 10))
    with pytest.raises(ValueError, match='size'):
        raw.RawSource(up[0].plane.view(6, 15), 'mipi10', 'rggb')
    with pytest.raises(ValueError, match='tone'):
        raw.RawSource(up[0].plane, 'mipi10', 'rggb', size=(6, 10), pitch=15, tone=torch.zeros(4095, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='order'):
        raw.demosaic(up, order='gbr', out=g.out)
    with pytest.raises(ValueError, match='method'):
        raw.demosaic(up, 'vng', out=g.out)
    assert g.untouched()
    # and the same call, unbroken, does write
    raw.demosaic(up, out=g.out)
    torch.cuda.synchronize()
    assert g.guards_intact() and all(torch.equal(o.cpu(), torch.from_numpy(ref.demosaic(s))) for o, s in zip(g.out, srcs))


def test_raw_source_reads_geometry_from_tensor_views(dev):
    """2-D plane tensors carry their own pitch and, for bytes and uint16, their size: a crop of a larger uint16 frame (an even
    origin keeps the pattern), a uint8 frame, float parameters through the Q10 conversion."""
    rng = np.random.Generator(np.random.PCG64(21))
    big = torch.from_numpy(rng.integers(0, 4096, (20, 40), dtype=np.uint16)).to(dev)
    crop = big[4:15, 6:29]                                                          # 11 x 23 at a pitch of 80 bytes
    s = raw.RawSource(crop, 'u16', 'grbg', bits=12, black=64, gains=(1.9, 1.0, 1.4), ccm=[[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [-0.1, -0.7, 1.8]])
    assert (s.h, s.w, s.pitch) == (11, 23, 80) and s.gain == [1024, 1946, 1434, 1024] and s.ccm == cases.CCM_NEGATIVE
    flat = big.cpu().numpy().astype('<u2').view(np.uint8).reshape(-1)[4 * 80 + 12:]
    want = ref.demosaic({'layout': 'u16', 'bits': 12, 'pattern': 'grbg', 'h': 11, 'w': 23, 'pitch': 80, 'plane': flat, 'black': s.black,
                         'gain': s.gain, 'ccm': s.ccm, 'tone': None})
    assert torch.equal(raw.demosaic([s])[0].cpu(), torch.from_numpy(want))
    b8 = torch.from_numpy(rng.integers(0, 256, (7, 9), dtype=np.uint8)).to(dev)
    tone = raw.tone_table('srgb').to(dev)
    s = raw.RawSource(b8, 'u8', 'bggr', tone=tone)
    assert (s.h, s.w, s.pitch, s.bits) == (7, 9, 9, 8)
    want = ref.demosaic(ref.make_source(np.zeros((7, 9)), 'u8', 8, 'bggr', plane=b8.cpu().numpy().reshape(-1), tone=tone.cpu().numpy()), 'bilinear')
    assert torch.equal(raw.demosaic([s], 'bilinear')[0].cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError, match='contiguous'):
        raw.RawSource(big[:, ::2], 'u16', 'rggb')


# ---------------------------------------------------------------------------------------------------- 7. the engine
def bayer_frames(small, pattern='rggb'):
    """The fixture's RGB frames as 10-bit mosaics (value << 2), packed MIPI RAW10 at a pitch of 256 + the bytes of a row."""
    srcs = []
    for f in small['frames']:
        m = ref.bayer_of(f.astype(np.int64) << 2, pattern)
        srcs.append(ref.make_source(m, 'mipi10', 10, pattern, pitch=ref.row_bytes('mipi10', m.shape[1]) + 256, black=16, gain=[1100, 1024, 1024, 1300]))
    return srcs


def test_engine_raw_sources_equal_detect_frames(dev, small):
    eng, K = small['engine'], small['K']
    srcs = bayer_frames(small)
    for method in cases.METHODS:
        up = [upload(s, dev) for s in srcs]
        packed = raw.demosaic(up, method)
        assert all(torch.equal(p.cpu(), torch.from_numpy(ref.demosaic(s, method))) for p, s in zip(packed, srcs))
        want_rec, want_rows = eng.detect_frames(packed, K, kitti=True)
        want_rec, want_rows = want_rec.clone(), want_rows.clone()
        assert int((want_rec[..., 31] >= 1).sum()) > 0 and int((want_rows[..., 14] == 2).sum()) > 0
        for _ in range(2):                                                   # the second call replays the captured graph
            rec, rows = eng.detect_frames_raw(up, K, method=method, kitti=True)
            torch.cuda.synchronize()
            assert torch.equal(rec, want_rec) and torch.equal(rows, want_rows)
        assert all(torch.equal(p, q) for p, q in zip(eng.last_packed, packed))
    # the caller's own buffers are used when given; B G R is the other byte order of the same frames
    up = [upload(s, dev) for s in srcs]
    mine = [torch.empty(s['h'], s['w'], 3, dtype=torch.uint8, device=dev) for s in srcs]
    eng.detect_frames_raw(up, K, order='bgr', packed=mine)
    assert eng.last_packed[0] is mine[0]
    assert all(torch.equal(p.cpu(), torch.from_numpy(ref.demosaic(s, 'mhc', 'bgr'))) for p, s in zip(mine, srcs))
    # draw= paints into the packed frames: the same bytes as draw_records on the demosaiced frames
    packed = raw.demosaic(up)
    want_rec = eng.detect_frames(packed, K).clone()
    params = rdraw.DrawParams(thickness=2)
    rec2 = eng.detect_frames_raw(up, K, draw=params)
    painted = [p.clone() for p in packed]
    rdraw.draw_records(painted, want_rec, torch.as_tensor(K, device=dev), params, check_classes=False)
    torch.cuda.synchronize()
    assert torch.equal(rec2, want_rec) and all(torch.equal(p, q) for p, q in zip(eng.last_packed, painted))
    assert any(not torch.equal(p, q) for p, q in zip(painted, packed))                                     # something was painted
    with pytest.raises(ValueError, match='batches of 2'):
        eng.detect_frames_raw(up[:1], K)
    # a source the demosaic refuses, and one the canvas cannot hold: by name, before anything is launched
    mine[0].fill_(7)
    bad = raw.c_sources(up)
    bad[1].pad = 1
    ptrs = (ctypes.c_void_p * 2)(*[p.data_ptr() for p in mine])
    rec = torch.empty_like(want_rec)
    args = (ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), bad, ptrs, 0, 0, ctypes.c_void_p(torch.as_tensor(K, device=dev).data_ptr()),
            ctypes.c_void_p(rec.data_ptr()), None, ctypes.c_void_p(eng.frames_workspace.data_ptr()))
    assert eng.lib.rtm3d_engine_detect_frames_raw(eng.ctx, *args) != 0 and 'frame 1: pad = 1' in eng.lib.rtm3d_last_error().decode()
    args = args[:3] + (3,) + args[4:]
    assert eng.lib.rtm3d_engine_detect_frames_raw(eng.ctx, *args) != 0 and 'method 3' in eng.lib.rtm3d_last_error().decode()
    big = torch.zeros(129, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match=r'frame 1 \(129x8'):
        eng.detect_frames_raw([up[0], raw.RawSource(big, 'u8', 'rggb')], K, packed=[mine[0], torch.empty(129, 8, 3, dtype=torch.uint8, device=dev)])
    torch.cuda.synchronize()
    assert bool((mine[0] == 7).all())


def test_c_example_prints_the_rows_of_the_python_path(dev, small, tmp_path):
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_detect_raw')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(REPO, 'rtm3d_amd', 'csrc'), 'example'], check=True)
    eng, K, B = small['engine'], small['K'], small['B']
    # the example takes one size for all its files: the first frame's RAW10 file, once per frame of the batch; GRBG, a black level
    # of 16, gains (r, g, b), and the sRGB table the example builds with pow() - the C library's, as math.pow here.  The sensor
    # is modelled backwards from the fixture's frame, so that what the detector sees resembles it: linear light, divided by the
    # gains, above the black level
    pattern, method, order, black, wb = 'grbg', 'mhc', 'rgb', 16, (1.25, 1.0, 1.5)
    f = small['frames'][0]
    h, w = f.shape[:2]
    u = f.astype(np.float64) / 255.0
    lin = np.where(u <= 0.04045, u / 12.92, ((u + 0.055) / 1.055) ** 2.4)
    m = ref.bayer_of(np.rint(black + lin * 1000.0 / np.asarray(wb)).astype(np.int64), pattern)
    tone = np.array([int(math.floor((12.92 * u if u <= 0.0031308 else 1.055 * math.pow(u, 1.0 / 2.4) - 0.055) * 255.0 + 0.5))
                     for u in (k / 4095.0 for k in range(4096))], np.uint8)
    assert np.abs(tone.astype(int) - raw.tone_table('srgb').numpy().astype(int)).max() <= 1
    gain = [raw.q10(wb[c]) for c in ref.CELLS[pattern]]
    s = ref.make_source(m, 'mipi10', 10, pattern, black=black, gain=gain, tone=tone)
    conv = torch.from_numpy(ref.demosaic(s, method, order)).to(dev)
    rec, rows = eng.detect_frames([conv, conv.clone()], K, kitti=True)
    rec, rows = rec.cpu().numpy(), rows.cpu().numpy()
    print('RAW10 example frames: %d live slots, %d kept, mean |frame - demosaic| = %.2f' % (
        int((rec[..., 31] >= 1).sum()), int((rows[..., 14] == 2).sum()), np.abs(conv.cpu().numpy().astype(int) - f.astype(int)).mean()))
    frame, params = str(tmp_path / 'frame.raw10'), str(tmp_path / 'params.bin')
    with open(frame, 'wb') as fh:
        fh.write(s['plane'].tobytes())
    with open(params, 'wb') as fh:
        fh.write(K.astype('<f8').tobytes() + np.asarray(small['mean'], '<f4').tobytes() + np.asarray(small['std'], '<f4').tobytes())
        fh.write(struct.pack('<5i', 0, ref.PATTERN_ID[pattern], ref.METHOD_ID[method], 0, black) + np.asarray(wb, '<f4').tobytes())
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, small['path'], params, str(w), str(h)] + [frame] * B, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().split('\n')
    pitch = (ref.row_bytes('mipi10', w) + 255) // 256 * 256
    assert lines[0] == 'engine_detect_raw: DLA-34 %d RAW10 frames of %dx%d (pitch %d) on a 128x256 canvas' % (B, h, w, pitch), lines[0]
    live = np.argwhere(rec[..., 31] >= 1)
    kept = int((rows[..., 14] == 2).sum())
    assert lines[-1] == 'engine_detect_raw: %d detections, %d KITTI rows' % (len(live), kept) and len(lines) == len(live) + 2
    assert len(live) > 0 and kept > 0
    for line, (b, i) in zip(lines[1:-1], live):
        head, _, tail = line.partition(' | ')
        v = head.split()
        assert (int(v[0]), int(v[1]), int(v[2])) == (b, i, int(rec[b, i, 0]))
        assert np.array_equal(np.array([float(x) for x in v[3:]], np.float32), rec[b, i, [1, 20, 21, 22, 23]])
        assert bool(tail) == (rows[b, i, 14] == 2)
        if tail:
            assert np.array_equal(np.array([float(x) for x in tail.split()]), rows[b, i])
