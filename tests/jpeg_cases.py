"""Case tables of the JPEG tests (tests/test_jpeg_cpu.py, tests/test_gpu_jpeg.py): the fixture streams of
tests/golden/jpeg_cases.npz with Pillow's pixels, byte surgery on them (every refusal of the header is made from a fixture
stream), the regime table of the launch plan, and synthetic coefficient buffers for the device stage."""
import os

import numpy as np

from tests import jpeg_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_cases.npz')
MODES = [ref.GREY, ref.YUV444, ref.YUV422, ref.YUV420]
PROGRESSIVE = '16x16_420_progressive'

_cache = {}


def fixtures():
    """{name: (stream as bytes, Pillow's (h, w, 3) uint8 pixels or None for the stream that exists to be refused)}, in file order."""
    if 'fx' not in _cache:
        g = np.load(GOLDEN, allow_pickle=False)
        _cache['fx'] = {str(n): (g['s_' + str(n)].tobytes(), g['p_' + str(n)] if 'p_' + str(n) in g.files else None) for n in g['names']}
    return _cache['fx']


def decodable():
    return [n for n, (_, p) in fixtures().items() if p is not None]


def reference(name):
    """(info, coefficient buffer) of tests/jpeg_ref.py for a fixture, computed once."""
    key = ('ref', name)
    if key not in _cache:
        _cache[key] = ref.entropy_decode(fixtures()[name][0])
        _cache[key][1].setflags(write=False)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- byte surgery
def find_segment(data, marker, nth=0):
    """(offset of the 0xFF, total bytes with the marker) of the nth segment with this marker in front of the scan."""
    hits = [(at, n) for m, at, n in ref.segments(data) if m == marker]
    return hits[nth]


def cut_segments(data, marker):
    """The stream without its segments of this marker."""
    out, last = b'', 0
    for m, at, n in ref.segments(data):
        if m == marker:
            out += data[last:at]
            last = at + n
    return out + data[last:]


def patch(data, at, new):
    new = bytes(new)
    return data[:at] + new + data[at + len(new):]


def sof_offset(data):
    for m in (0xC0, 0xC1):
        try:
            return find_segment(data, m)[0]
        except IndexError:
            pass
    raise AssertionError('no SOF0 / SOF1')


def scan_offset(data):
    at, n = find_segment(data, 0xDA)
    return at + n


def dqt_16bit(data):
    """Every DQT segment rewritten with 16-bit entries of the same values."""
    out, last = b'', 0
    for m, at, n in ref.segments(data):
        if m != 0xDB:
            continue
        body, p, new = data[at + 4:at + n], 0, b''
        while p < len(body):
            assert body[p] >> 4 == 0
            new += bytes([0x10 | (body[p] & 15)]) + b''.join(bytes([0, v]) for v in body[p + 1:p + 65])
            p += 65
        out += data[last:at] + b'\xff\xdb' + bytes([(len(new) + 2) >> 8, (len(new) + 2) & 255]) + new
        last = at + n
    return out + data[last:]


def restart_markers(data):
    """Offsets of the RSTn markers inside the scan."""
    i, out = scan_offset(data), []
    while i + 1 < len(data):
        if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7:
            out.append(i)
        i += 1
    return out


def refusals():
    """[(name of the case, the mangled stream, a word the message must hold)]: every refusal of the header, each made from a
    fixture stream."""
    fx = fixtures()
    base = fx['16x16_420_q90'][0]
    grey = fx['16x16_grey_q90'][0]
    rst = fx['37x53_420_q90_r1'][0]
    opt = fx['17x33_420_q30_opt'][0]
    sof = sof_offset(base)
    sos_at, sos_n = find_segment(base, 0xDA)
    scan = scan_offset(base)
    marks = restart_markers(rst)
    out = [
        ('progressive', fx[PROGRESSIVE][0], 'progressive'),
        ('lossless', patch(base, sof + 1, [0xC3]), 'lossless'),
        ('hierarchical', patch(base, sof + 1, [0xC5]), 'hierarchical'),
        ('arithmetic', patch(base, sof + 1, [0xC9]), 'arithmetic'),
        ('12 bit', patch(base, sof + 4, [12]), '12-bit'),
        ('2 components', patch(patch(base, sof + 9, [2]), sof + 2, [0, 14]), '2 components'),
        ('4 components', patch(patch(base, sof + 9, [4]), sof + 2, [0, 20]), '4 components'),
        ('sampling 1x2', patch(base, sof + 11, [0x12]), 'sampling'),
        ('sampling 4x1', patch(base, sof + 11, [0x41]), 'sampling'),
        ('chroma 2x1', patch(base, sof + 14, [0x21]), 'sampling'),
        # a scan of one component of three: the first of several
        ('several scans (Ns)', base[:sos_at] + b'\xff\xda\x00\x08\x01' + base[sos_at + 5:sos_at + 7] + b'\x00\x3f\x00' + base[scan:], 'several scans'),
        # a second SOS behind the complete scan
        ('several scans (second SOS)', base[:-2] + base[sos_at:sos_at + sos_n] + b'\x00\xff\xd9', 'several scans'),
        ('progressive scan parameters', patch(base, sos_at + sos_n - 2, [5]), 'Se 5'),
        ('quantisation table never defined', patch(base, sof + 12, [3]), 'never defined'),
        ('huffman table never defined', patch(base, sos_at + 6, [0x22]), 'never defined'),
        ('code not in table', opt[:scan_offset(opt)] + b'\xff\x00' * 40 + b'\xff\xd9', 'not in'),
        ('entropy data ends', base[:scan + (len(base) - scan) // 2] + b'\xff\xd9', 'ends before the last MCU'),
        ('entropy data ends without EOI', base[:scan + (len(base) - scan) // 2], 'ends before the last MCU'),
        ('restart marker missing', rst[:marks[2]] + rst[marks[2] + 2:], 'restart marker'),
        ('restart marker out of sequence', patch(rst, marks[2] + 1, [0xD5]), 'out of sequence'),
        ('h of 0', patch(base, sof + 5, [0, 0]), '0 x 16'),
        ('w of 0', patch(base, sof + 7, [0, 0]), '16 x 0'),
        ('h above 16384', patch(base, sof + 5, [0x40, 0x01]), '16385 x 16'),
        ('w above 16384', patch(base, sof + 7, [0xFF, 0xFF]), '16 x 65535'),
        ('segment length past the end', patch(base, dht_at_of(base) + 2, [0xFF, 0xFF]), 'runs past the end'),
        ('segment length past the end (cut)', base[:dht_at_of(base) + 20], 'runs past the end'),
        ('adobe transform 0', base[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00' + base[2:], 'Adobe'),
        ('no SOI', b'\x00' + base[1:], 'SOI'),
        ('grey 12 bit', patch(grey, sof_offset(grey) + 4, [12]), '12-bit'),
    ]
    # a run that passes coefficient 63, with a table of two codes made for it: '0' = run 15 size 1, '10' = end of block.  The DC
    # table is Annex K's (the DHT segments are cut), where '00' is size 0; then (run 15, size 1, value bit) again and again: the fourth lands on coefficient 64
    dht = b'\xff\xc4\x00\x15\x10' + bytes([1, 1] + [0] * 14) + bytes([0xF1, 0x00])
    head = cut_segments(grey, 0xC4)
    s_at = find_segment(head, 0xDA)[0]
    out.append(('run passes 63', head[:s_at] + dht + head[s_at:scan_offset(head)] + bytes([0b00010101, 0b01010101]) + b'\xff\xd9', 'passes coefficient 63'))
    return out


def dht_at_of(data):
    return find_segment(data, 0xC4)[0]


# ---------------------------------------------------------------------------------------------------- the plan
def tile():
    """(tile_w, tile_h, halo, threads) as the library's plan reports them."""
    from rtm3d_amd import jpeg
    p = jpeg.plan([(0x1000, 8, 8, ref.GREY)])[0]
    return p.tile_w, p.tile_h, p.halo, p.threads


# what the header promises: tiles of 128 x 64 pixels, one chroma sample of halo, 256 threads, 32 frames per chunk
TILE_W, TILE_H, HALO, THREADS, CHUNK = 128, 64, 1, 256, 32


def plan_regimes():
    """[(sizes (h, w) of a batch, the expected (first, count, tiles, grid_x, grid_y) per chunk)]"""
    return [
        ([(1, 1)], [(0, 1, 1, 1, 1)]),
        ([(TILE_H, TILE_W)], [(0, 1, 1, 1, 1)]),
        ([(TILE_H + 1, TILE_W)], [(0, 1, 2, 2, 1)]),
        ([(TILE_H, TILE_W + 1)], [(0, 1, 2, 2, 1)]),
        ([(375, 1242)], [(0, 1, 60, 60, 1)]),
        ([(8, 8), (375, 1242), (65, 129)], [(0, 3, 60, 60, 3)]),
        ([(16384, 16384)], [(0, 1, 128 * 256, 128 * 256, 1)]),
        ([(9, 17)] * 32 + [(65, 17)], [(0, 32, 1, 1, 32), (32, 1, 2, 2, 1)]),
        ([(9, 17)] * 65, [(0, 32, 1, 1, 32), (32, 32, 1, 1, 32), (64, 1, 1, 1, 1)]),
    ]


# ---------------------------------------------------------------------------------------------------- synthetic coefficients
SMALL_SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (17, 33)]


def edge_sizes(tw=TILE_W, th=TILE_H):
    """Sizes on either side of every tile boundary."""
    return [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (9, tw + 1), (th + 1, 17), (2 * th + 3, 2 * tw + 5)]


def coef_buffer(kind, h, w, mode, rng):
    """A coefficient buffer (int16, ref.layout(h, w, mode)['count']) of one of the kinds:
    'zero'     all coefficients 0, tables 1;
    'dc'       random DC terms only, tables up to 255;
    ('ac', k)  a single extreme term +-32767 at coefficient k of every block, tables 1 (k = 1, 8, 63);
    'image'    coefficients of the size real pictures have (|c| q within a few thousand), tables up to 64;
    'wrap8'    full-range random int16, tables up to 255: pass 2 of the inverse DCT wraps;
    'wrap16'   full-range random int16, 16-bit tables: the dequantisation wraps too."""
    L = ref.layout(h, w, mode)
    buf = np.zeros(L['count'], np.int16)
    n = L['count'] - ref.TABLE_WORDS
    q = np.ones(64 * L['ncomp'], np.int64)
    if kind == 'zero':
        pass
    elif kind == 'dc':
        buf[ref.TABLE_WORDS::64] = rng.integers(-1024, 1024, n // 64)
        q = rng.integers(1, 256, q.size)
    elif isinstance(kind, tuple):
        buf[ref.TABLE_WORDS + kind[1]::64] = rng.choice(np.array([-32767, 32767, -32768], np.int16), n // 64)
    elif kind == 'image':
        c = rng.integers(-40, 41, n) * (rng.random(n) < 0.3)
        c[0::64] = rng.integers(-60, 61, n // 64)
        buf[ref.TABLE_WORDS:] = c
        q = rng.integers(1, 65, q.size)
    elif kind == 'wrap8':
        buf[ref.TABLE_WORDS:] = rng.integers(-32768, 32768, n)
        q = rng.integers(1, 256, q.size)
    elif kind == 'wrap16':
        buf[ref.TABLE_WORDS:] = rng.integers(-32768, 32768, n)
        q = rng.integers(1, 65536, q.size)
    else:
        raise ValueError(kind)
    buf[:q.size] = q.astype(np.uint16).view(np.int16)
    return buf


KINDS = ['zero', 'dc', ('ac', 1), ('ac', 8), ('ac', 63), 'image', 'wrap8', 'wrap16']
