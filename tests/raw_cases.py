"""The case table of the raw-sensor tests and seeded builders of sources (tests/raw_ref.py dicts).  Padding bytes hold random
data; a plane's buffer ends with the last row's own bytes: no pitch padding behind it.

The tile the sizes are chosen against is READ from rtm3d_frames_demosaic_plan (tile()), never copied: a workgroup takes
TW x TH pixels and stages `halo` samples around them; a thread writes 8 pixels of 2 rows; a launch takes 32 frames."""
import ctypes

import numpy as np

from tests import raw_ref as ref

CHUNK = 32
PATTERNS = ('rggb', 'bggr', 'grbg', 'gbrg')
METHODS = ('mhc', 'bilinear')
LAYOUT_BITS = ref.LAYOUT_BITS
# one (layout, bits) per layout, for the sweeps that are about addresses and not about the unpacking
ONE_PER_LAYOUT = [('u8', 8), ('u16', 12), ('u16_msb', 10), ('mipi10', 10), ('mipi12', 12)]


def tile():
    """(tile_w, tile_h, halo, threads) of the launcher's own plan (host only: the plane pointer is never followed)."""
    from rtm3d_amd import _lib
    s = _lib.RawSrc()
    s.plane, s.pitch, s.h, s.w, s.layout, s.bits, s.pattern = 0x1000, 8, 4, 8, 0, 8, 0
    s.ccm[0] = s.ccm[4] = s.ccm[8] = 1024
    out = (_lib.DemosaicPlan * 1)()
    _lib.check(_lib.load().rtm3d_frames_demosaic_plan(1, (_lib.RawSrc * 1)(s), 0, out), 'frames_demosaic_plan')
    return out[0].tile_w, out[0].tile_h, out[0].halo, out[0].threads


def sizes(TW, TH):
    """(h, w): the smallest frames (fold with a period of 2 and 4), a frame below, at and above one tile, more than one tile
    either way with odd remainders, and a column of two pixels that crosses a tile."""
    return [(2, 2), (2, 3), (3, 2), (3, 3), (4, 5), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, TW + 2),
            (5, 2 * TW + 3), (TH + 2, 2)]


def regimes(h, w, TW, TH, halo):
    """What a frame of h x w exercises, as a set of names (tests/test_raw_cpu.py asks that sizes() covers all of them)."""
    r = set()
    tx, ty = -(-w // TW), -(-h // TH)
    r.add('one tile' if tx * ty == 1 else 'tiles in x' if ty == 1 else 'tiles in y' if tx == 1 else 'tiles both ways')
    if h == 2 or w == 2:
        r.add('fold period 2')                   # the reflection of a reflection
    if w % TW == 0 and h % TH == 0:
        r.add('whole tiles')
    if w % TW and w % 8:
        r.add('partial run')                     # the row's last run is stored byte by byte
    if h % 2:
        r.add('odd height')                      # a thread's second row does not exist
    if 0 < w % TW <= halo or 0 < h % TH <= halo:
        r.add('last tile inside the halo')       # the last tile's pixels were all in its neighbour's halo
    if w >= 8:
        r.add('whole staged units')              # the wide loads
    if w >= 8 and w % 8:
        r.add('staged unit crosses the right border')
    return r


ALL_REGIMES = {'one tile', 'tiles in x', 'tiles in y', 'tiles both ways', 'fold period 2', 'whole tiles', 'partial run', 'odd height',
               'last tile inside the halo', 'whole staged units', 'staged unit crosses the right border'}


def pitch_steps(layout):
    """least, and least + 7 (uint16: + 6, the pitch must be even): every residue of a row's first byte modulo 4"""
    return (0, 6) if layout in ('u16', 'u16_msb') else (0, 7)


def base_offsets(layout):
    return (0, 2) if layout in ('u16', 'u16_msb') else (0, 1, 2, 3)


def random_source(layout, bits, pattern, h, w, rng, extra_pitch=0, **kw):
    """Random BYTES everywhere (padding included): uint16 samples above 2^bits - 1 and MSB-justified samples with low bits set
    occur, so the min and the shift of the layouts are exercised."""
    pitch = ref.row_bytes(layout, w) + extra_pitch
    plane = rng.integers(0, 256, (h - 1) * pitch + ref.row_bytes(layout, w), dtype=np.uint8)
    return ref.make_source(np.zeros((h, w)), layout, bits, pattern, pitch=pitch, plane=plane, **kw)


def camera_params(bits, rng):
    """Plausible per-cell parameters: a black level of ~1/16 of the range, gains between 1 and 2.5."""
    M = (1 << bits) - 1
    return {'black': [int(v) for v in rng.integers(0, M // 16 + 1, 4)], 'gain': [int(v) for v in rng.integers(1024, 2560, 4)]}


# a matrix with negative entries (rows sum to 1024) and one with entries at both bounds
CCM_NEGATIVE = [1843, -614, -205, -307, 1638, -307, -102, -717, 1843]
CCM_BOUNDS = [8192, -8192, 1024, -8192, 8192, 1024, 0, 0, 1024]


def value_source(kind, layout, bits, pattern, h, w, rng):
    """Frames of chosen VALUES: 'zero', 'full' (all M), 'checker' (0 and M by (x + y) & 1: the negative lobes of the 5 x 5
    filters reach both clamps), 'black' (a black level above some samples), 'gain' (16384 = 16.0 on every cell), 'ccm_neg',
    'ccm_bounds'."""
    M = (1 << bits) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    rand = rng.integers(0, M + 1, (h, w))
    kw = {}
    if kind == 'zero':
        s = np.zeros((h, w), np.int64)
    elif kind == 'full':
        s = np.full((h, w), M, np.int64)
    elif kind == 'checker':
        s = np.where((xx + yy) & 1, M, 0)
    elif kind == 'black':
        s, kw = rand, {'black': [M // 2, M // 3, M, 1]}
    elif kind == 'gain':
        s, kw = rand, {'gain': 16384}
    elif kind == 'ccm_neg':
        s, kw = rand, {'ccm': CCM_NEGATIVE}
    else:
        assert kind == 'ccm_bounds'
        s, kw = rand, {'ccm': CCM_BOUNDS}
    return ref.make_source(s, layout, bits, pattern, rng=rng, **kw)


VALUE_KINDS = ('zero', 'full', 'checker', 'black', 'gain', 'ccm_neg', 'ccm_bounds')


def permutation_tone(rng):
    """A tone table no index error hides behind: the low bytes of a random permutation of 0..4095."""
    return (rng.permutation(4096) & 255).astype(np.uint8)


def c_source(src, plane_ptr, tone_ptr=None):
    """A ref source dict as the library's descriptor (the plane and the table at the given addresses)."""
    from rtm3d_amd import _lib
    s = _lib.RawSrc()
    s.plane, s.d_tone = plane_ptr, tone_ptr
    s.pitch, s.h, s.w = src['pitch'], src['h'], src['w']
    s.layout, s.bits, s.pattern = ref.LAYOUT_ID[src['layout']], src['bits'], ref.PATTERN_ID[src['pattern']]
    for k in range(4):
        s.black[k], s.gain[k] = src['black'][k], src['gain'][k]
    for k in range(9):
        s.ccm[k] = src['ccm'][k]
    return s


def c_array(items):
    from rtm3d_amd import _lib
    return (_lib.RawSrc * len(items))(*items)


def null_dst(n):
    return (ctypes.c_void_p * n)()
