"""numpy restatement of the raw-sensor rule of include/rtm3d_hip.h ("raw sensor frames"): sample layouts, black level, white
balance, the folded Malvar-He-Cutler / bilinear demosaic, colour matrix, tone table, byte order.  Vectorised (fold indices
through np.take), int64 throughout - the rule keeps every intermediate below 2^31, which demosaic() asserts.

A source is a dict: layout, bits, pattern (names), h, w, pitch, plane (uint8 array of (h - 1) * pitch + row bytes at least),
black[4], gain[4] (Q10), ccm[9] (Q10), tone (None or uint8[4096])."""
import numpy as np

LAYOUT_ID = {'u8': 0, 'u16': 1, 'u16_msb': 2, 'mipi10': 3, 'mipi12': 4}
LAYOUT_BITS = [('u8', 8), ('u16', 10), ('u16', 12), ('u16', 14), ('u16', 16), ('u16_msb', 10), ('u16_msb', 12), ('u16_msb', 14),
               ('u16_msb', 16), ('mipi10', 10), ('mipi12', 12)]
PATTERN_ID = {'rggb': 0, 'bggr': 1, 'grbg': 2, 'gbrg': 3}
# colour (0 R, 1 G, 2 B) of cells k = (y & 1) * 2 + (x & 1)
CELLS = {'rggb': (0, 1, 1, 2), 'bggr': (2, 1, 1, 0), 'grbg': (1, 0, 2, 1), 'gbrg': (1, 2, 0, 1)}
METHOD_ID = {'mhc': 0, 'bilinear': 1}
IDENTITY = [1024, 0, 0, 0, 1024, 0, 0, 0, 1024]


def row_bytes(layout, w):
    return {'u8': w, 'u16': 2 * w, 'u16_msb': 2 * w, 'mipi10': 5 * ((w + 3) // 4), 'mipi12': 3 * ((w + 1) // 2)}[layout]


def pack(samples, layout, bits, pitch=None, fill=0x5A, rng=None):
    """(h, w) sample VALUES (0 .. 2^bits - 1) -> the uint8 plane of (h - 1) * pitch + row bytes bytes.  Pitch padding holds
    ``fill`` (or random bytes with ``rng``); the unused samples of a last MIPI group and, for 'u16', the bits above ``bits``
    are zero (so a 'u16' plane made here never reaches the min of the rule; planes of random bytes do)."""
    s = np.asarray(samples, dtype=np.int64)
    h, w = s.shape
    assert s.min() >= 0 and s.max() < (1 << bits)
    rb = row_bytes(layout, w)
    pitch = rb if pitch is None else pitch
    assert pitch >= rb
    rows = np.zeros((h, rb), np.uint8)
    if layout == 'u8':
        rows[:] = s
    elif layout in ('u16', 'u16_msb'):
        u = s if layout == 'u16' else s << (16 - bits)
        rows[:, 0::2], rows[:, 1::2] = u & 255, u >> 8
    elif layout == 'mipi10':
        p = np.zeros((h, 4 * ((w + 3) // 4)), np.int64)
        p[:, :w] = s
        g = p.reshape(h, -1, 4)
        out = rows.reshape(h, -1, 5)
        out[:, :, :4] = g >> 2
        out[:, :, 4] = (g[:, :, 0] & 3) | ((g[:, :, 1] & 3) << 2) | ((g[:, :, 2] & 3) << 4) | ((g[:, :, 3] & 3) << 6)
    else:
        p = np.zeros((h, 2 * ((w + 1) // 2)), np.int64)
        p[:, :w] = s
        g = p.reshape(h, -1, 2)
        out = rows.reshape(h, -1, 3)
        out[:, :, :2] = g >> 4
        out[:, :, 2] = (g[:, :, 0] & 15) | ((g[:, :, 1] & 15) << 4)
    full = np.full((h, pitch), fill, np.uint8) if rng is None else rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    full[:, :rb] = rows
    return np.ascontiguousarray(full.reshape(-1)[:(h - 1) * pitch + rb])


def unpack(plane, layout, bits, h, w, pitch):
    """The sample values s(x, y) of the rule, (h, w) int64."""
    rb = row_bytes(layout, w)
    plane = np.asarray(plane, np.uint8)
    assert pitch >= rb and plane.size >= (h - 1) * pitch + rb
    idx = (np.arange(h) * pitch)[:, None] + np.arange(rb)[None, :]
    rows = np.take(plane, idx).astype(np.int64)
    x = np.arange(w)
    if layout == 'u8':
        return rows
    if layout in ('u16', 'u16_msb'):
        u = rows[:, 0::2] | (rows[:, 1::2] << 8)
        return np.minimum(u, (1 << bits) - 1) if layout == 'u16' else u >> (16 - bits)
    if layout == 'mipi10':
        g, j = x >> 2, x & 3
        return (rows[:, 5 * g + j] << 2) | ((rows[:, 5 * g + 4] >> (2 * j)) & 3)
    g, j = x >> 1, x & 1
    return (rows[:, 3 * g + j] << 4) | ((rows[:, 3 * g + 2] >> (4 * j)) & 15)


def fold(i, n):
    """Reflection without repeating the edge, for any integer i."""
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def mosaic(src):
    """Steps 1-2: the balanced mosaic m, (h, w) int64."""
    h, w = src['h'], src['w']
    M = (1 << src['bits']) - 1
    s = unpack(src['plane'], src['layout'], src['bits'], h, w, src['pitch'])
    k = ((np.arange(h) & 1) * 2)[:, None] + (np.arange(w) & 1)[None, :]
    black, gain = np.asarray(src['black'], np.int64)[k], np.asarray(src['gain'], np.int64)[k]
    lv = np.maximum(s - black, 0)
    assert (lv * gain + 512).max() < 2 ** 31
    return np.minimum((lv * gain + 512) >> 10, M)


def demosaic(src, method='mhc', order='rgb'):
    """The packed (h, w, 3) uint8 frame of the rule."""
    h, w = src['h'], src['w']
    assert h >= 2 and w >= 2
    M = (1 << src['bits']) - 1
    m = mosaic(src)
    ys, xs = np.arange(h), np.arange(w)

    def at(dy, dx):
        return np.take(np.take(m, fold(ys + dy, h), axis=0), fold(xs + dx, w), axis=1)

    C = m
    ax1, ay1 = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
    d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    ax2, ay2 = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
    if method == 'mhc':
        clampM = lambda v: np.clip(v, 0, M)
        G = clampM((8 * C + 4 * (ax1 + ay1) - 2 * (ax2 + ay2) + 8) >> 4)
        O = clampM((12 * C + 4 * d - 3 * (ax2 + ay2) + 8) >> 4)
        H = clampM((10 * C + 8 * ax1 - 2 * d - 2 * ax2 + ay2 + 8) >> 4)
        V = clampM((10 * C + 8 * ay1 - 2 * d - 2 * ay2 + ax2 + 8) >> 4)
    else:
        assert method == 'bilinear'
        G, O, H, V = (ax1 + ay1 + 2) >> 2, (d + 2) >> 2, (ax1 + 1) >> 1, (ay1 + 1) >> 1
    cells = np.asarray(CELLS[src['pattern']])
    k = ((ys & 1) * 2)[:, None] + (xs & 1)[None, :]
    own = cells[k]                                             # colour of the pixel's own cell
    hcol, vcol = cells[k ^ 1], cells[k ^ 2]                    # colour of the horizontal / vertical neighbours
    rgb = np.zeros((h, w, 3), np.int64)
    for c in range(3):
        at_g = np.where(hcol == c, H, V)                       # at a green pixel: R and B come from H or V
        at_rb = np.where(own == c, C, O)                       # at a red / blue pixel: its own colour, or the other one
        rgb[:, :, c] = np.where(own == 1, C if c == 1 else at_g, G if c == 1 else at_rb)
    ccm = np.asarray(src['ccm'], np.int64).reshape(3, 3)
    acc = rgb @ ccm.T + 512
    assert np.abs(acc).max() < 2 ** 31
    col = np.clip(acc >> 10, 0, M)
    bits = src['bits']
    t = col >> (bits - 12) if bits >= 12 else col << (12 - bits)
    assert t.min() >= 0 and t.max() < 4096
    out = (t >> 4) if src.get('tone') is None else np.asarray(src['tone'], np.uint8).astype(np.int64)[t]
    out = out.astype(np.uint8)
    return np.ascontiguousarray(out if order == 'rgb' else out[:, :, ::-1])


def make_source(samples, layout, bits, pattern, pitch=None, black=0, gain=1024, ccm=None, tone=None, rng=None, plane=None):
    """A source dict from (h, w) sample values (packed here) or from a ready ``plane``."""
    h, w = np.asarray(samples).shape
    rb = row_bytes(layout, w)
    pitch = rb if pitch is None else pitch
    return {'layout': layout, 'bits': bits, 'pattern': pattern, 'h': h, 'w': w, 'pitch': pitch,
            'plane': pack(samples, layout, bits, pitch, rng=rng) if plane is None else plane,
            'black': [int(v) for v in np.broadcast_to(np.asarray(black), (4,))],
            'gain': [int(v) for v in np.broadcast_to(np.asarray(gain), (4,))],
            'ccm': list(IDENTITY) if ccm is None else [int(v) for v in ccm], 'tone': tone}


def bayer_of(rgb, pattern):
    """(h, w, 3) colour values -> the (h, w) mosaic a sensor with ``pattern`` samples from them."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    k = ((np.arange(h) & 1) * 2)[:, None] + (np.arange(w) & 1)[None, :]
    return np.take_along_axis(rgb, np.asarray(CELLS[pattern])[k][:, :, None], axis=2)[:, :, 0]
