"""numpy restatement of the header's "JPEG encoding": colour conversion, edge replication, chroma downsampling, the forward DCT in
fixed point, the quantiser, the quality tables, the coefficient buffer and the Huffman encoder with its marker layout - each
written separately.  The rule is libjpeg's default encode (jccolor, h2v1 / h2v2 downsampling without smoothing, jfdctint, the
Annex K Huffman tables); tests/golden/jpeg_encode_cases.npz holds the streams Pillow (libjpeg-turbo) made of the fixture
pictures, and tests/test_jpeg_enc_cpu.py requires equal bytes.  Written for clarity, one bit at a time: the library's encoder
is compared against it, not modelled on it."""
import numpy as np

from tests import jpeg_ref as ref

GREY, YUV444, YUV422, YUV420 = ref.GREY, ref.YUV444, ref.YUV422, ref.YUV420
MODES = {'grey': GREY, '444': YUV444, '422': YUV422, '420': YUV420}

# ITU-T T.81 Annex K, tables K.1 and K.2, natural order k = 8 v + u
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32)


# ---------------------------------------------------------------------------------------------------- step 6: tables
def quality_tables(quality):
    """(luma, chroma) tables of 64 in natural order for quality 1..100."""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


# ---------------------------------------------------------------------------------------------------- step 1: colour
def colour(img, order='rgb'):
    """(h, w, 3) uint8 -> Y, Cb, Cr as (h, w) int64."""
    p = img.astype(np.int64)
    r, g, b = (p[:, :, 0], p[:, :, 1], p[:, :, 2]) if order == 'rgb' else (p[:, :, 2], p[:, :, 1], p[:, :, 0])
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


# ---------------------------------------------------------------------------------------------------- steps 2 and 3
def _grow(p, rows, cols):
    """p with its last row and column replicated out to (rows, cols)."""
    return np.pad(p, ((0, max(rows - p.shape[0], 0)), (0, max(cols - p.shape[1], 0))), mode='edge')


def downsample(p, hx, vy):
    """Step 3 on a plane whose sides are multiples of (vy, hx)."""
    if hx == 1 and vy == 1:
        return p
    i = np.arange(p.shape[1] // 2)
    if vy == 1:
        return (p[:, 0::2] + p[:, 1::2] + (i & 1)) >> 1
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + (i & 1)) >> 2


def component_plane(p, c, L):
    """Step 2 in libjpeg's order for the full-resolution plane p of component c: the (hib * 8, wib * 8) samples of its REAL blocks."""
    H, V = ref.MODE_HV[L['mode']]
    hx, vy = (1, 1) if c == 0 else (H, V)                                # how much the component is subsampled
    wib, hib = -(-L['cw'][c] // 8), -(-L['ch'][c] // 8)
    h = p.shape[0]
    p = _grow(p, -(-h // V) * V, wib * 8 * hx)                           # columns out from w - 1; rows from h - 1 to a multiple of V
    p = downsample(p, hx, vy)
    p = _grow(p[:L['ch'][c]], hib * 8, wib * 8)                          # downsampled rows from ch - 1 up to hib * 8
    return p[:hib * 8, :wib * 8]


# ---------------------------------------------------------------------------------------------------- step 4: forward DCT
def _fpass(d, first):
    d0, d1, d2, d3, d4, d5, d6, d7 = d
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    s = 11 if first else 15
    D = lambda x: (x + (1 << (s - 1))) >> s
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o2, o6 = D(z1 + t13 * 6270), D(z1 - t12 * 15137)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    return [o0, D(t7 + z1 + z4), o2, D(t6 + z2 + z3), o4, D(t5 + z2 + z4), o6, D(t4 + z1 + z3)]


def fdct(samples):
    """(n, 8, 8) samples 0..255 -> (n, 64) coefficients (scaled by 8) in natural order."""
    d = samples.astype(np.int64) - 128                                   # [n, v, u]
    row = np.stack(_fpass([d[:, :, u] for u in range(8)], True), axis=2)  # along every row
    col = np.stack(_fpass([row[:, v, :] for v in range(8)], False), axis=1)
    return col.reshape(-1, 64)


# ---------------------------------------------------------------------------------------------------- step 5: quantiser
def quantise(c, q):
    a = (np.abs(c) + 4 * q) // (8 * q)
    return np.where(c < 0, -a, a)


# ---------------------------------------------------------------------------------------------------- the coefficient buffer
def coef_buffer(img, mode, tables, order='rgb'):
    """The whole buffer of the device stage: tables, every real block, zeros in the padding blocks.  int16[layout count]."""
    h, w = img.shape[:2]
    L = ref.layout(h, w, mode)
    buf = np.zeros(L['count'], np.int64)
    planes = colour(img, order)
    for c in range(L['ncomp']):
        q = np.asarray(tables[0 if c == 0 else 1], np.int64)
        buf[64 * c:64 * c + 64] = q
        p = component_plane(planes[c], c, L)
        hib, wib = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(hib, 8, wib, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        k = quantise(fdct(blocks), q[None, :]).reshape(hib, wib, 64)
        grid = np.zeros((L['bh'][c], L['bw'][c], 64), np.int64)
        grid[:hib, :wib] = k
        buf[L['plane'][c]:L['plane'][c] + grid.size] = grid.reshape(-1)
    return buf.astype(np.int16)


def real_block_mask(L):
    """bool[count]: True on the tables and on every coefficient of a block inside its component's real grid."""
    m = np.zeros(L['count'], bool)
    m[:64 * L['ncomp']] = True
    for c in range(L['ncomp']):
        grid = np.zeros((L['bh'][c], L['bw'][c], 64), bool)
        grid[:-(-L['ch'][c] // 8), :-(-L['cw'][c] // 8)] = True
        m[L['plane'][c]:L['plane'][c] + grid.size] = grid.reshape(-1)
    return m


# ---------------------------------------------------------------------------------------------------- step 7: entropy coding
def _codes(counts, symbols):
    """{symbol: (code, length)}"""
    return {s: (code, length) for (length, code), s in ref._huff(counts, symbols).items()}


class _Writer(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        for i in range(length - 1, -1, -1):
            self.acc = (self.acc << 1) | ((code >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc, self.n = 0, 0

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value(w, table, run, v, limit):
    s = int(abs(v)).bit_length()
    if s > limit:
        raise ref.Refused('category %d' % s)
    w.put(*table[(run << 4) | s])
    if s:
        w.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)


def headers(h, w, mode, tables, restart):
    ncomp = 1 if mode == GREY else 3
    H, V = ref.MODE_HV[mode]
    seg = lambda m, body: bytes([0xFF, m, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(2 if ncomp == 3 else 1):
        out += seg(0xDB, bytes([t]) + bytes(int(tables[t][ref.ZIGZAG[i]]) for i in range(64)))
    sof = [8, h >> 8, h & 255, w >> 8, w & 255, ncomp]
    for c in range(ncomp):
        sof += [c + 1, ((H << 4) | V) if c == 0 and ncomp == 3 else 0x11, 0 if c == 0 else 1]
    out += seg(0xC0, sof)
    for t in range(2 if ncomp == 3 else 1):
        for cls in (0, 1):
            counts, symbols = ref.STD_TABLES[(cls, t)]
            out += seg(0xC4, [(cls << 4) | t] + list(counts) + list(symbols))
    if restart:
        out += seg(0xDD, [restart >> 8, restart & 255])
    sos = [ncomp]
    for c in range(ncomp):
        sos += [c + 1, 0x00 if c == 0 else 0x11]
    return out + seg(0xDA, sos + [0, 63, 0])


def entropy_encode(buf, h, w, mode, restart=0):
    """A coefficient buffer -> the whole stream, SOI to EOI."""
    buf = np.asarray(buf).view(np.int16).astype(np.int64)
    L = ref.layout(h, w, mode)
    H, V = ref.MODE_HV[mode]
    tables = [buf[0:64] & 0xFFFF, buf[64:128] & 0xFFFF]
    dc = [_codes(*ref.STD_TABLES[(0, t)]) for t in (0, 1)]
    ac = [_codes(*ref.STD_TABLES[(1, t)]) for t in (0, 1)]
    wr = _Writer()
    wr.out += headers(h, w, mode, tables, restart)
    pred, nrst = [0, 0, 0], 0
    for mcu in range(L['mcus_x'] * L['mcus_y']):
        if restart and mcu and mcu % restart == 0:
            wr.flush()
            wr.out += bytes([0xFF, 0xD0 + (nrst & 7)])
            nrst += 1
            pred = [0, 0, 0]
        my, mx = divmod(mcu, L['mcus_x'])
        for c in range(L['ncomp']):
            hc, vc = (H, V) if c == 0 else (1, 1)
            t = 0 if c == 0 else 1
            for v in range(vc):
                for u in range(hc):
                    bx, by = mx * hc + u, my * vc + v
                    if bx >= -(-L['cw'][c] // 8) or by >= -(-L['ch'][c] // 8):         # a padding block: difference 0, EOB
                        wr.put(*dc[t][0])
                        wr.put(*ac[t][0])
                        continue
                    at = L['plane'][c] + (by * L['bw'][c] + bx) * 64
                    blk = buf[at:at + 64]
                    _value(wr, dc[t], 0, int(blk[0]) - pred[c], 11)
                    pred[c] = int(blk[0])
                    run = 0
                    for k in range(1, 64):
                        v_ = int(blk[ref.ZIGZAG[k]])
                        if v_ == 0:
                            run += 1
                            continue
                        while run > 15:
                            wr.put(*ac[t][0xF0])
                            run -= 16
                        _value(wr, ac[t], run, v_, 10)
                        run = 0
                    if run:
                        wr.put(*ac[t][0])
    wr.flush()
    return bytes(wr.out) + b'\xff\xd9'


def encode(img, mode, quality=90, restart=0, tables=None, order='rgb'):
    tables = quality_tables(quality) if tables is None else tables
    h, w = img.shape[:2]
    return entropy_encode(coef_buffer(img, mode, tables, order), h, w, mode, restart)
