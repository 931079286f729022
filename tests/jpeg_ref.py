"""numpy restatement of the header's "JPEG frames": a parser and Huffman decoder for the accepted baseline streams, the
coefficient-buffer layout, and the decode rule (dequantise, 8 x 8 inverse DCT in fixed point, chroma upsampling, YCbCr -> RGB).
The rule is libjpeg's default decode (islow, fancy upsampling, fixed-point colour tables); tests/golden/jpeg_cases.npz holds what
Pillow (libjpeg-turbo) made of the fixture streams, and tests/test_jpeg_cpu.py requires equal bytes.  Written for clarity, one
bit at a time: the library's decoder is compared against it, not modelled on it."""
import numpy as np

GREY, YUV444, YUV422, YUV420 = 0, 1, 2, 3
MODE_NAMES = {GREY: 'grey', YUV444: '444', YUV422: '422', YUV420: '420'}
MODE_HV = {GREY: (1, 1), YUV444: (1, 1), YUV422: (2, 1), YUV420: (2, 2)}      # luma sampling; chroma is 1 x 1
TABLE_WORDS = 192                                                           # three tables of 64 uint16 in front of the planes

# natural index k = 8 v + u of the i-th coefficient of the zigzag sequence
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K, tables K.3 - K.6: (the 16 code counts, the symbols in code order)
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
               [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209,
                240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
                71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
                122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
                168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
                213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248,
                249, 250])
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
                 [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82,
                  240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68,
                  69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
                  120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
                  165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
                  210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247,
                  248, 249, 250])
STD_TABLES = {(0, 0): STD_DC_LUMA, (0, 1): STD_DC_CHROMA, (1, 0): STD_AC_LUMA, (1, 1): STD_AC_CHROMA}     # (class, id)


class Refused(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------- layout
def layout(h, w, mode):
    """The coefficient buffer of a frame: dict with mcus_x, mcus_y, bw[3], bh[3] (block grids, padded to whole MCUs), cw[3], ch[3]
    (the real sample sizes), plane[3] (offsets in int16) and count (int16 of the whole buffer); grey has one plane."""
    H, V = MODE_HV[mode]
    ncomp = 1 if mode == GREY else 3
    mcus_x, mcus_y = -(-w // (8 * H)), -(-h // (8 * V))
    bw, bh, cw, ch, plane = [], [], [], [], []
    at = TABLE_WORDS
    for c in range(ncomp):
        hc, vc = (H, V) if c == 0 else (1, 1)
        bw.append(mcus_x * hc); bh.append(mcus_y * vc)
        cw.append(-(-w * hc // H)); ch.append(-(-h * vc // V))
        plane.append(at)
        at += bw[c] * bh[c] * 64
    return dict(h=h, w=w, mode=mode, ncomp=ncomp, mcus_x=mcus_x, mcus_y=mcus_y, bw=bw, bh=bh, cw=cw, ch=ch, plane=plane, count=at)


# ---------------------------------------------------------------------------------------------------- parser
def segments(data):
    """[(marker, offset of the 0xFF, total bytes of the segment with its marker)] up to and including SOS."""
    d = bytes(data)
    assert d[:2] == b'\xff\xd8'
    out, i = [(0xD8, 0, 2)], 2
    while True:
        assert d[i] == 0xFF
        j = i
        while d[j + 1] == 0xFF:
            j += 1
        m = d[j + 1]
        L = (d[j + 2] << 8) | d[j + 3]
        out.append((m, i, j + 2 + L - i))
        i = j + 2 + L
        if m == 0xDA:
            return out


def _huff(counts, symbols):
    """{(length, code): symbol}"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1; k += 1
        code <<= 1
    return table


def parse(data):
    """The headers of an accepted stream: dict with h, w, ncomp, mode, restart, q (ncomp x 64 in natural order, per component),
    dc / ac (a code table per component) and scan (offset of the entropy-coded data)."""
    d = bytes(data)
    qt, ht, frame, restart = {}, {}, None, 0
    for m, at, n in segments(d):
        j = at
        while d[j + 1] == 0xFF:
            j += 1
        body = d[j + 4:at + n]
        if m == 0xDB:
            p = 0
            while p < len(body):
                pq, tq = body[p] >> 4, body[p] & 15
                p += 1
                t = np.zeros(64, np.int64)
                for i in range(64):
                    if pq:
                        t[ZIGZAG[i]] = (body[p] << 8) | body[p + 1]; p += 2
                    else:
                        t[ZIGZAG[i]] = body[p]; p += 1
                qt[tq] = t
        elif m == 0xC4:
            p = 0
            while p < len(body):
                tc, th = body[p] >> 4, body[p] & 15
                counts = list(body[p + 1:p + 17])
                nsym = sum(counts)
                ht[(tc, th)] = _huff(counts, list(body[p + 17:p + 17 + nsym]))
                p += 17 + nsym
        elif m in (0xC0, 0xC1):
            if body[0] != 8:
                raise Refused('precision')
            h, w, nf = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            frame = (h, w, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)])
        elif m == 0xDD:
            restart = (body[0] << 8) | body[1]
        elif m == 0xDA:
            ns = body[0]
            sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            scan = at + n
        elif 0xC2 <= m <= 0xCF:
            raise Refused('coding process 0x%02X' % m)
    h, w, comps = frame
    if len(comps) == 1:
        mode = GREY
    else:
        assert len(comps) == 3 and all(c[1:3] == (1, 1) for c in comps[1:])
        mode = {(1, 1): YUV444, (2, 1): YUV422, (2, 2): YUV420}[comps[0][1:3]]
    assert [s[0] for s in sel] == [c[0] for c in comps]
    table = lambda tc, th: ht[(tc, th)] if (tc, th) in ht else _huff(*STD_TABLES[(tc, th)])
    return dict(h=h, w=w, ncomp=len(comps), mode=mode, restart=restart, q=np.stack([qt[c[3]] for c in comps]),
                dc=[table(0, s[1]) for s in sel], ac=[table(1, s[2]) for s in sel], scan=scan)


class _Bits(object):
    def __init__(self, d, pos):
        self.d, self.pos, self.acc, self.n = d, pos, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.d[self.pos]
            if b == 0xFF:
                assert self.d[self.pos + 1] == 0, 'marker inside the entropy-coded data'
                self.pos += 1
            self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise Refused('code not in table')

    def restart(self, k):
        self.n = 0
        while self.d[self.pos + 1] == 0xFF:
            self.pos += 1
        assert self.d[self.pos] == 0xFF and self.d[self.pos + 1] == 0xD0 + (k & 7), 'restart marker'
        self.pos += 2


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def entropy_decode(data):
    """(parse(data) + layout, the coefficient buffer as int16[count]): tables, then the planes Y Cb Cr, blocks in raster order of
    the padded grid, coefficients in natural order."""
    d = bytes(data)
    P = parse(d)
    L = layout(P['h'], P['w'], P['mode'])
    buf = np.zeros(L['count'], np.int64)
    for c in range(P['ncomp']):
        buf[64 * c:64 * c + 64] = P['q'][c]
    H, V = MODE_HV[P['mode']]
    rd = _Bits(d, P['scan'])
    pred = [0, 0, 0]
    n_mcu, nrst = L['mcus_x'] * L['mcus_y'], 0
    for mcu in range(n_mcu):
        if P['restart'] and mcu and mcu % P['restart'] == 0:
            rd.restart(nrst)
            nrst += 1
            pred = [0, 0, 0]
        my, mx = divmod(mcu, L['mcus_x'])
        for c in range(P['ncomp']):
            hc, vc = (H, V) if c == 0 else (1, 1)
            for v in range(vc):
                for u in range(hc):
                    at = L['plane'][c] + ((my * vc + v) * L['bw'][c] + mx * hc + u) * 64
                    s = rd.symbol(P['dc'][c])
                    pred[c] += _extend(rd.bits(s), s)
                    buf[at] = pred[c]
                    k = 1
                    while k < 64:
                        rs = rd.symbol(P['ac'][c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise Refused('run passes coefficient 63')
                        buf[at + ZIGZAG[k]] = _extend(rd.bits(s), s)
                        k += 1
    info = dict(P)
    info.update(L)
    return info, (buf & 0xFFFF).astype(np.uint16).view(np.int16)


# ---------------------------------------------------------------------------------------------------- the rule
def _w32(x):
    """int64 -> the int32 it wraps to (still int64)."""
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _pass(x, s):
    """The one-dimensional pass on x[0..7] (int64 arrays holding int32 values) with shift s.  Sums and products are formed in
    int64, where nothing overflows, and wrapped once: wrapping commutes with +, - and *."""
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    z1 = (x2 + x6) * 4433
    t2 = z1 - x6 * 15137
    t3 = z1 + x2 * 6270
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [_w32(v + (1 << (s - 1))) >> s for v in out]


def idct(coef, q):
    """coef (n, 64) int16 and q (64,) -> samples (n, 8, 8) uint8: steps 1 and 2."""
    d = _w32(coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)                 # [n, v, u]
    col = np.stack(_pass([d[:, v, :] for v in range(8)], 11), axis=1)                     # down every column
    row = np.stack(_pass([col[:, :, u] for u in range(8)], 18), axis=2)                   # along every row
    return np.clip(_w32(row + 128), 0, 255).astype(np.uint8)


def planes(buf, L):
    """The sample planes of a coefficient buffer, cut to their real sizes: [ (ch, cw) uint8 ] per component."""
    buf = np.asarray(buf).view(np.int16)
    out = []
    for c in range(L['ncomp']):
        q = buf[64 * c:64 * c + 64].view(np.uint16)
        n = L['bw'][c] * L['bh'][c]
        s = idct(buf[L['plane'][c]:L['plane'][c] + 64 * n].reshape(n, 64), q)
        p = s.reshape(L['bh'][c], L['bw'][c], 8, 8).transpose(0, 2, 1, 3).reshape(L['bh'][c] * 8, L['bw'][c] * 8)
        out.append(p[:L['ch'][c], :L['cw'][c]])
    return out


def _up_h(s, lo, hi, shift):
    """o[2i] = (3 s[i] + s[i-1] + lo) >> shift, o[2i+1] = (3 s[i] + s[i+1] + hi) >> shift, neighbours clamped."""
    e = np.pad(s, ((0, 0), (1, 1)), mode='edge')
    o = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    o[:, 0::2] = (3 * s + e[:, :-2] + lo) >> shift
    o[:, 1::2] = (3 * s + e[:, 2:] + hi) >> shift
    return o


def upsample(p, mode):
    """Step 3 for one chroma plane (ch, cw) -> (ch * V, cw * H) int64."""
    p = p.astype(np.int64)
    if mode == YUV422:
        return _up_h(p, 1, 2, 2)
    if mode == YUV420:
        e = np.pad(p, ((1, 1), (0, 0)), mode='edge')
        s = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
        s[0::2] = 3 * p + e[:-2]
        s[1::2] = 3 * p + e[2:]
        return _up_h(s, 8, 7, 4)
    return p


def colour(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode_coef(buf, h, w, mode, order='rgb'):
    """The device stage: a coefficient buffer -> the packed (h, w, 3) frame."""
    L = layout(h, w, mode)
    pl = planes(buf, L)
    y = pl[0][:h, :w]
    if mode == GREY:
        out = np.repeat(y[:, :, None], 3, axis=2)
    else:
        out = colour(y, upsample(pl[1], mode)[:h, :w], upsample(pl[2], mode)[:h, :w])
    return np.ascontiguousarray(out if order == 'rgb' else out[:, :, ::-1])


def decode(data, order='rgb'):
    info, buf = entropy_decode(data)
    return decode_coef(buf, info['h'], info['w'], info['mode'], order)
