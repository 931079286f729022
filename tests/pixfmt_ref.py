"""numpy restatement of the pixel-format rule of include/rtm3d_hip.h ("pixel formats"), written from the header's text.  The
coefficient tables are derived here from (Kr, Kb) in float64 - the library carries them as integer literals.

A source is a dict: {'format': name, 'h', 'w', 'planes': [1-D uint8 arrays: the raw bytes of each plane], 'pitches': [bytes
from row to row], 'matrix': 'bt601' | 'bt709', 'range': 'limited' | 'full'}."""
import numpy as np

FORMATS = ['rgb24', 'bgr24', 'rgba32', 'bgra32', 'gray8', 'nv12', 'nv21', 'i420', 'yuyv', 'uyvy', 'p010']
FORMAT_ID = {n: i for i, n in enumerate(FORMATS)}
YUV = ('nv12', 'nv21', 'i420', 'yuyv', 'uyvy', 'p010')
KR_KB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}


def layout(fmt, h, w):
    """[(row bytes, rows)] per plane."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return {'rgb24': [(3 * w, h)], 'bgr24': [(3 * w, h)], 'rgba32': [(4 * w, h)], 'bgra32': [(4 * w, h)], 'gray8': [(w, h)],
            'nv12': [(w, h), (2 * cw, ch)], 'nv21': [(w, h), (2 * cw, ch)], 'i420': [(w, h), (cw, ch), (cw, ch)],
            'yuyv': [(4 * cw, h)], 'uyvy': [(4 * cw, h)], 'p010': [(2 * w, h), (4 * cw, ch)]}[fmt]


def real_matrix(matrix, rng, bits):
    """The textbook float64 coefficients (cy, crv, cgu, cgv, cbu) on integer samples, and (yo, chroma offset)."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    if bits == 8:
        sy, sc, yo, co = (255.0 / 219.0, 255.0 / 224.0, 16, 128) if rng == 'limited' else (1.0, 1.0, 0, 128)
    else:
        sy, sc, yo, co = (255.0 / 876.0, 255.0 / 896.0, 64, 512) if rng == 'limited' else (255.0 / 1023.0, 255.0 / 1023.0, 0, 512)
    v = (sy, 2.0 * (1.0 - kr) * sc, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc, 2.0 * (1.0 - kb) * sc)
    return v, yo, co


def table(matrix, rng, bits):
    """([cy, crv, cgu, cgv, cbu] = round(2^S * v), yo, chroma offset, S)."""
    S = 16 if bits == 8 else 18
    v, yo, co = real_matrix(matrix, rng, bits)
    return [int(np.rint(np.float64(2 ** S) * x)) for x in v], yo, co, S


def yuv_to_rgb(Y, Cb, Cr, matrix, rng, bits=8):
    """The rule on int arrays of equal shape -> uint8 (..., 3) R G B.  int32 throughout, >> arithmetic."""
    (cy, crv, cgu, cgv, cbu), yo, co, S = table(matrix, rng, bits)
    Y = np.asarray(Y, np.int32) - np.int32(yo)
    U, V = np.asarray(Cb, np.int32) - np.int32(co), np.asarray(Cr, np.int32) - np.int32(co)
    half = np.int32(1 << (S - 1))
    l = np.int32(cy) * Y
    r = (l + np.int32(crv) * V + half) >> S
    g = (l + np.int32(cgu) * U + np.int32(cgv) * V + half) >> S
    b = (l + np.int32(cbu) * U + half) >> S
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def yuv_to_rgb_real(Y, Cb, Cr, matrix, rng, bits=8):
    """The float64 matrix with round-half-up and clamp: what the integer rule approximates."""
    (cy, crv, cgu, cgv, cbu), yo, co = real_matrix(matrix, rng, bits)
    Y, U, V = np.asarray(Y, np.float64) - yo, np.asarray(Cb, np.float64) - co, np.asarray(Cr, np.float64) - co
    rgb = np.stack([cy * Y + crv * V, cy * Y + cgu * U + cgv * V, cy * Y + cbu * U], -1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def _rows(buf, pitch, row_bytes, rows):
    """(rows, row_bytes) uint8: the rows' own bytes of a pitched plane (nothing behind the last row's bytes is touched)."""
    out = np.empty((rows, row_bytes), np.uint8)
    for y in range(rows):
        out[y] = buf[y * pitch:y * pitch + row_bytes]
    return out


def convert(src, order='rgb'):
    """One source -> (h, w, 3) uint8, pixels written R G B (order 'rgb') or B G R ('bgr')."""
    fmt, h, w = src['format'], src['h'], src['w']
    lay = layout(fmt, h, w)
    P = [_rows(np.asarray(b, np.uint8), p, rb, r) for b, p, (rb, r) in zip(src['planes'], src['pitches'], lay)]
    cw = (w + 1) // 2
    xs, ys = np.arange(w), np.arange(h)
    if fmt in ('rgb24', 'bgr24', 'rgba32', 'bgra32'):
        c = 3 if fmt.endswith('24') else 4
        rgb = P[0].reshape(h, w, c)[:, :, :3]
        if fmt.startswith('bgr'):
            rgb = rgb[:, :, ::-1]
    elif fmt == 'gray8':
        rgb = np.repeat(P[0][:, :, None], 3, 2)
    else:
        m, r = src.get('matrix', 'bt601'), src.get('range', 'limited')
        if fmt in ('nv12', 'nv21', 'i420', 'p010'):
            if fmt == 'p010':
                Yp = P[0].reshape(h, w, 2).astype(np.int32)
                Y = (Yp[..., 0] | (Yp[..., 1] << 8)) >> 6
                Cp = P[1].reshape(-1, cw, 2, 2).astype(np.int32)
                C = (Cp[..., 0] | (Cp[..., 1] << 8)) >> 6                      # (ch, cw, 2): Cb Cr
                cb, cr = C[..., 0], C[..., 1]
            else:
                Y = P[0].astype(np.int32)
                if fmt == 'i420':
                    cb, cr = P[1].astype(np.int32), P[2].astype(np.int32)
                else:
                    C = P[1].reshape(-1, cw, 2).astype(np.int32)
                    cb, cr = (C[..., 0], C[..., 1]) if fmt == 'nv12' else (C[..., 1], C[..., 0])
            Cb, Cr = cb[(ys >> 1)[:, None], (xs >> 1)[None, :]], cr[(ys >> 1)[:, None], (xs >> 1)[None, :]]
        else:                                                               # yuyv / uyvy: pairs of four bytes
            Q = P[0].reshape(h, cw, 4).astype(np.int32)
            y0, u, y1, v = (0, 1, 2, 3) if fmt == 'yuyv' else (1, 0, 3, 2)
            Y = np.stack([Q[..., y0], Q[..., y1]], -1).reshape(h, 2 * cw)[:, :w]
            Cb, Cr = Q[..., u][:, xs >> 1], Q[..., v][:, xs >> 1]
        rgb = yuv_to_rgb(Y, Cb, Cr, m, r, 10 if fmt == 'p010' else 8)
    rgb = np.ascontiguousarray(rgb)
    return np.ascontiguousarray(rgb[:, :, ::-1]) if order == 'bgr' else rgb
