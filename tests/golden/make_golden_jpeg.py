"""Writes tests/golden/jpeg_cases.npz: JPEG streams and what Pillow (libjpeg-turbo) decodes them to.

Run by hand where Pillow is installed (python tests/golden/make_golden_jpeg.py); no test imports this file.  The pictures are
seeded mixtures of a smooth gradient, hard-edged rectangles and noise, so that the inverse DCT overshoots 0 and 255 and the
clamps of the rule are live.  Keys of the file: 'names' (one string per case), 's_<name>' the stream as uint8, 'p_<name>' Pillow's
(h, w, 3) RGB decode (absent for the progressive stream, which exists to be refused), 'pillow' the version that wrote it."""
import io
import os
import zlib

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (37, 53), (72, 136)]            # (h, w)
MODES = ['grey', '444', '422', '420']
SUBSAMPLING = {'444': 0, '422': 1, '420': 2}
MCU = {'grey': (8, 8), '444': (8, 8), '422': (8, 16), '420': (16, 16)}                         # (rows, columns) of an MCU


def picture(h, w, grey, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = 1 if grey else 3
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = rng.uniform(0, 255, (2, c))
    img = a[0] + (a[1] - a[0]) * ((xx / max(w - 1, 1) + yy / max(h - 1, 1)) / 2)[:, :, None]
    for _ in range(1 + (h * w) // 300):                                                       # hard edges, saturated colours
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        y1, x1 = y0 + rng.integers(1, max(h // 2, 2)), x0 + rng.integers(1, max(w // 2, 2))
        img[y0:y1, x0:x1] = rng.choice([0.0, 255.0], c)
    ny, nx = rng.integers(0, h), rng.integers(0, w)                                            # a patch of noise
    img[ny:ny + max(h // 3, 1), nx:nx + max(w // 3, 1)] = rng.uniform(0, 255, img[ny:ny + max(h // 3, 1), nx:nx + max(w // 3, 1)].shape)
    img = np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8)
    return img[:, :, 0] if grey else img


def encode(img, mode, quality, **kw):
    b = io.BytesIO()
    if mode != 'grey':
        kw['subsampling'] = SUBSAMPLING[mode]
    Image.fromarray(img).save(b, 'JPEG', quality=quality, **kw)
    return b.getvalue()


def cases():
    """[(name, h, w, mode, quality, save options)]"""
    out = []
    for h, w in SIZES:                                                                        # every size x every mode
        for mode in MODES:
            out.append(('%dx%d_%s_q90' % (h, w, mode), h, w, mode, 90, {}))
    for mode in MODES:                                                                        # the other qualities
        for q in (30, 100):
            out.append(('9x17_%s_q%d' % (mode, q), 9, 17, mode, q, {}))
    out.append(('37x53_420_q100', 37, 53, '420', 100, {}))
    for mode in MODES:                                                                        # optimised Huffman tables
        out.append(('17x33_%s_q30_opt' % mode, 17, 33, mode, 30, {'optimize': True}))
    for mode in MODES:                                                                        # restart intervals 1, 2, one MCU row (RST7 -> RST0 wraps)
        out.append(('37x53_%s_q90_r1' % mode, 37, 53, mode, 90, {'restart_marker_blocks': 1}))
        for ri, tag in ((2, 'r2'), (-(-33 // MCU[mode][1]), 'rrow')):
            out.append(('17x33_%s_q90_%s' % (mode, tag), 17, 33, mode, 90, {'restart_marker_blocks': ri}))
    out.append(('40x33_420_q30_opt_r2', 40, 33, '420', 30, {'optimize': True, 'restart_marker_blocks': 2}))
    return out


def main():
    arrays, names = {}, []
    for name, h, w, mode, q, kw in cases():
        img = picture(h, w, mode == 'grey', zlib.crc32(name.encode()))
        s = encode(img, mode, q, **kw)
        pix = np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))
        assert pix.shape == (h, w, 3)
        names.append(name)
        arrays['s_' + name] = np.frombuffer(s, np.uint8)
        arrays['p_' + name] = pix
    s = encode(picture(16, 16, False, 1), '420', 90, progressive=True)                        # to be refused
    names.append('16x16_420_progressive')
    arrays['s_16x16_420_progressive'] = np.frombuffer(s, np.uint8)
    path = os.path.join(HERE, 'jpeg_cases.npz')
    np.savez_compressed(path, names=np.array(names), pillow=np.array(PIL.__version__), **arrays)
    print('%d cases, %d stream bytes, file %d bytes' % (len(names), sum(len(arrays['s_' + n]) for n in names), os.path.getsize(path)))


if __name__ == '__main__':
    main()
