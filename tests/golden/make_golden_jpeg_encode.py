"""Writes tests/golden/jpeg_encode_cases.npz: pictures and the streams Pillow (libjpeg-turbo) encodes them to, Huffman tables not
optimised.

Run by hand where Pillow is installed (python tests/golden/make_golden_jpeg_encode.py); no test imports this file.  The pictures
follow make_golden_jpeg.picture (gradient, saturated rectangles, a patch of noise), one colour and one grey picture per size,
shared by the cases of that size; a grey picture is stored as (h, w) and is encoded by the library as R = G = B.  Keys of the
file: 'names' (one string per case: <h>x<w>_<mode>_q<quality>[_r<interval in MCUs>]), 's_<name>' the stream as uint8,
'img_<h>x<w>_c' / 'img_<h>x<w>_g' the pictures, 'pillow' the version that wrote it."""
import io
import os
import zlib

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (37, 53), (20, 40), (72, 136)]   # (h, w); (20, 40) in 4:2:0 has padding blocks right and below
MODES = ['grey', '444', '422', '420']
SUBSAMPLING = {'444': 0, '422': 1, '420': 2}
MCU_W = {'grey': 8, '444': 8, '422': 16, '420': 16}


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


def cases():
    """[(name, h, w, mode, quality, restart interval in MCUs)]"""
    out = []
    for h, w in SIZES:
        for mode in MODES:
            out.append(('%dx%d_%s_q90' % (h, w, mode), h, w, mode, 90, 0))
    for h, w in ((9, 17), (37, 53)):
        for mode in MODES:
            for q in (1, 30, 75, 100):
                out.append(('%dx%d_%s_q%d' % (h, w, mode, q), h, w, mode, q, 0))
    for h, w in ((37, 53), (17, 33)):
        for mode in MODES:
            for ri in (1, 2, -(-w // MCU_W[mode])):
                out.append(('%dx%d_%s_q90_r%d' % (h, w, mode, ri), h, w, mode, 90, ri))
    return out


def main():
    arrays, names = {}, []
    for name, h, w, mode, q, ri in cases():
        key = 'img_%dx%d_%s' % (h, w, 'g' if mode == 'grey' else 'c')
        if key not in arrays:
            arrays[key] = picture(h, w, mode == 'grey', zlib.crc32(key.encode()))
        kw = {} if mode == 'grey' else {'subsampling': SUBSAMPLING[mode]}
        if ri:
            kw['restart_marker_blocks'] = ri
        b = io.BytesIO()
        Image.fromarray(arrays[key]).save(b, 'JPEG', quality=q, optimize=False, **kw)
        names.append(name)
        arrays['s_' + name] = np.frombuffer(b.getvalue(), np.uint8)
    path = os.path.join(HERE, 'jpeg_encode_cases.npz')
    np.savez_compressed(path, names=np.array(names), pillow=np.array(PIL.__version__), **arrays)
    print('%d cases, %d stream bytes, file %d bytes' % (len(names), sum(len(arrays['s_' + n]) for n in names), os.path.getsize(path)))


if __name__ == '__main__':
    main()
