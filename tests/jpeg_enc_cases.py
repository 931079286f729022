"""Case tables of the JPEG encoding tests (tests/test_jpeg_enc_cpu.py, tests/test_gpu_jpeg_enc.py): the fixture pictures of
tests/golden/jpeg_encode_cases.npz with the streams Pillow (libjpeg-turbo) wrote for them, the reference's coefficient buffers
(computed once), the size lists of the device stage, the regime table of the launch plan and the refusal tables."""
import os

import numpy as np

from tests import jpeg_enc_ref as enc
from tests import jpeg_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_encode_cases.npz')
OLD_GOLDEN = os.path.join(HERE, 'golden', 'jpeg_cases.npz')
MODES = [ref.GREY, ref.YUV444, ref.YUV422, ref.YUV420]

_cache = {}


def _file():
    if 'g' not in _cache:
        _cache['g'] = np.load(GOLDEN, allow_pickle=False)
    return _cache['g']


def names():
    return [str(n) for n in _file()['names']]


def case(name):
    """(picture (h, w, 3) uint8 - a grey one as R = G = B -, h, w, mode, quality, restart interval, Pillow's stream as bytes)"""
    if ('case', name) not in _cache:
        g = _file()
        p = name.split('_')
        h, w = [int(v) for v in p[0].split('x')]
        img = g['img_%dx%d_%s' % (h, w, 'g' if p[1] == 'grey' else 'c')]
        if img.ndim == 2:
            img = np.repeat(img[:, :, None], 3, axis=2)
        img = np.ascontiguousarray(img)
        img.setflags(write=False)
        _cache[('case', name)] = (img, h, w, enc.MODES[p[1]], int(p[2][1:]), int(p[3][1:]) if len(p) > 3 else 0, g['s_' + name].tobytes())
    return _cache[('case', name)]


def reference(name):
    """The reference's coefficient buffer of a fixture, computed once."""
    if ('ref', name) not in _cache:
        img, h, w, mode, q, ri, _ = case(name)
        buf = enc.coef_buffer(img, mode, enc.quality_tables(q))
        buf.setflags(write=False)
        _cache[('ref', name)] = buf
    return _cache[('ref', name)]


def picture(h, w, seed):
    """A picture of the fixture's kind - gradient, saturated rectangles, noise - of any size, for the device tests."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = rng.uniform(0, 255, (2, 3))
    img = a[0] + (a[1] - a[0]) * ((xx / max(w - 1, 1) + yy / max(h - 1, 1)) / 2)[:, :, None]
    for _ in range(1 + min((h * w) // 300, 40)):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        img[y0:y0 + rng.integers(1, max(h // 2, 2)), x0:x0 + rng.integers(1, max(w // 2, 2))] = rng.choice([0.0, 255.0], 3)
    ny, nx = rng.integers(0, h), rng.integers(0, w)
    patch = img[ny:ny + max(h // 3, 1), nx:nx + max(w // 3, 1)]
    patch[...] = rng.uniform(0, 255, patch.shape)
    return np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- the plan
# what the header promises: tiles of 128 x 64 pixels, 256 threads, LDS rows of 144 / 72 bytes, 32 frames per chunk
TILE_W, TILE_H, THREADS, LDS_STRIDE, LDS_STRIDE_SUB, CHUNK = 128, 64, 256, 144, 72, 32
SMALL_SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (37, 53), (20, 40), (72, 136)]


def edge_sizes(tw=TILE_W, th=TILE_H):
    """Sizes on either side of every tile boundary, and two tiles + 1."""
    return [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (th - 1, tw + 1), (th + 1, tw - 1), (2 * th + 1, 2 * tw + 1)]


def plan_regimes():
    """[(sizes (h, w) of a batch, the expected (first, count, tiles, grid_x, grid_y) per chunk)]"""
    return [
        ([(1, 1)], [(0, 1, 1, 1, 1)]),
        ([(TILE_H, TILE_W)], [(0, 1, 1, 1, 1)]),
        ([(TILE_H + 1, TILE_W)], [(0, 1, 2, 2, 1)]),
        ([(TILE_H, TILE_W + 1)], [(0, 1, 2, 2, 1)]),
        ([(384, 1280)], [(0, 1, 60, 60, 1)]),
        ([(8, 8), (384, 1280), (65, 129)], [(0, 3, 60, 60, 3)]),
        ([(16384, 16384)], [(0, 1, 128 * 256, 128 * 256, 1)]),
        ([(9, 17)] * 32 + [(65, 17)], [(0, 32, 1, 1, 32), (32, 1, 2, 2, 1)]),
        ([(9, 17)] * 65, [(0, 32, 1, 1, 32), (32, 32, 1, 1, 32), (64, 1, 1, 1, 1)]),
    ]


# ---------------------------------------------------------------------------------------------------- refusals
def entropy_refusals():
    """[(name, coefficient buffer, h, w, mode, restart, capacity or None for the bound, a word of the message)] for
    rtm3d_jpeg_entropy_encode; the buffer is the reference's of 9x17 4:2:0 with one thing wrong."""
    good = np.array(reference('9x17_420_q90'))
    L = ref.layout(9, 17, ref.YUV420)

    def with_(at, v):
        b = good.copy()
        b[at] = v
        return b

    big_dc = good.copy()
    big_dc[L['plane'][0]] = 1024
    big_dc[L['plane'][0] + 64] = -1024                                   # a difference of -2048: category 12
    return [
        ('unknown mode', good, 9, 17, 4, 0, None, 'unknown mode 4'),
        ('negative mode', good, 9, 17, -1, 0, None, 'unknown mode -1'),
        ('h of 0', good, 0, 17, 3, 0, None, 'a frame of 0 x 17'),
        ('w above 16384', good, 9, 16385, 3, 0, None, 'a frame of 9 x 16385'),
        ('restart above 65535', good, 9, 17, 3, 65536, None, 'restart interval of 65536'),
        ('negative restart', good, 9, 17, 3, -1, None, 'restart interval of -1'),
        ('luma table entry 0', with_(5, 0), 9, 17, 3, 0, None, 'entry 5 of quantisation table 0 is 0'),
        ('chroma table entry 256', with_(64 + 63, 256), 9, 17, 3, 0, None, 'entry 63 of quantisation table 1 is 256'),
        ('DC difference of category 12', big_dc, 9, 17, 3, 0, None, 'category 12'),
        ('AC of category 11', with_(L['plane'][1] + 9, -1024), 9, 17, 3, 0, None, 'an AC coefficient of -1024'),
        ('capacity below the bound', good, 9, 17, 3, 0, -1, 'may need'),
    ]


def fdct_refusals():
    """[(frame (src, coef, h, w, mode) with one thing wrong, a word of the message)] for rtm3d_frames_jpeg_fdct_check; frame 1 of 2."""
    return [
        ((0x1000, 0x2000, 0, 8, 0), 'frame 1 is 0 x 8'), ((0x1000, 0x2000, 8, 16385, 0), 'frame 1 is 8 x 16385'),
        ((0x1000, 0x2000, 8, 8, 4), 'frame 1 has the unknown mode 4'), ((0x1000, 0x2000, 8, 8, -1), 'unknown mode'),
        ((0, 0x2000, 8, 8, 0), 'frame 1: the source is a NULL'), ((0x1000, 0, 8, 8, 0), 'frame 1: the coefficient buffer is a NULL'),
        ((0x1001, 0x2008, 8, 8, 0), 'frame 1: the coefficient buffer is not 16-byte aligned'),
    ]
