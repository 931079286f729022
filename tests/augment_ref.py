"""numpy restatement of the rules of include/rtm3d_hip.h ("training augmentation"): Philox4x32-10, the noise table, the fp64
geometry of rtm3d_augment_geometry and the integer pixel rule of rtm3d_frames_augment (int64 throughout).  Written from the
header's text, not from csrc/augment.hip."""
import statistics

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
ONE = 32 * 65536                          # a source pixel in the units of ax / bx


def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two 32-bit words -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def noise_table():
    """T[k] = round(1024 * Phi^-1((k + 0.5) / 4096)), 4096 int16."""
    nd = statistics.NormalDist()
    return np.array([round(1024 * nd.inv_cdf((k + 0.5) / 4096)) for k in range(4096)], np.int16)


def quantise(alpha=1.0, beta=0.0, sigma=0.0):
    """What the facade hands the library: (alpha_q, beta_q, sigma_q)."""
    return int(round(alpha * 65536)), int(round(beta * 255 * 65536)), int(round(sigma * 64))


def geometry(h, w, rh, rw, scale=1.0, off_x=0.0, off_y=0.0, flip=0):
    """(ax, bx, ay, by) of rtm3d_augment_geometry: fp64, the header's operation order."""
    def axis(n_src, n_rect, off, mirror):
        r = np.float64(n_src) / np.float64(n_rect)
        g = r / np.float64(scale)
        m0 = np.float64(n_rect - 1) if mirror else np.float64(0.0)
        c = ((m0 - np.float64(off)) / np.float64(scale) + 0.5) * r - 0.5
        a = -g if mirror else g
        return int(np.floor(a * np.float64(ONE) + 0.5)), int(np.floor(c * np.float64(ONE) + 0.5)) + 32768
    ax, bx = axis(w, rw, off_x, bool(flip))
    ay, by = axis(h, rh, off_y, False)
    return ax, bx, ay, by


def photometric(src, alpha_q=65536, beta_q=0, sigma_q=0, seed=0, table=None):
    """The values `a` of every source byte: brightness / contrast, then noise.  src (h, w, 3) uint8 -> (h, w, 3) int64."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    L = np.clip((src.astype(np.int64) * int(alpha_q) + int(beta_q)) >> 16, 0, 255)
    if sigma_q == 0:
        return L
    T = (noise_table() if table is None else np.asarray(table)).astype(np.int64)
    p = (np.arange(h, dtype=np.int64)[:, None] * w + np.arange(w, dtype=np.int64)[None, :])
    r = philox4x32_10((p, 0, 0, 0), (int(seed) & MASK, (int(seed) >> 32) & MASK))
    n = np.stack([(T[(r[c] >> np.uint64(20)).astype(np.int64)] * int(sigma_q) + 32768) >> 16 for c in range(3)], -1)
    return np.clip(L + n, 0, 255)


def noise_values(h, w, sigma_q, seed, table=None):
    """The (h, w, 3) int64 noise n of a frame, before it is added."""
    T = (noise_table() if table is None else np.asarray(table)).astype(np.int64)
    p = (np.arange(h, dtype=np.int64)[:, None] * w + np.arange(w, dtype=np.int64)[None, :])
    r = philox4x32_10((p, 0, 0, 0), (int(seed) & MASK, (int(seed) >> 32) & MASK))
    return np.stack([(T[(r[c] >> np.uint64(20)).astype(np.int64)] * int(sigma_q) + 32768) >> 16 for c in range(3)], -1)


def rectangle(src, rw, rh, coef, alpha_q=65536, beta_q=0, sigma_q=0, seed=0, fill=(0, 0, 0), table=None):
    """The rh x rw x 3 bytes of the placed rectangle."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    ax, bx, ay, by = [int(v) for v in coef]
    a = photometric(src, alpha_q, beta_q, sigma_q, seed, table)
    # python ints: x * ax may pass 2^63 only beyond the checked range, but object arithmetic costs nothing at these sizes
    sx = np.array([(x * ax + bx) >> 16 for x in range(rw)], np.int64)[None, :]
    sy = np.array([(y * ay + by) >> 16 for y in range(rh)], np.int64)[:, None]
    out_of = (sx <= -32) | (sx >= 32 * w) | (sy <= -32) | (sy >= 32 * h)
    sx = np.clip(sx, 0, 32 * (w - 1)) + 0 * sy
    sy = np.clip(sy, 0, 32 * (h - 1)) + 0 * sx
    ix, fx, iy, fy = sx >> 5, sx & 31, sy >> 5, sy & 31
    fill = np.asarray(fill, np.int64)

    def S(i, j):
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        v = a[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)]
        return np.where(inside[..., None], v, fill)

    wx0, wx1, wy0, wy1 = (32 - fx)[..., None], fx[..., None], (32 - fy)[..., None], fy[..., None]
    out = (wx0 * wy0 * S(ix, iy) + wx1 * wy0 * S(ix + 1, iy) + wx0 * wy1 * S(ix, iy + 1) + wx1 * wy1 * S(ix + 1, iy + 1) + 512) >> 10
    out = np.where(out_of[..., None], fill, out)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def canvas(src, H, W, x0, y0, rw, rh, coef, **kw):
    """The H x W x 3 uint8 canvas of one frame: the rectangle, the rest in its truncated mean colour."""
    rect = rectangle(src, rw, rh, coef, **kw)
    pad = rect.reshape(-1, 3).astype(np.int64).sum(axis=0) // (rw * rh)
    out = np.empty((H, W, 3), np.uint8)
    out[:] = pad.astype(np.uint8)
    out[y0:y0 + rh, x0:x0 + rw] = rect
    return out


def normalise32(canvas_u8, lut32):
    """mode 0: (3, H, W) float32 through the (3, 256) table."""
    return np.stack([np.asarray(lut32)[c][canvas_u8[..., c]] for c in range(3)], 0)


def normalise16(canvas_u8, lut16, border=0):
    """mode 1: (H + 2P, W + 2P, 4) uint16 bit patterns (the border rows / columns are returned as 0 and not compared)."""
    H, W = canvas_u8.shape[:2]
    out = np.zeros((H + 2 * border, W + 2 * border, 4), np.uint16)
    for c in range(3):
        out[border:border + H, border:border + W, c] = np.asarray(lut16)[c][canvas_u8[..., c]]
    return out
