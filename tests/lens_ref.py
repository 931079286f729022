"""numpy restatement of the lens rules of include/rtm3d_hip.h ("lens undistortion"): the bilinear remap in int64, the map
builder in float64 operation by operation (numpy evaluates each ufunc on its own, so nothing is contracted).  Written from
the header's text, not from csrc/lens.hip."""
import numpy as np

OUTSIDE = -2 ** 31
BROWN, FISHEYE = 0, 1
KIND_ID = {'brown': BROWN, 'fisheye': FISHEYE}


def remap(src, m, fill=(0, 0, 0)):
    """src (h, w, 3) uint8, m (ho, wo, 2) int32 -> (ho, wo, 3) uint8."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    m = np.asarray(m).astype(np.int64)
    sx, sy = m[..., 0], m[..., 1]
    ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31
    fill = np.asarray(fill, np.int64)

    def S(i, j):
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        v = src[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)].astype(np.int64)
        return np.where(inside[..., None], v, fill)

    wx0, wx1, wy0, wy1 = (32 - ax)[..., None], ax[..., None], (32 - ay)[..., None], ay[..., None]
    out = (wx0 * wy0 * S(ix, iy) + wx1 * wy0 * S(ix + 1, iy) + wx0 * wy1 * S(ix, iy + 1) + wx1 * wy1 * S(ix + 1, iy + 1) + 512) >> 10
    out = np.where((sx == OUTSIDE)[..., None], fill, out)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def sample_pattern(m, h, w):
    """Per map entry the 4-bit pattern of which of its four samples lie inside an h x w source (bit 0: (ix, iy), 1: (ix + 1, iy),
    2: (ix, iy + 1), 3: (ix + 1, iy + 1)); -1 for an OUTSIDE entry."""
    m = np.asarray(m).astype(np.int64)
    ix, iy = m[..., 0] >> 5, m[..., 1] >> 5
    inx = [(ix >= 0) & (ix < w), (ix + 1 >= 0) & (ix + 1 < w)]
    iny = [(iy >= 0) & (iy < h), (iy + 1 >= 0) & (iy + 1 < h)]
    p = sum(((inx[k & 1] & iny[k >> 1]).astype(np.int64) << k) for k in range(4))
    return np.where(m[..., 0] == OUTSIDE, -1, p)


def build_uv(kind, K, dist, K_rect, R, ho, wo):
    """The float64 positions (U, V) and the mask of entries that are OUTSIDE, for every destination pixel.  R: rectified ray ->
    physical ray (the header's sense)."""
    K, Kr, R = [np.asarray(a, np.float64).reshape(9) for a in (K, K_rect, R)]
    k = np.zeros(8, np.float64)
    k[:len(dist)] = np.asarray(dist, np.float64)
    v, u = np.meshgrid(np.arange(ho), np.arange(wo), indexing='ij')
    with np.errstate(all='ignore'):
        a = (u.astype(np.float64) - Kr[2]) / Kr[0]
        b = (v.astype(np.float64) - Kr[5]) / Kr[4]
        X = R[0] * a + R[1] * b + R[2]
        Y = R[3] * a + R[4] * b + R[5]
        Wz = R[6] * a + R[7] * b + R[8]
        behind = ~(Wz > 0)
        x = X / Wz
        y = Y / Wz
        if KIND_ID.get(kind, kind) == BROWN:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            r2 = x * x + y * y
            num = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            den = 1 + r2 * (k4 + r2 * (k5 + r2 * k6))
            cdist = num / den
            xd = x * cdist + ((2 * p1) * x * y + p2 * (r2 + (2 * x) * x))
            yd = y * cdist + (p1 * (r2 + (2 * y) * y) + (2 * p2) * x * y)
        else:
            k1, k2, k3, k4 = k[:4]
            r = np.sqrt(x * x + y * y)
            t = np.arctan(r)
            t2 = t * t
            td = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r > 1e-8, td / r, 1.0)
            xd = x * s
            yd = y * s
        U = K[0] * xd + K[2]
        V = K[4] * yd + K[5]
        outside = behind | ~(np.abs(U) <= 2.0 ** 20) | ~(np.abs(V) <= 2.0 ** 20)
    return U, V, outside


def build_map(kind, K, dist, K_rect, R, ho, wo):
    """(ho, wo, 2) int32."""
    U, V, outside = build_uv(kind, K, dist, K_rect, R, ho, wo)
    with np.errstate(all='ignore'):
        sx = np.floor(np.where(outside, 0.0, U) * 32.0 + 0.5)
        sy = np.floor(np.where(outside, 0.0, V) * 32.0 + 0.5)
    m = np.stack([sx, sy], -1).astype(np.int64)
    m[outside] = OUTSIDE
    return m.astype(np.int32)


def near_half(kind, K, dist, K_rect, R, ho, wo, eps=1e-6):
    """(ho, wo, 2) bool: entries whose U*32 + 0.5 (V*32 + 0.5) lies within eps of an integer - where a last-bit difference in
    atan or sqrt may move the floor."""
    U, V, outside = build_uv(kind, K, dist, K_rect, R, ho, wo)
    with np.errstate(all='ignore'):
        out = []
        for A in (U, V):
            q = np.where(outside, 0.25, A * 32.0 + 0.5)
            out.append(np.abs(q - np.rint(q)) <= eps)
    return np.stack(out, -1)
