"""The case table of the lens tests: destination sizes on either side of every boundary of the remap's thread mapping, source
sizes, seeded map makers and the lens models of the builder tests.

The thread mapping the sizes are chosen against (rtm3d_frames_remap_plan; tests/test_lens_cpu.py pins these numbers): a thread
takes PX = 4 consecutive pixels of one destination row, a workgroup T = 256 such runs in row-major order of the frame's runs
(SPAN = 1024 pixels of a long row), a launch 32 frames.  The largest shapes are a 37 x 53 source and a 48 x 64 destination."""
import numpy as np

from tests import lens_ref as ref

PX, T, CHUNK = 4, 256, 32
SPAN = PX * T
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

# the issue's list, and the largest destination
DST_SMALL = [(1, 1), (1, 7), (2, 9), (33, 65), (48, 64)]
# widths one below, at and above one run and two runs
DST_RUN_EDGES = [(3, PX - 1), (3, PX), (3, PX + 1), (2, 2 * PX - 1), (2, 2 * PX), (2, 2 * PX + 1)]
# widths one below, at and above the workgroup's span of one row
DST_SPAN_EDGES = [(1, SPAN - 1), (2, SPAN), (1, SPAN + 1)]
# 255, 256, 257 runs as rows of one run each (whole and partial runs)
DST_BLOCK_EDGES = [(T - 1, PX), (T, PX - 1), (T + 1, PX)]
DST_SIZES = DST_SMALL + DST_RUN_EDGES + DST_SPAN_EDGES + DST_BLOCK_EDGES
SRC_SIZES = [(37, 53), (1, 1), (2, 3), (5, 4)]

MAP_KINDS = ('random', 'outside', 'special', 'fractions')


def expected_runs(ho, wo):
    return ((wo + PX - 1) // PX) * ho


def special_values(n):
    """The issue's values for a coordinate of a source side n."""
    return [INT32_MAX, INT32_MIN + 1, -1, -32, -33, 32 * n - 1, 32 * n, 32 * (n - 1)]


def make_map(kind, h, w, ho, wo, rng):
    """(ho, wo, 2) int32 for an h x w source."""
    n = ho * wo
    if kind == 'random':        # every border combination of the four samples
        m = np.stack([rng.integers(-3 * 32, (w + 3) * 32, n), rng.integers(-3 * 32, (h + 3) * 32, n)], -1)
    elif kind == 'outside':
        m = np.stack([np.full(n, INT32_MIN), rng.integers(INT32_MIN, INT32_MAX, n, endpoint=True)], -1)
    elif kind == 'special':     # every pair of (a special or an ordinary sx) x (a special or an ordinary sy), cycled
        xs = special_values(w) + [int(v) for v in rng.integers(0, 32 * w, 3)]
        ys = special_values(h) + [INT32_MIN] + [int(v) for v in rng.integers(0, 32 * h, 3)]      # sy == INT32_MIN is an ordinary value
        pairs = np.array([(x, y) for x in xs for y in ys], np.int64)
        m = pairs[(np.arange(n) + int(rng.integers(0, len(pairs)))) % len(pairs)]
    elif kind == 'fractions':   # every (ax, ay), around integer positions from one left of / above the frame to its last pixel
        f = (np.arange(n) + int(rng.integers(0, 1024))) % 1024
        m = np.stack([32 * rng.integers(-1, w, n) + (f & 31), 32 * rng.integers(-1, h, n) + (f >> 5)], -1)
    else:
        raise ValueError(kind)
    return m.reshape(ho, wo, 2).astype(np.int32)


def frames_for(h, w, rng):
    """random bytes, all 0, all 255"""
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)]


def axis_states(m, h, w):
    """The set of (x state, y state) pairs of a map's entries: a state is (first sample inside, second sample inside) along
    one axis - 4 x 4 = 16 combinations."""
    m = np.asarray(m).astype(np.int64).reshape(-1, 2)
    m = m[m[:, 0] != INT32_MIN]
    ix, iy = m[:, 0] >> 5, m[:, 1] >> 5
    sx = ((ix >= 0) & (ix < w)).astype(int) + 2 * ((ix + 1 >= 0) & (ix + 1 < w)).astype(int)
    sy = ((iy >= 0) & (iy < h)).astype(int) + 2 * ((iy + 1 >= 0) & (iy + 1 < h)).astype(int)
    return set(zip(sx.tolist(), sy.tolist()))


# ---------------------------------------------------------------------------------------------------- the builder
LENS_SIZE, MAP_SIZE = (40, 56), (48, 64)
K_LENS = [41.5, 0, 27.25, 0, 43.0, 19.5, 0, 0, 1]
K_WIDE = [12.0, 0, 30.5, 0, 13.5, 25.25, 0, 0, 1]          # a short rectified focal length: rays far off the axis
EYE = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def rot(ax_deg, ay_deg, az_deg):
    """Rz Ry Rx, row-major 9 (rectified ray -> physical ray)."""
    a, b, c = np.deg2rad([ax_deg, ay_deg, az_deg])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).reshape(9).tolist()


# (name, kind, K, dist, K_rect, R, (ho, wo))
BROWN_CASES = [
    ('none', 'brown', K_LENS, [0] * 8, K_LENS, EYE, LENS_SIZE),
    ('k1', 'brown', K_LENS, [-0.21, 0, 0, 0, 0, 0, 0, 0], K_LENS, EYE, MAP_SIZE),
    ('five', 'brown', K_LENS, [-0.28, 0.07, 1.5e-3, -2.5e-3, -0.011], K_LENS, EYE, MAP_SIZE),
    ('rational', 'brown', K_LENS, [0.31, -0.12, 4e-4, 9e-4, 0.013, 0.52, -0.09, 0.004], [38.0, 0, 31.5, 0, 39.0, 23.5, 0, 0, 1], rot(2, -3, 1.5), MAP_SIZE),
    # a tilted rectified camera with a short focal length: some rays have Wz <= 0, some positions pass 2^20
    ('tilted', 'brown', K_LENS, [-0.28, 0.07, 1.5e-3, -2.5e-3, -0.011], K_WIDE, rot(8, 60, -4), MAP_SIZE),
]
FISHEYE_CASES = [
    ('equidistant', 'fisheye', K_LENS, [0, 0, 0, 0], K_LENS, EYE, MAP_SIZE),
    ('kb4', 'fisheye', K_LENS, [-0.035, 0.011, -0.004, 0.0007], [20.0, 0, 31.5, 0, 21.0, 23.5, 0, 0, 1], EYE, MAP_SIZE),
    ('kb4_tilted', 'fisheye', K_LENS, [0.08, -0.02, 0.003, -0.0004], K_WIDE, rot(8, 60, -4), MAP_SIZE),
]


def reference_map(case):
    _, kind, K, dist, Kr, R, (ho, wo) = case
    return ref.build_map(kind, K, dist, Kr, R, ho, wo)
