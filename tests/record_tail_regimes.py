"""The named cases of the record tail - rtm3d_pack_records, rtm3d_project_boxes (csrc/decode3d.hip), rtm3d_frames_adjust_k,
rtm3d_records_to_camera (csrc/frames.hip) and csrc/box_project.h under both - one per regime of their thread mappings and
branches, seeded and tiny, with the conditions a case must meet as functions.  tests/test_record_tail_regimes.py asserts those
conditions on the yardstick (tests/record_tail_ref.py) alone; tests/test_gpu_record_tail_regimes.py runs the device on the same
tables.  Solver outputs (x, fun, status) are made by hand: nothing here runs the solver or a network.

Thread mappings the sizes come from: pack_records one thread per float, 256 per block, slot = t >> 5 (8 slots per block);
project_boxes 9 threads per slot (slot 7 = threads 63..71 straddles the first wave boundary, slot 28 = threads 252..260 the first
block boundary); frames_adjust_K nb * 9 threads in chunks of 64 frames (29 frames = 261 threads, two blocks); records_to_camera
32 lanes per slot, two slots per wave, chunks of 64 frames."""
import functools
import math

import numpy as np

from tests import record_tail_ref as ref

FUN_ACCEPT = 0.1                      # model_utils.FUN_ACCEPT, what the Python wrappers pass
CANVAS = (128, 256)
K_PLAIN = [721.5377, 0.0, 609.5593, 0.0, 721.5377, 172.854, 0.0, 0.0, 1.0]
K_SKEW = [700.0, 1.5, 600.0, 0.3, 710.0, 170.0, 1e-3, -2e-3, 1.01]        # skew entries, third row other than (0, 0, 1)
K_CX0 = [721.5377, 0.0, 0.0, 0.0, 721.5377, 172.854, 0.0, 0.0, 1.0]       # cx = 0: pu = 0 for a point on the optical axis plane
KS = [K_PLAIN, K_SKEW, K_CX0]

# (h, w, rh, rw, pad_w, pad_h) on the 128 x 256 canvas: the five of RAGGED in tests/test_gpu_frames.py (identity, width-limited
# Resize, padding on both axes, odd differences, height-limited Resize), a 1 x 1 frame, an 8192-wide frame resized down
GEOMS = [(128, 256, 128, 256, 0, 0), (300, 1000, 76, 256, 0, 26), (100, 201, 100, 201, 27, 14), (101, 223, 101, 223, 16, 13),
         (500, 300, 128, 76, 90, 0), (1, 1, 1, 1, 127, 63), (2048, 8192, 64, 256, 0, 32)]
GEOM_SPECS = [(128, 256, None), (300, 1000, 256), (100, 201, None), (101, 223, None), (500, 300, 128), (1, 1, None), (2048, 8192, 256)]


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def random_boxes(g, n):
    """Plausible solver iterates x = [sin, cos, l, h, w, X, Y, Z] with a non-unit (x0, x1), in front of the camera."""
    ang, r = g.uniform(-math.pi, math.pi, n), g.uniform(0.5, 1.5, n)
    return np.stack([r * np.sin(ang), r * np.cos(ang), g.uniform(3, 5, n), g.uniform(1.2, 2, n), g.uniform(1.4, 2, n),
                     g.uniform(-8, 8, n), g.uniform(0.5, 2, n), g.uniform(8, 60, n)], 1)


# ------------------------------------------------------------------------------------------------ 1. pack_records
PACK_SHAPES = [(1, 1, [1]), (1, 1, [0]), (1, 1, [-2]), (1, 1, [6]), (1, 7, [12]), (1, 7, [7]), (1, 8, [8]), (1, 8, [0]),
               (3, 3, [0, 3, 8]), (3, 3, [-2, 3, 3]), (5, 13, [-2, 13, 0, 18, 6])]
PACK_NAMES = ['b%dk%d_n%s' % (B, k, '_'.join(str(v) for v in n)) for B, k, n in PACK_SHAPES]
YAW_PAIRS = [(0.0, -1.0), (-0.0, -1.0), (0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (3.0, 4.0)]
EDGE_ACCEPTS = [0.1, 0.25, math.inf, math.nan]
# (status, fun): 'below' = the double below fun_accept, 'equal' = fun_accept itself; slots alternate kept / not kept
EDGE_SLOTS = [(0, 'below'), (0, 'equal'), (3, '-inf'), (0, 'nan'), (3, 'below'), (0, '+inf'), (0, '-inf'), (-1, 'below'),
              (0, 'below'), (-1, '-inf'), (3, 'below'), (3, 'nan')]


def _pack_inputs(g, B, topk):
    N = B * topk
    return {'cls': g.integers(0, 3, N).astype(np.int64), 'score': g.uniform(0, 1, N).astype(np.float32),
            'mproj': g.uniform(0, 1280, (N, 2)).astype(np.float32), 'verts': g.uniform(-450, 1050, (N, 16)).astype(np.float32),
            'bbox': g.uniform(0, 1280, (N, 4)).astype(np.float32), 'x': random_boxes(g, N) * g.choice([1.0, -1.0], (N, 1)),
            'fun': g.uniform(0, 0.2, N), 'status': g.integers(-1, 4, N).astype(np.int32)}


@functools.lru_cache(maxsize=None)
def pack_case(name):
    """dict: B, topk, n (B,) int32, the six slot arrays, x / fun / status, fun_accept."""
    if name in PACK_NAMES:
        B, topk, n = PACK_SHAPES[PACK_NAMES.index(name)]
        c = _pack_inputs(rng(100 + PACK_NAMES.index(name)), B, topk)
        c.update(B=B, topk=topk, n=np.array(n, np.int32), fun_accept=FUN_ACCEPT)
        return frozen(c)
    if name.startswith('kept_edge_'):
        acc = EDGE_ACCEPTS[int(name[len('kept_edge_'):])]
        topk = len(EDGE_SLOTS)
        c = _pack_inputs(rng(150), 1, topk)
        value = {'below': np.nextafter(acc, -math.inf), 'equal': acc, '-inf': -math.inf, '+inf': math.inf, 'nan': math.nan}
        c['status'] = np.array([s for s, _ in EDGE_SLOTS], np.int32)
        c['fun'] = np.array([value[k] for _, k in EDGE_SLOTS])
        c.update(B=1, topk=topk, n=np.array([topk], np.int32), fun_accept=acc)
        return frozen(c)
    if name == 'fields':
        # classes 0, negative, 2^24 + 1 (rounds to 2^24 in fp32); x beyond FLT_MAX (inf in the record); the yaw pairs
        topk = 8
        c = _pack_inputs(rng(151), 1, topk)
        c['cls'] = np.array([0, -3, 2 ** 24 + 1, -(2 ** 24 + 1), 1, 2, 2 ** 31 + 3, 0], np.int64)
        for k, (x0, x1) in enumerate(YAW_PAIRS):
            c['x'][k, 0], c['x'][k, 1] = x0, x1
        c['x'][6, 2], c['x'][6, 5], c['x'][7, 3], c['x'][7, 7] = 1e39, -1e300, 3.5e38, -3.5e38
        c['status'] = np.zeros(topk, np.int32)
        c['fun'] = np.full(topk, 0.01)
        c.update(B=1, topk=topk, n=np.array([topk], np.int32), fun_accept=FUN_ACCEPT)
        return frozen(c)
    raise KeyError(name)


PACK_ALL = PACK_NAMES + ['kept_edge_%d' % k for k in range(len(EDGE_ACCEPTS))] + ['fields']


def ry_clear_of_fp32_midpoints(x0, x1):
    """Ry = atan2(x0, x1) lies at least 4 fp64 ulps from the midpoint of two adjacent fp32 values: a one-ulp difference of the
    device's atan2 cannot move the fp32 field."""
    r = math.atan2(x0, x1)
    f = np.float32(r)
    gap = 4 * float(np.spacing(np.float64(abs(r)))) if r != 0 else 0.0
    for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        mid = (float(f) + float(other)) / 2           # exact: two adjacent fp32 values
        if abs(r - mid) < gap:
            return False
    return True


# ------------------------------------------------------------------------------------------------ 2. the box pool
AXES = [0.0, math.pi / 2, math.pi, -math.pi / 2]
WINDOW = [0.9e-3, 1.1e-3]


@functools.lru_cache(maxsize=None)
def pool():
    """[(name, x (8,), k)]: the boxes every projection case is built from; k = the index into KS of the intrinsics the box
    meets when a case has one K per slot.  'win_<axis>_<side>_<size>': a yaw whose smaller of |sin|, |cos| is size, on
    either side of the axis direction."""
    out = []
    body = [4.0, 1.5, 1.7]                                           # l, h, w
    for a, axis in enumerate(AXES):
        for side in (1, -1):
            for size in WINDOW:
                ang = axis + side * math.asin(size)
                out.append(('win_%d_%+d_%g' % (a, side, size), [math.sin(ang), math.cos(ang)] + body + [3.0 + a, 1.0, 9.0 + a], 0))
    for a, pair in enumerate([(0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (-0.0, -1.0)]):
        out.append(('axis_%d' % a, list(pair) + body + [-4.3 + a, 1.2, 12.0], 0))
    ang = math.pi / 2 - math.asin(0.9e-3)
    out.append(('win_nonunit_0.0009', [3.7 * math.sin(ang), 3.7 * math.cos(ang)] + body + [-5.0, 0.8, 10.0], 1))
    out.append(('win_nonunit_0.0011', [0.2 * math.sin(math.asin(1.1e-3)), 0.2 * math.cos(math.asin(1.1e-3))] + body + [5.0, 0.8, 10.0], 1))
    out.append(('far_corners_in_front', [0.0, 1.0, 4.0, 1.5, 2.0, 1.0, 1.0, -0.3], 0))         # Z = -0.3 -+ 1
    out.append(('centre_behind', [0.6, 0.8, 4.0, 1.5, 1.7, 2.0, 1.0, -5.0], 0))
    out.append(('zero_size_inf', [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.5, -1e-6], 0))               # pw + 1e-6 == 0: -inf, +inf
    out.append(('zero_size_nan', [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.5, -1e-6], 2))               # and pu == 0: NaN, +inf
    out.append(('skewed_K', [0.3, -0.9, 3.9, 1.6, 1.8, -2.5, 1.1, 14.0], 1))
    g = rng(7)
    for i, xs in enumerate(random_boxes(g, 57 - len(out))):
        out.append(('random_%d' % i, [float(v) for v in xs], i % 3))
    assert len(out) == 57
    return tuple((n, tuple(x), k) for n, x, k in out)


def pool_index(name):
    return [n for n, _, _ in pool()].index(name)


def snap_margin(xs):
    """Distance of min(|sin ry|, |cos ry|) from the 1e-3 threshold."""
    ry = math.atan2(xs[0], xs[1])
    return abs(min(abs(math.sin(ry)), abs(math.cos(ry))) - ref.SNAP)


def snap_moves(xs, K):
    """Largest change of a rectangle coordinate between the snapped and an unsnapped yardstick, in pixels."""
    a, b = ref.project_box(xs, K, True)[1], ref.project_box(xs, K, False)[1]
    return max(abs(p - q) for p, q in zip(a, b))


PROJECT_NAMES = ['n1', 'n7', 'n8', 'n28', 'n29', 'n57', 'n57_unsolved', 'n29_unsolved', 'b3k19']


@functools.lru_cache(maxsize=None)
def project_case(name):
    """dict: N, topk, x (N, 8), status (N,), K (N or B, 9).  Slots 0..N-1 are the first N of the pool, so slot 7 and slot 28 are
    live window boxes; '_unsolved' marks slots 0, 28 and the last with status < 0."""
    p = pool()
    if name == 'b3k19':
        N, topk = 57, 19
        K = np.array(KS)
    else:
        N, topk = int(name[1:].split('_')[0]), 0
        K = np.array([KS[k] for _, _, k in p[:N]])
    x = np.array([xs for _, xs, _ in p[:N]])
    status = np.array([(0, 1, 3)[i % 3] for i in range(N)], np.int32)
    if name.endswith('_unsolved'):
        status[[0, 28, N - 1]] = (-1, -7, -1)
    return frozen({'N': N, 'topk': topk, 'x': x, 'status': status, 'K': K})


# ------------------------------------------------------------------------------------------------ 3. frames_adjust_K
ADJUST_B = [1, 28, 29, 64, 65, 130]


def geoms_for(B, first=0):
    return [GEOMS[(first + b) % len(GEOMS)] for b in range(B)]


@functools.lru_cache(maxsize=None)
def adjust_case(B):
    g = rng(300 + B)
    K = np.tile(np.array(K_PLAIN), (B, 1)) * g.uniform(0.5, 1.5, (B, 9))
    K[:, 6:] = g.uniform(-1, 1, (B, 3))                                  # row 2 is copied whatever it holds
    K[:, [1, 3]] = g.uniform(-2, 2, (B, 2))
    return frozen({'B': B, 'K': K, 'geoms': geoms_for(B)})


# ------------------------------------------------------------------------------------------------ 4. records_to_camera
CAMERA_SHAPES = [(1, 1), (1, 3), (64, 1), (65, 8), (130, 3)]
CAMERA_NAMES = ['b%dk%d' % s for s in CAMERA_SHAPES] + ['kept_rule', 'alpha', 'clip', 'pool']
# the frames of the clip case: (h, w) fed at their own size on a canvas that holds them (no Resize: scale 1)
CLIP_FRAME = (300, 1000, 300, 1000, 140, 42)


def _records(g, x, flag, fun_accept=FUN_ACCEPT):
    """Records as rtm3d_pack_records would have written them for solver outputs x (consistent fun / status), with the given
    flags: 2 kept, 1 rejected by fun, 0 empty."""
    B, topk = flag.shape
    c = _pack_inputs(g, B, topk)
    c['mproj'], c['verts'], c['bbox'] = (g.uniform(0, 256, c[k].shape).astype(np.float32) for k in ('mproj', 'verts', 'bbox'))
    fl = flag.reshape(-1)
    fun = np.where(fl == 2, 0.01, 5.0)
    status = np.where(fl >= 1, 0, -1).astype(np.int32)
    n = np.full(B, topk, np.int32)
    rec = ref.pack_records(n, c['cls'], c['score'], c['mproj'], c['verts'], c['bbox'], topk, x, fun, status, fun_accept)
    rec[flag == 0] = 0
    return rec, fun, status


def _camera_K(g, B):
    K = np.tile(np.array(K_PLAIN), (B, 1)) * g.uniform(0.9, 1.1, (B, 1))
    K[:, 6:] = (0, 0, 1)
    return K


@functools.lru_cache(maxsize=None)
def camera_case(name):
    """dict: B, topk, rec (B, topk, 32) canvas records, x, fun, status, K (B, 9) camera intrinsics, geoms, fun_accept."""
    g = rng(400 + CAMERA_NAMES.index(name))
    if name in CAMERA_NAMES[:len(CAMERA_SHAPES)]:
        B, topk = CAMERA_SHAPES[CAMERA_NAMES.index(name)]
        # mixed waves: a wave holds the flat slots 2m and 2m + 1; kept and not-kept slots alternate and the alternation flips
        # every four slots, so one half of a wave shuffles while the other does not, in both orders; every third not-kept slot
        # is empty
        s = np.arange(B * topk).reshape(B, topk)
        flag = np.where((s + s // 4) % 2 == 0, 2, np.where(s % 3 == 0, 0, 1))
        x = random_boxes(g, B * topk)
        rec, fun, status = _records(g, x, flag)
        return frozen({'B': B, 'topk': topk, 'rec': rec, 'x': x, 'fun': fun, 'status': status, 'K': _camera_K(g, B),
                       'geoms': geoms_for(B, 1), 'fun_accept': FUN_ACCEPT})
    if name == 'kept_rule':
        # (flag, status, fun) per slot -> a row?   2 consistent: yes.  2 with fun >= fun_accept or status < 0 (inconsistent input):
        # no.  1 with status >= 0 and a small fun (what rtm3d_records_nms3d leaves): no.  0 with garbage in the other 31
        # fields: no, and untouched.
        below = float(np.nextafter(FUN_ACCEPT, 0.0))
        table = [(2, 0, 0.01), (2, 0, 5.0), (1, 0, 0.01), (2, 3, below), (0, 0, 0.01), (2, 0, FUN_ACCEPT), (2, 1, -math.inf),
                 (2, 0, math.nan), (1, 0, 5.0), (2, -1, 0.01), (2, 0, below), (2, 0, math.inf), (1, 3, below), (0, -1, 5.0),
                 (2, 2, 0.0), (1, -1, 0.01)]
        B, topk = 2, len(table)
        x = random_boxes(g, B * topk)
        flag = np.array([[t[0] for t in table]] * B)
        rec, _, _ = _records(g, x, np.where(flag == 0, 1, flag))
        rec[..., 31] = flag
        garbage = g.uniform(-500, 500, (B, topk, 31)).astype(np.float32)
        rec[..., :31] = np.where((flag == 0)[..., None], garbage, rec[..., :31])
        status = np.array([t[1] for t in table] * B, np.int32)
        fun = np.array([t[2] for t in table] * B)
        want_row = np.array([[f == 2 and s >= 0 and v < FUN_ACCEPT for f, s, v in table]] * B)
        return frozen({'B': B, 'topk': topk, 'rec': rec, 'x': x, 'fun': fun, 'status': status, 'K': _camera_K(g, B),
                       'geoms': geoms_for(B, 2), 'fun_accept': FUN_ACCEPT, 'want_row': want_row})
    if name == 'alpha':
        # (ry, unwrapped alpha wanted): ry - atan2(X, Z) in (pi, 2 pi) and (-2 pi, -pi); within 1e-3 of +-pi on both sides;
        # then the two exact cases X = 0 with ry = +-pi from (+-0, -1)
        want = [(3.0, 4.5), (3.0, 6.0), (-3.0, -4.5), (-3.0, -6.0), (2.0, math.pi + 5e-4), (2.0, math.pi - 5e-4),
                (-2.0, -math.pi + 5e-4), (-2.0, -math.pi - 5e-4), (2.5, math.pi + 2e-6), (-2.5, -math.pi - 2e-6)]
        topk = len(want) + 2
        x = random_boxes(g, topk)
        for k, (ry, a) in enumerate(want):
            t = ry - a                                                   # atan2(X, Z)
            x[k, 0], x[k, 1], x[k, 5], x[k, 7] = math.sin(ry), math.cos(ry), 20 * math.sin(t), 20 * math.cos(t)
        x[len(want), :2], x[len(want) + 1, :2] = (0.0, -1.0), (-0.0, -1.0)
        x[len(want):, 5] = 0.0
        rec, fun, status = _records(g, x, np.full((1, topk), 2))
        return frozen({'B': 1, 'topk': topk, 'rec': rec, 'x': x, 'fun': fun, 'status': status, 'K': _camera_K(g, 1),
                       'geoms': [CLIP_FRAME], 'fun_accept': FUN_ACCEPT, 'want_alpha': np.array([a for _, a in want])})
    if name == 'clip':
        # image 0, a 300 x 1000 frame: wholly left, wholly right, cut on the left only, cut on all four sides, inside; image 1, a
        # 1 x 1 frame (xmax = ymax = 0): the same boxes
        boxes = [[0.0, 1.0, 4.0, 1.5, 1.7, -30.0, 1.0, 10.0], [0.0, 1.0, 4.0, 1.5, 1.7, 30.0, 1.0, 10.0],
                 [0.0, 1.0, 4.0, 1.5, 1.7, -8.3, 0.5, 10.0], [0.0, 1.0, 4.0, 3.0, 2.0, 0.0, -0.2, 2.5],
                 [0.3, 0.9, 4.0, 1.5, 1.7, 1.0, 0.4, 20.0]]
        x = np.array(boxes * 2)
        rec, fun, status = _records(g, x, np.full((2, len(boxes)), 2))
        K = np.tile(np.array(K_PLAIN), (2, 1))
        K[:, 2], K[:, 5] = 500.0, 150.0
        return frozen({'B': 2, 'topk': len(boxes), 'rec': rec, 'x': x, 'fun': fun, 'status': status, 'K': K,
                       'geoms': [CLIP_FRAME, GEOMS[5]], 'fun_accept': FUN_ACCEPT,
                       'kinds': ('left', 'right', 'cut_left', 'cut_all', 'inside')})
    if name == 'pool':
        # the whole pool under each of the three intrinsics (snap window, depth and non-finite cases through the KITTI rows)
        topk = len(pool())
        x = np.array([xs for _, xs, _ in pool()] * 3)
        rec, fun, status = _records(g, x, np.full((3, topk), 2))
        return frozen({'B': 3, 'topk': topk, 'rec': rec, 'x': x, 'fun': fun, 'status': status, 'K': np.array(KS),
                       'geoms': [CLIP_FRAME, (300, 1000, 76, 256, 0, 26), CLIP_FRAME], 'fun_accept': FUN_ACCEPT})
    raise KeyError(name)


def clip_margin(case):
    """Smallest distance of an unclipped rectangle coordinate of a kept slot from the clip limits 0 and w - 1 / h - 1, over the
    finite coordinates."""
    un = ref.kitti_rows(case['rec'], case['x'], case['fun'], case['status'], case['K'], case['geoms'], case['fun_accept'], clip=False)
    worst = math.inf
    for b, g in enumerate(case['geoms']):
        for r in range(case['topk']):
            if un[b, r, 14] != 2:
                continue
            for k, lim in ((2, g[1] - 1), (3, g[0] - 1), (4, g[1] - 1), (5, g[0] - 1)):
                v = un[b, r, k]
                if math.isfinite(v):
                    worst = min(worst, abs(v), abs(v - lim))
    return worst


# ------------------------------------------------------------------------------------------------ 5. NMS and the rows
NMS_THRESH = 0.5


@functools.lru_cache(maxsize=None)
def nms_order_case():
    """Two images of six kept slots in score order: slots 1 and 4 nearly repeat slots 0 and 2 (BEV IoU well above 0.5), the
    others stand apart."""
    g = rng(500)
    B, topk = 2, 6
    x = np.zeros((B * topk, 8))
    for b in range(B):
        base = random_boxes(g, topk)
        base[:, 5] = np.array([-12.0, -12.0, 0.0, 12.0, 0.0, 24.0]) + b           # 12 m apart, except the repeats
        base[:, 7] = 30.0
        base[1], base[4] = base[0], base[2]
        base[1, 5] += 0.1
        base[4, 7] += 0.1
        x[b * topk:(b + 1) * topk] = base
    rec, fun, status = _records(g, x, np.full((B, topk), 2))
    rec[..., 1] = np.linspace(0.9, 0.3, topk, dtype=np.float32)[None, :]
    return frozen({'B': B, 'topk': topk, 'rec': rec, 'x': x, 'fun': fun, 'status': status, 'K': _camera_K(g, B),
                   'geoms': [CLIP_FRAME, GEOMS[1]], 'fun_accept': FUN_ACCEPT})
