"""Constructed records that take the rig fusion (csrc/rig.hip) into every regime of its three kernels, and a host model of what
the kernels will do with them - the cases of tests/test_rig_regimes.py (CPU: the model against the yardstick, the regimes, wrong
variants of the model) and of tests/test_gpu_rig_regimes.py (the device against the yardstick).  Host only, seeded, nothing from
outside; the records are written directly, not rendered from a scene.

The linked graphs are built under the ``dist`` metric on a lattice: every centre is a multiple of 1 / 16 m (exact in fp32, and
through the identity extrinsic exact in fp64), thresh = -1.45 links the distance 1 m and not 2 m and is hit by no lattice distance
(the nearest, sqrt(538) / 16 and sqrt(539) / 16, are 3.2e-4 and 4.8e-4 away), so the graph is what the case intends and the
yardstick's decision margin is large by construction; it is asserted all the same, over at most 100 seeds, as rig_cases.case does.
Unless a case says otherwise the candidate at POSITION p of the score order has the score 1 - (p + 1) / 4096 (exact, distinct),
and the candidates are scattered over all record slots q of the rig, with junk (flag 0, flag 1 carrying a box, flag 2 below
min_score, flag 2 with a NaN score, each at the box of a real candidate) in the other slots.

A case: name, R, C, topk, cap, params, ext (R, C, 12), rec (R * C, topk, 32) - the keys of tests/rig_cases.py - and ``regimes``,
the keys of REGIMES in tests/test_rig_regimes.py it is there for.  ``case(name)`` returns (case, the yardstick's result),
computed once per process; ``schedule(case)`` is the host model, see there.  At most three cases hold a rig with n > 1024: the
large regimes that share parameters are the RIGS of one case (star_dense_2048_mean: the star, the dense graph, n = 2047 and a
sparse rig for the stale-workspace test; star_n1025_best; dense_2048_flags_on)."""
import numpy as np

from tests import rig_ref as ref
from tests import rig_cases as rc
from tests import box_overlap_ref as bo

MARGIN = rc.MARGIN
THRESH = -1.45
STEP = 1.0 / 16.0
LANES = 256                      # BO_LANES of csrc/rig.hip
M64 = (1 << 64) - 1
DIST = dict(metric='dist', thresh=THRESH, class_aware=False, cross_only=False, merge='mean', min_score=0.3)
_cache, _sched = {}, {}


# ------------------------------------------------------------------------------------------ records
def pos_score(p):
    return np.float32(1.0 - (p + 1) / 4096.0)


def car(rng, x, z, y=1.0, ry=None):
    """A car-sized box (h w l X Y Z ry) at a centre the caller chose; the sizes are fp32 values."""
    d = (rng.uniform(0.9, 1.1, 3) * np.array([1.6, 1.8, 4.0])).astype(np.float32).astype(np.float64)
    return np.array([d[0], d[1], d[2], x, y, z, rng.uniform(-3.1, 3.1) if ry is None else ry], np.float64)


def item(box, score=None, cls=0.0, cam=None, q=None):
    return dict(box=np.asarray(box, np.float64), score=score, cls=cls, cam=cam, q=q)


def ranked(boxes, cls=None):
    """Items whose position in the score order is their index in ``boxes``."""
    return [item(b, pos_score(p), 0.0 if cls is None else cls[p]) for p, b in enumerate(boxes)]


def below(min_score):
    """The largest fp32 value that is below min_score."""
    with np.errstate(over='ignore'):
        s = np.float32(min_score)
    if np.float64(s) >= min_score:
        s = np.nextafter(s, np.float32(-np.inf))
    return s


def fill(C, topk, items, rng, min_score, junk=True):
    """(C, topk, 32) records of one rig: every item in the record slot q it asks for, in a random slot of the camera it asks for,
    or in a random free slot of the rig; junk in the slots that stay free."""
    N = C * topk
    rec = np.zeros((N, 32), np.float32)
    taken = {it['q'] for it in items if it['q'] is not None}
    assert len(taken) == sum(it['q'] is not None for it in items) and len(items) <= N
    free = [int(q) for q in rng.permutation(N) if int(q) not in taken]
    for it in items:
        if it['q'] is not None:
            q = it['q']
        elif it['cam'] is not None:
            q = next(f for f in free if f // topk == it['cam'])
            free.remove(q)
        else:
            q = free.pop()
        rec[q, 0], rec[q, 1], rec[q, 31] = it['cls'], it['score'], 2.0
        rec[q, 2:24] = rng.uniform(0, 300, 22)
        rec[q, 24:31] = it['box']
    for n, q in enumerate(sorted(free)):
        kind = n % 4 if junk else 1
        src = items[int(rng.integers(len(items)))] if items else item(car(rng, 0.0, 0.0), 0.9)
        if kind == 1:
            continue                                             # an empty slot
        rec[q, 0], rec[q, 24:31] = src['cls'], src['box']
        rec[q, 2:24] = rng.uniform(0, 300, 22)
        if kind == 0:
            rec[q, 1], rec[q, 31] = 0.99, 1.0                    # a 2D-only slot carrying a box
        elif kind == 2 and min_score > -np.inf:
            rec[q, 1], rec[q, 31] = below(min_score), 2.0        # a kept slot just below min_score
        else:
            rec[q, 1], rec[q, 31] = np.nan, 2.0                  # a kept slot whose score is not a number
    return rec.reshape(C, topk, 32)


def identity(R, C):
    return np.tile(np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (R, C, 1))


# ------------------------------------------------------------------------------------------ graphs, as boxes by position
def far(i):
    """Filler i: 4 m from every other filler and far from everything placed by hand."""
    return 2000.0 + 4.0 * (i % 40), 2000.0 + 4.0 * (i // 40)


def dense(rng, n, side=None):
    """n random lattice points of a square; by default of the density of 2048 points in 60 m x 60 m (about 1.9 links per point)."""
    side = 60.0 * np.sqrt(n / 2048.0) if side is None else side
    k = max(int(side / STEP), 1)
    xz = rng.integers(0, k + 1, (n, 2)) * STEP
    return [car(rng, x, z) for x, z in xz]


def chain(rng, length, n, lead=0):
    """``lead`` isolated boxes, then ``length`` boxes 1 m apart on a line in the order of their scores, then isolated ones."""
    xz = [far(i) for i in range(lead)] + [(float(p), 0.0) for p in range(length)] + [far(lead + i) for i in range(n - lead - length)]
    return [car(rng, x, z) for x, z in xz]


def explicit(rng, n, placed):
    """placed: {position: (x, z)}; every other position an isolated filler."""
    return [car(rng, *(placed[p] if p in placed else far(p))) for p in range(n)]


def groups(rng, sizes, tail=None, fold=None):
    """Clusters of the given sizes: group g sits within +-0.5 m of the site (8 g, 0), so its boxes are linked to one another and
    to nothing else, and its earliest box is its representative.  The positions are a random interleaving; the boxes of group
    ``tail`` come last, behind all others.  fold = g: the members of group g get headings on both sides of +-pi / 2 from the
    representative's."""
    labels = [g for g, s in enumerate(sizes) for _ in range(s) if g != tail]
    labels = [labels[i] for i in rng.permutation(len(labels))] + ([tail] * sizes[tail] if tail is not None else [])
    turns = [0.1, np.pi / 2 - 0.3, np.pi / 2 + 0.3, -(np.pi / 2 - 0.3), -(np.pi / 2 + 0.3), 3.0, -3.0, -0.2]
    seen, boxes = {}, []
    for g in labels:
        k = seen.get(g, 0)
        seen[g] = k + 1
        off = rng.integers(-8, 9, 2) * STEP
        ry = None
        if g == fold:
            ry = 0.3 if k == 0 else 0.3 + turns[k % len(turns)]
        boxes.append(car(rng, 8.0 * g + off[0], off[1], y=1.0 + rng.integers(-2, 3) * STEP, ry=ry))      # at most sqrt(1 + 1 + 1 / 16) = 1.436 m apart
    return boxes


def star(rng, n):
    """n boxes within 0.65 m of one point (and 0.19 m of one height): every pair is linked, the first box represents them all."""
    out = []
    while len(out) < n:
        x, z = rng.integers(-10, 11, 2) * STEP
        if x * x + z * z <= 0.65 * 0.65:
            out.append(car(rng, 100.0 + x, 50.0 + z, y=1.0 + rng.integers(-3, 4) * STEP))
    return out


def road(rng, n, side, ext, classes=1):
    """n car boxes with random yaw at random places of a square, each written in the coordinates of a random camera of ``ext``
    (C, 3, 4): the dense graph of the IoU metrics.  Returns items with a camera each."""
    out = []
    for p in range(n):
        x, z = rng.uniform(-side / 2, side / 2, 2)
        b = car(rng, x, z, y=1.0 + rng.uniform(-0.3, 0.3))
        c = int(rng.integers(ext.shape[0]))
        pos, ry = rc.to_camera(b[3:6], b[6], ext[c])
        out.append(item(np.concatenate([b[:3], pos, [ry]]), pos_score(p), float(rng.integers(classes)), cam=c))
    return out


# ------------------------------------------------------------------------------------------ the cases
def make(name, C, topk, rigs, rng, params, cap=None, ext=None, regimes=(), junk=True, **note):
    R = len(rigs)
    c = dict(name=name, R=R, C=C, topk=topk, params=params, cap=min(256, C * topk) if cap is None else cap, regimes=tuple(regimes))
    c['ext'] = identity(R, C) if ext is None else np.ascontiguousarray(np.asarray(ext, np.float64)[..., :3, :].reshape(R, C, 12))
    c['rec'] = np.ascontiguousarray(np.concatenate([fill(C, topk, items, rng, params['min_score'], junk) for items in rigs]))
    c.update(note)
    return c


def build(name, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    P = lambda **kw: ref.params(**dict(DIST, **kw))
    if name == 'sort_n1_63_64_65':
        # C = 1, topk = 65, four rigs: M = 64 with one key, one pad, no pad; n = 65 = N: M = 128, the first stage with j >= 64
        return make(name, 1, 65, [ranked(dense(rng, n)) for n in (1, 63, 64, 65)], rng, P(), regimes=('sort_sizes', 'odd_stride'))
    if name == 'sort_n128_to_513':
        # C = 3, topk = 171 (N = 513, three 256-slot passes, odd), six rigs: both sides of M = 128, 256, 512 and n = N = 513 (M = 1024)
        return make(name, 3, 171, [ranked(dense(rng, n)) for n in (128, 129, 256, 257, 512, 513)], rng, P(),
                    regimes=('sort_sizes', 'scattered', 'odd_stride'))
    if name == 'sort_n1024':
        # every second slot of N = 2048 a candidate: M = 1024, two pairs per lane; 32 link words per row, 16 of them in use
        return make(name, 16, 128, [ranked(dense(rng, 1024))], rng, P(), regimes=('sort_sizes', 'scattered'))
    if name == 'star_dense_2048_mean':
        # C = 16, topk = 128 (N = 2048): the star and the dense graph with n = N (nothing padded, every slot a candidate), n = 2047
        # (one pad), and a sparse rig of 300 for the stale-workspace test
        rigs = [ranked(star(rng, 2048)), ranked(dense(rng, 2048)), ranked(dense(rng, 2047)), ranked(dense(rng, 300, side=60.0))]
        return make(name, 16, 128, rigs, rng, P(), regimes=('sort_sizes', 'star', 'dense_2048', 'scattered', 'capacity_overflow'))
    if name == 'star_n1025_best':
        rigs = [ranked(star(rng, 2048)), ranked(dense(rng, 1025))]
        return make(name, 16, 128, rigs, rng, P(merge='best'), regimes=('sort_sizes', 'star'))
    if name == 'dense_2048_flags_on':
        boxes = dense(rng, 2048)
        return make(name, 16, 128, [ranked(boxes, cls=[float(v) for v in rng.integers(0, 2, 2048)])], rng,
                    P(class_aware=True, cross_only=True), regimes=('dense_2048',))
    if name == 'odd_n_three_rigs':
        return make(name, 3, 7, [ranked(dense(rng, n, side=5.0)) for n in (15, 21, 8)], rng, P(), regimes=('odd_stride',))
    if name == 'ties':
        # 100 candidates, six scores: ties across cameras and within a camera decide most of the order
        boxes = dense(rng, 100)
        pool = np.array([0.9, 0.75, 0.75 + 2.0 ** -20, 0.5, 0.4, 0.31], np.float32)
        items = [item(b, pool[int(rng.integers(len(pool)))]) for b in boxes]
        return make(name, 4, 32, [items], rng, P(), regimes=('ties',))
    if name == 'keys_negative_special':
        # min_score = -inf, merge best: +inf first, denormals of both signs, -0 against +0 in both slot orders, negative scores, -inf last
        boxes = dense(rng, 110)
        sc = [np.float32(v) for v in rng.uniform(-1.0, 1.0, 96)]
        items = [item(b, s) for b, s in zip(boxes, sc)]
        fixed = [(3, -0.0), (5, 0.0), (7, 0.0), (9, -0.0), (40, np.inf), (41, -np.inf), (70, 1e-40), (71, -1e-40), (100, -np.inf), (101, 1.5),
                 (102, -1.5), (103, 2.0 ** -126), (104, -2.0 ** -149), (105, np.inf)]
        with np.errstate(under='ignore'):
            items += [item(b, np.float32(s), q=q) for b, (q, s) in zip(boxes[96:], fixed)]
        return make(name, 4, 32, [items], rng, P(merge='best', min_score=-np.inf), regimes=('keys_special',))
    if name == 'min_score_edge':
        # a score exactly min_score is kept, the fp32 value below it (junk kind 2) is dropped; min_score is not an fp32 value's
        # neighbour by accident: 0.3f as a double
        ms = float(np.float32(0.3))
        boxes = dense(rng, 40)
        items = [item(b, np.float32(0.3) if p % 4 == 0 else pos_score(p)) for p, b in enumerate(boxes)]
        return make(name, 2, 40, [items], rng, P(min_score=ms), regimes=('min_score_edge',))
    if name == 'min_score_inf':
        # nothing is kept: n = 0, with flag-2 slots of finite scores (up to the largest fp32) and of NaN present
        return make(name, 2, 40, [[]], rng, P(min_score=np.inf), regimes=('min_score_inf',))
    if name == 'link_every_word':
        # n = 330: row 329, 1 m from the point where the positions 64 w and 64 w + 63 (w < 5), 320 and 328 sit
        sel = [64 * w + b for w in range(5) for b in (0, 63)] + [320, 328]
        placed = {p: (0.0, 0.0) for p in sel}
        placed[329] = (1.0, 0.0)
        return make(name, 6, 64, [ranked(explicit(rng, 330, placed))], rng, P(), regimes=('link_every_word',), row=329, cols=sel)
    if name == 'class_nan':
        # class_aware: two copies of one box with a NaN class link to nothing, two copies with class 1 link
        b0, b1 = car(rng, 0.0, 0.0), car(rng, 20.0, 0.0)
        items = [item(b0, 0.9, np.nan, cam=0), item(b0, 0.8, np.nan, cam=1), item(b1, 0.7, 1.0, cam=0), item(b1, 0.6, 1.0, cam=1),
                 item(b1, 0.5, 2.0, cam=1)]
        return make(name, 2, 8, [items], rng, P(class_aware=True, cross_only=True), regimes=('class_nan',))
    if name == 'cross_only_one_camera':
        boxes = [car(rng, 8.0 * (p // 3), 0.0) for p in range(12)]
        return make(name, 3, 16, [[item(b, pos_score(p), cam=1) for p, b in enumerate(boxes)]], rng, P(cross_only=True),
                    regimes=('cross_only_one_camera',))
    if name == 'iou_bad_boxes':
        # BEV IoU: good twins, and at their very place boxes with w = 0, w < 0, a NaN centre, an infinite length: clusters of one
        g = car(rng, 5.0, 20.0, ry=0.4)
        bad = [g.copy() for _ in range(4)]
        bad[0][1], bad[1][1], bad[2][3], bad[3][2] = 0.0, -1.8, np.nan, np.inf
        items = [item(g, 0.9, cam=0), item(g, 0.8, cam=1)] + [item(b, 0.85 - 0.01 * i, cam=i % 2) for i, b in enumerate(bad)] \
            + [item(b, 0.5 - 0.01 * i, cam=(i + 1) % 2) for i, b in enumerate(bad)]
        return make(name, 2, 8, [items], rng, ref.params(metric='bev', thresh=0.1, class_aware=False, cross_only=False, merge='mean', min_score=0.3),
                    regimes=('iou_bad_boxes',))
    if name == 'reach_bar':
        # BEV IoU with a bar of 1e-5.  Squares of side 2 standing on a corner (yaw pi / 4, half diagonal sqrt 2, reach 2.828): at
        # 2.80 m their tips overlap by an IoU of 5e-5 - inside the reach, linked; at 2.86 m the shortcut gives 0.  Axis-parallel
        # squares 2.5 m apart are inside the reach and do not touch: 0 through the polygon path.
        sq = lambda x, z, ry: np.array([1.5, 2.0, 2.0, x, 1.0, z, ry])
        items = [item(sq(0.0, 0.0, np.pi / 4), 0.9), item(sq(2.80, 0.0, np.pi / 4), 0.8), item(sq(0.0, 20.0, np.pi / 4), 0.7),
                 item(sq(2.86, 20.0, np.pi / 4), 0.6), item(sq(0.0, 40.0, 0.0), 0.5), item(sq(2.5, 40.0, 0.0), 0.4)]
        return make(name, 2, 4, [items], rng, ref.params(metric='bev', thresh=1e-5, class_aware=False, cross_only=False, merge='best', min_score=0.3),
                    regimes=('reach_bar',))
    if name in ('chain_parity0', 'chain_parity1'):
        lead = int(name[-1])
        return make(name, 4, 64, [ranked(chain(rng, 210, 230 + lead, lead))], rng, P(), regimes=(name,))
    if name == 'two_reps_other_chunks':
        # A (position 3) and B (70) are 2 m apart; X (140) between them joins A through the push of chunk 0; Y (75) in B's own
        # chunk, linked to both, is taken by A before chunk 1 is settled.  A chain of 10 from position 200 on.
        placed = {3: (0.0, 0.0), 70: (2.0, 0.0), 140: (1.0, 0.0), 75: (1.0, 0.0625)}
        placed.update({200 + k: (float(k), 30.0) for k in range(10)})
        return make(name, 4, 64, [ranked(explicit(rng, 222, placed))], rng, P(), regimes=('two_reps_other_chunks',))
    if name == 'two_reps_same_chunk':
        # A (5) and B (9) of chunk 0; X (20, settled in chunk 0) and X2 (100, pushed) are linked to both and join A
        placed = {5: (0.0, 0.0), 9: (2.0, 0.0), 20: (1.0, 0.0), 100: (1.0, 0.0625)}
        return make(name, 4, 64, [ranked(explicit(rng, 150, placed))], rng, P(), regimes=('two_reps_same_chunk',))
    if name in ('member_link_same_chunk', 'member_link_earlier_chunk'):
        # A (2) - M (10) - X in a row, 1 m apart: X is linked to the member M only and represents itself
        x = 40 if name == 'member_link_same_chunk' else 100
        placed = {2: (0.0, 0.0), 10: (1.0, 0.0), x: (2.0, 0.0)}
        return make(name, 4, 64, [ranked(explicit(rng, 150, placed))], rng, P(), regimes=(name,), x=x)
    if name in ('dense_300_bev', 'dense_300_iou3d'):
        ext = rc.ring(6, rng, tilt=name.endswith('iou3d'))
        Q = ref.params(metric=name.split('_')[-1], thresh=0.1, class_aware=name.endswith('iou3d'), cross_only=name.endswith('iou3d'),
                       merge='mean', min_score=0.3)
        return make(name, 6, 80, [road(rng, 300, 42.0, ext, classes=2)], rng, Q, ext=ext[None], regimes=('dense_300',))
    if name in ('cap_exact', 'cap_plus_one'):
        sizes = [1, 2, 3, 1, 4, 2, 1, 3, 2, 1, 5, 2] + ([4] if name == 'cap_plus_one' else [])
        boxes = groups(rng, sizes, tail=12 if name == 'cap_plus_one' else None)
        return make(name, 3, 16, [ranked(boxes)], rng, P(), cap=12, regimes=(name,))
    if name == 'cap_one':
        boxes = groups(rng, [3, 2, 4, 1])
        return make(name, 2, 8, [ranked(boxes)], rng, P(), cap=1, regimes=(name,))
    if name == 'cap_256_n4':
        boxes = groups(rng, [2, 1, 1])
        return make(name, 1, 4, [ranked(boxes)], rng, P(), cap=256, regimes=(name,))
    if name == 'sizes_2_5_70_heading_fold':
        boxes = groups(rng, [2, 5, 70, 1, 1, 1, 3], fold=2)
        return make(name, 4, 32, [ranked(boxes)], rng, P(), regimes=('cluster_sizes', 'heading_fold'))
    raise KeyError(name)


NAMES = ('sort_n1_63_64_65', 'sort_n128_to_513', 'sort_n1024', 'star_dense_2048_mean', 'star_n1025_best', 'dense_2048_flags_on',
         'odd_n_three_rigs', 'ties', 'keys_negative_special', 'min_score_edge', 'min_score_inf', 'link_every_word', 'class_nan',
         'cross_only_one_camera', 'iou_bad_boxes', 'reach_bar', 'chain_parity0', 'chain_parity1', 'two_reps_other_chunks',
         'two_reps_same_chunk', 'member_link_same_chunk', 'member_link_earlier_chunk', 'dense_300_bev', 'dense_300_iou3d', 'cap_exact',
         'cap_plus_one', 'cap_one', 'cap_256_n4', 'sizes_2_5_70_heading_fold')
SORT_N = (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048)


def case(name):
    """The case and the yardstick's result; reseeded until the margin is >= MARGIN."""
    if name not in _cache:
        first = 10000 + 100 * NAMES.index(name)
        for seed in range(first, first + 100):
            c = build(name, seed)
            res = ref.fuse(c['rec'], c['ext'], c['R'], c['C'], c['params'], c['cap'])
            if res['margin'] >= MARGIN:
                _cache[name] = (c, res)
                break
        else:
            raise RuntimeError('no seed gives case %s a decision margin of %g' % (name, MARGIN))
    return _cache[name]


def cases():
    return [case(n)[0] for n in NAMES]


def reference(c):
    return case(c['name'])[1]


# ------------------------------------------------------------------------------------------ the host model of the schedule
def key_of(r, q, min_score, C, topk, variant=None):
    """rig_key: the ascending 64-bit key of record slot q."""
    s = np.float32(r[1])
    with np.errstate(invalid='ignore'):
        if not (r[31] == np.float32(2.0) and np.float64(s) >= min_score):
            return (0xffffffff << 32) | q
    u = 0 if s == np.float32(0.0) and variant != 'signed_zero' else int(np.array(s, np.float32).view(np.uint32))
    u = (~u & 0xffffffff) if u & 0x80000000 and variant != 'no_negative_branch' else (u | 0x80000000)
    low = q if variant != 'slot_before_camera' else (q % topk) * C + q // topk
    return ((~u & 0xffffffff) << 32) | low


def bitonic(key, variant=None):
    """The network of rig_prepare_kernel over the M keys, stage by stage; the exchanges of one stage touch disjoint pairs.
    Wrong variants: 'sort_direction' (every stage j = 64 exchanges the other way round.  In a merge before the last this leaves
    each block a rotation of its sorted self - still bitonic, so the next merge repairs it; only in the last merge, kk = M, does
    it show: an error in one stage is visible at ONE padded size, which is why every M has its case), 'sort_one_pair_per_lane'
    (the in-wave stages j <= 32 run for a lane's first pair t only)."""
    M, kk = len(key), 2
    while kk <= M:
        j = kk >> 1
        while j > 0:
            up = 0 if variant == 'sort_direction' and j == 64 else 1
            for t in range(min(M >> 1, LANES) if variant == 'sort_one_pair_per_lane' and j <= 32 else M >> 1):
                i = ((t & ~(j - 1)) << 1) | (t & (j - 1))
                o = i | j
                a, b = key[i], key[o]
                if (a > b) == (((i & kk) == 0) == bool(up)):
                    key[i], key[o] = b, a
            j >>= 1
        kk <<= 1
    return key


def prepare(c, r, variant=None):
    """rig_prepare_kernel up to the end of the sort: the keys of rig r, the ballot compaction (slot order; any order would do),
    the padding to M, the network.  Returns (n, M, the M keys after the network)."""
    C, topk, P = c['C'], c['topk'], c['params']
    N = C * topk
    rec = c['rec'][r * C:(r + 1) * C].reshape(N, 32)
    keys = [key_of(rec[q], q, P['min_score'], C, topk, variant) for q in range(N)]
    cand = [k for k in keys if k >> 32 != 0xffffffff]
    n, M = len(cand), 64
    while M < n:
        M <<= 1
    net = bitonic(cand + [(1 << 64) - 1] * (M - n), variant)
    assert len(set(cand)) == n and (net == sorted(net) or str(variant).startswith('sort_'))
    return n, M, net


def link_rows(boxes, cam, cls, P):
    """rig_link_kernel: row i as an int, bit j < i = linked(i, j)."""
    n = len(boxes)
    if n == 0:
        return []
    B = np.array(boxes, np.float64).reshape(n, 7)
    cam, cls = np.asarray(cam), np.asarray(cls, np.float32)
    ok = np.tril(np.ones((n, n), bool), -1)
    if P['cross_only']:
        ok &= cam[:, None] != cam[None, :]
    if P['class_aware']:
        ok &= cls[:, None] == cls[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        ex, ey, ez = B[None, :, 3] - B[:, None, 3], B[None, :, 4] - B[:, None, 4], B[None, :, 5] - B[:, None, 5]     # [i][j]: a = box j, b = box i
        if ref.METRICS[P['metric']] == 2:
            L = ok & (-np.sqrt((ex * ex + ey * ey) + ez * ez) > P['thresh'])
        else:
            half = 0.5 * np.sqrt(B[:, 1] * B[:, 1] + B[:, 2] * B[:, 2])
            reach = half[None, :] + half[:, None]
            inside = ok & ~(ex * ex + ez * ez > reach * reach)
            L = ok & ~inside & (0.0 > P['thresh'])
            for i, j in np.argwhere(inside):
                bev, vol = bo.overlap(B[j], B[i])
                L[i, j] = (bev if P['metric'] == 'bev' else vol) > P['thresh']
    packed = np.packbits(L, axis=1, bitorder='little')
    return [int.from_bytes(packed[i].tobytes(), 'little') for i in range(n)]


def ffs(x):
    return (x & -x).bit_length() - 1


def scan(rows, n, variant=None):
    """rig_cluster_kernel's chunked scan.  Returns rep_of, rounds per chunk, taken per position ('rep', 'settle', 'push')."""
    pick = ffs if variant != 'latest_rep' else (lambda x: x.bit_length() - 1)
    nch = (n + 63) >> 6
    rep_of, taken, rounds, repmask = [-1] * n, [None] * n, [], []
    word = lambda i, c: (rows[i] >> (64 * c)) & M64
    for c in range(nch):
        # wave 0 settles the chunk
        open_ = [64 * c + l < n and rep_of[64 * c + l] < 0 for l in range(64)]
        mine = [word(64 * c + l, c) & ((1 << l) - 1) if open_[l] else 0 for l in range(64)]
        settled = M64 & ~sum(1 << l for l in range(64) if open_[l])
        reps, r = 0, 0
        while settled != M64:
            ready = [open_[l] and not (settled >> l) & 1 and (mine[l] & ~settled) == 0 for l in range(64)]
            rb = sum(1 << l for l in range(64) if ready[l])
            pb = sum(1 << l for l in range(64) if ready[l] and (mine[l] & reps) == 0)
            reps |= pb
            settled |= rb
            r += 1
            assert rb, 'the lowest unsettled lane is always ready'
        for l in range(64):
            if open_[l]:
                i = 64 * c + l
                rep_of[i] = i if (reps >> l) & 1 else 64 * c + pick(mine[l] & reps)
                taken[i] = 'rep' if (reps >> l) & 1 else 'settle'
        rounds.append(r)
        repmask.append(reps)
        # every lane pushes the chunk's representatives to the later rows (their word c was fetched a chunk ahead)
        for i in range(64 * (c + 1), n):
            w = word(i, c + 1) if variant == 'push_next_word' else word(i, c)
            x = w & reps
            if x and (rep_of[i] < 0 or variant == 'push_overwrites'):
                rep_of[i] = 64 * c + pick(x)
                taken[i] = 'push'
    return rep_of, rounds, taken, repmask


def schedule(c, variant=None):
    """What the three kernels of rtm3d_rig_fuse will do with the case, restated in plain Python from csrc/rig.hip: per rig a dict
      n, M, pairs (the pairs t a lane of the sort owns, max(1, M / 2 / 256)), order [(camera, slot)] by position,
      rounds [settle rounds of chunk c], rep_of [position -> position], taken [position -> 'rep' | 'settle' | 'push'],
      chunk_dist [position -> chunks between a member and its representative, 0 for a representative],
      ncl, cap, sizes [members per cluster], largest, clusters [[(camera, slot)]] representative first, map (C, topk), counts (2,).
    ``variant`` names a deliberately wrong schedule (tests/test_rig_regimes.py): 'push_next_word', 'latest_rep',
    'push_overwrites', 'slot_before_camera', 'signed_zero', 'no_negative_branch'."""
    if (c['name'], variant) in _sched:
        return _sched[c['name'], variant]
    C, topk, cap, P = c['C'], c['topk'], c['cap'], c['params']
    N = C * topk
    out = []
    for r in range(c['R']):
        rec = c['rec'][r * C:(r + 1) * C].reshape(N, 32)
        n, M, net = prepare(c, r, variant)
        qs = [k & 0xffffffff for k in net[:n]]
        if variant == 'slot_before_camera':
            qs = [(v % C) * topk + v // C for v in qs]
        order = [(q // topk, q % topk) for q in qs]
        boxes = [ref.transform(rec[q, 24:31].astype(np.float64), c['ext'][r, q // topk]) for q in qs]
        rows = link_rows(boxes, [q // topk for q in qs], [rec[q, 0] for q in qs], P)
        rep_of, rounds, taken, repmask = scan(rows, n, variant)
        # output slots by prefix popcount, the map, the counters
        reps = [p for p in range(n) if rep_of[p] == p]
        assert reps == [64 * w + b for w, m in enumerate(repmask) for b in range(64) if (m >> b) & 1]
        slot = {p: s for s, p in enumerate(reps)}
        omap = np.full((C, topk), -1, np.int32)
        for p in range(n):
            s = slot[rep_of[p]]
            omap[order[p]] = s if s < cap else -2
        members = {p: [p] for p in reps}
        for p in range(n):
            if rep_of[p] != p:
                members[rep_of[p]].append(p)                     # the walk over next_of: by position
        ncl = len(reps)
        sizes = [len(members[p]) for p in reps]
        out.append(dict(n=n, M=M, pairs=max(1, M // 2 // LANES), order=order, rounds=rounds, rep_of=rep_of, taken=taken,
                        chunk_dist=[(p >> 6) - (rep_of[p] >> 6) for p in range(n)], ncl=ncl, cap=cap, sizes=sizes,
                        largest=max(sizes) if sizes else 0, clusters=[[order[p] for p in members[j]] for j in reps], map=omap,
                        counts=np.array([min(ncl, cap), max(ncl - cap, 0)], np.int32), rows=rows, reps=reps))
    _sched[c['name'], variant] = out
    return out


def same_as_yardstick(c, sch, want):
    """Does a schedule agree with the yardstick on the representatives and members, the map and n?"""
    C = c['C']
    return all(s['clusters'] == want['clusters'][r] and np.array_equal(s['map'], want['map'][r * C:(r + 1) * C])
               and np.array_equal(s['counts'], want['n'][r]) for r, s in enumerate(sch))
