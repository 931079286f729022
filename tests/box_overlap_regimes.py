"""Cases for every regime of csrc/box_geom.h + csrc/box_overlap.hip (box_overlaps_kernel, records_nms3d_kernel), an EXACT
yardstick of the rotated-box overlap, and host models of the two kernels.  Host only; shared by tests/test_box_overlap_regimes.py
(which asserts that every case is in the regime it is named for and that the cases tell wrong kernels from the right one) and
tests/test_gpu_box_overlap_regimes.py.

The exact yardstick (``exact_overlap``) takes c = cos(ry), s = sin(ry) from numpy in fp64 and does everything after that in
``fractions.Fraction``: corner offsets relative to b's centre (distance from the origin costs no digits), Sutherland-Hodgman with
closed inside tests against b's four directed edges in those world-parallel coordinates (NOT in b's frame, as the device does),
shoelace area, vertical overlap, ratio.  Only the final conversion to float rounds.

The pair set of ``pair_set()`` is built as POOLS of pairs (not an N x N product) and meant to be launched as B = npairs,
cap_a = cap_b = 1: every lane of a 256-lane block is its own pair, neighbours hold polygons of different vertex counts.
The NMS cases are constructed: boxes sit on a lattice whose pitch (8 m) is larger than the largest footprint diagonal (4.48 m),
so only the planted pairs meet and the expected flags follow from the construction.
"""
import functools
from fractions import Fraction as F

import numpy as np

from tests import box_overlap_ref as ref
from tests import box_overlap_cases as cases

CRITERIA = ref.CRITERIA
NEAR_ANGLES = (1e-15, 1e-12, 1e-9, 1e-6, 1e-4)      # rad between the closest edges of a near-parallel pair
FRAGILE = 1e-9                                      # m: no corner of a random pair is closer than this to an edge line of the other box
LATTICE = 2.0 ** -10
PI = F('3.14159265358979323846264338327950288419716939937510582097494459')
PITCH = 8.0                                         # m, the lattice of the NMS cases
NMS_BOX = (1.5, 2.0, 4.0)                           # h, w, l of the NMS cases: footprint diagonal 4.48 < PITCH


# ------------------------------------------------------------------------------------------------ the exact yardstick
def _corners(box, origin):
    """Corners (x, z) of the footprint as Fractions, relative to ``origin`` (X, Z), in the order of box_overlap_ref.footprint."""
    h, w, l, X, Y, Z, ry = [float(v) for v in box]
    c, s = F(float(np.cos(ry))), F(float(np.sin(ry)))
    dX, dZ = F(X) - origin[0], F(Z) - origin[1]
    hl, hw = F(l) / 2, F(w) / 2
    return [(c * lx + s * lz + dX, c * lz - s * lx + dZ) for lx, lz in ((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw))]


def _shoelace(poly):
    return sum(poly[i - 1][0] * poly[i][1] - poly[i - 1][1] * poly[i][0] for i in range(len(poly)))


def _clip(subject, clipper, closed=True):
    """Sutherland-Hodgman in exact arithmetic: ``subject`` inside the convex ``clipper``."""
    if _shoelace(clipper) < 0:
        clipper = clipper[::-1]
    out = list(subject)
    for k in range(len(clipper)):
        (ex, ez), (fx, fz) = clipper[k], clipper[(k + 1) % len(clipper)]
        dx, dz = fx - ex, fz - ez
        side = [dx * (p[1] - ez) - dz * (p[0] - ex) for p in out]
        inp, out = out, []
        for i in range(len(inp)):
            cur, prev, sc, sp = inp[i], inp[i - 1], side[i], side[i - 1]
            cin, pin = (sc >= 0, sp >= 0) if closed else (sc > 0, sp > 0)
            if cin != pin:
                t = sp / (sp - sc)
                out.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
            if cin:
                out.append(cur)
        if not out:
            break
    return out


def _far_apart(a, b):
    """Certainly disjoint footprints, from plain sums: a half diagonal is at most (l + w) / 2 (and |c|, |s| <= 1 + 2^-52)."""
    reach = (a[1] + a[2] + b[1] + b[2]) / 2 * (1 + 1e-9)
    return abs(a[3] - b[3]) > reach or abs(a[5] - b[5]) > reach


def exact_pair(a, b, closed=True):
    """(intersection area, vertical overlap, footprint area a, footprint area b) as Fractions, the number of DISTINCT vertices
    of the intersection polygon and how many of them are a corner of neither box.  Zeros for an invalid box."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not (ref.valid(a) and ref.valid(b)):
        return F(0), F(0), F(0), F(0), 0, 0
    sa, sb = F(float(a[2])) * F(float(a[1])), F(float(b[2])) * F(float(b[1]))
    ov = max(F(0), min(F(float(a[4])) + F(float(a[0])) / 2, F(float(b[4])) + F(float(b[0])) / 2)
             - max(F(float(a[4])) - F(float(a[0])) / 2, F(float(b[4])) - F(float(b[0])) / 2))
    if _far_apart(a, b):
        return F(0), ov, sa, sb, 0, 0
    origin = (F(float(b[3])), F(float(b[5])))
    ca, cb = _corners(a, origin), _corners(b, origin)
    poly = _clip(ca, cb, closed)
    verts = set(poly)
    inter = abs(_shoelace(poly)) / 2 if len(poly) >= 3 else F(0)
    return inter, ov, sa, sb, len(verts), len(verts - set(ca) - set(cb))


def _ratio(inter, sa, sb, criterion):
    den = {'iou': sa + sb - inter, 'a': sa, 'b': sb}[criterion]
    return float(inter / den) if den > 0 else 0.0


def ratios(geom, a, b, criterion):
    inter, ov, sa, sb = geom[:4]
    return _ratio(inter, sa, sb, criterion), _ratio(inter * ov, sa * F(float(a[0])), sb * F(float(b[0])), criterion)


def exact_overlap(a, b, criterion='iou'):
    """((bev, vol) overlap of two boxes, correctly rounded from exact rationals; number of distinct vertices of the polygon)."""
    g = exact_pair(a, b)
    return ratios(g, a, b, criterion), g[4]


# ------------------------------------------------------------------------------------------------ host model of box_geom.h
def model_overlap(a, b, criterion='iou', maxv=8, closed=True, stages=None):
    """The operation sequence of box_geom.h (box_prepare, box_pair, overlap_ratio) in python floats: fp64, no contraction.
    ``maxv`` and ``closed`` make the wrong clips of tests/test_box_overlap_regimes.py; ``stages``: a list that receives the vertex
    count after each clip that ran.  Returns (bev, vol, final vertex count)."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    if not (ref.valid(a) and ref.valid(b)):
        return 0.0, 0.0, 0
    inside = (lambda d: d >= 0.0) if closed else (lambda d: d > 0.0)
    ac, as_, bc, bs = float(np.cos(a[6])), float(np.sin(a[6])), float(np.cos(b[6])), float(np.sin(b[6]))
    ahl, ahw, bhl, bhw = a[2] / 2.0, a[1] / 2.0, b[2] / 2.0, b[1] / 2.0
    ov = max(min(a[4] + a[0] / 2.0, b[4] + b[0] / 2.0) - max(a[4] - a[0] / 2.0, b[4] - b[0] / 2.0), 0.0)
    dX, dZ = a[3] - b[3], a[5] - b[5]
    poly = []
    for k in range(4):
        lx = ahl if k in (0, 3) else -ahl
        lz = ahw if k < 2 else -ahw
        wx, wz = (ac * lx + as_ * lz) + dX, (ac * lz - as_ * lx) + dZ
        poly.append((bc * wx - bs * wz, bs * wx + bc * wz))
    for axis, sign, bound in ((0, 1.0, bhl), (0, -1.0, bhl), (1, 1.0, bhw), (1, -1.0, bhw)):
        if not poly:
            break
        out, prev = [], poly[-1]
        dprev = bound - sign * prev[axis]
        for cur in poly:
            dcur = bound - sign * cur[axis]
            if inside(dcur) != inside(dprev):
                t = dprev / (dprev - dcur)
                q = (sign * bound, prev[1] + t * (cur[1] - prev[1])) if axis == 0 else (prev[0] + t * (cur[0] - prev[0]), sign * bound)
                if len(out) < maxv:
                    out.append(q)
            if inside(dcur) and len(out) < maxv:
                out.append(cur)
            prev, dprev = cur, dcur
        poly = out
        if stages is not None:
            stages.append(len(poly))
    inter = 0.0
    if len(poly) >= 3:
        total, prev = 0.0, poly[-1]
        for cur in poly:
            total = total + (prev[0] * cur[1] - prev[1] * cur[0])
            prev = cur
        inter = abs(total) / 2.0

    def ratio(i, sa, sb):
        den = (sa + sb) - i if criterion == 'iou' else (sa if criterion == 'a' else sb)
        r = i / den if den > 0.0 else 0.0
        return r if r == r else 0.0
    with np.errstate(all='ignore'):
        sa, sb = np.float64(a[2]) * a[1], np.float64(b[2]) * b[1]
        return float(ratio(np.float64(inter), sa, sb)), float(ratio(np.float64(inter) * ov, sa * a[0], sb * b[0])), len(poly)


# ------------------------------------------------------------------------------------------------ plain geometry of a pair
def in_frame_of(a, b):
    """The four corners of a in b's own frame (x along l, z along w), as Fractions of the fp64 c / s."""
    origin = (F(float(b[3])), F(float(b[5])))
    c, s = F(float(np.cos(b[6]))), F(float(np.sin(b[6])))
    return [(c * x - s * z, s * x + c * z) for x, z in _corners(a, origin)]


def clearance_ok(a, b, bar=FRAGILE):
    """Every corner of either box is at least ``bar`` away from every edge line of the other (exact)."""
    origin = (F(float(b[3])), F(float(b[5])))
    ca, cb = _corners(a, origin), _corners(b, origin)
    bar2 = F(bar) ** 2
    for pts, poly in ((ca, cb), (cb, ca)):
        for k in range(4):
            (ex, ez), (fx, fz) = poly[k], poly[(k + 1) % 4]
            dx, dz = fx - ex, fz - ez
            n2 = dx * dx + dz * dz
            for p in pts:
                side = dx * (p[1] - ez) - dz * (p[0] - ex)
                if side * side < bar2 * n2:
                    return False
    return True


def _clear_float(a, b, bar):
    """The same in fp64, for the redraw loops (with a bar well above FRAGILE)."""
    fa, fb = ref.footprint(a) - b[[3, 5]], ref.footprint(b) - b[[3, 5]]
    for pts, poly in ((fa, fb), (fb, fa)):
        d = np.roll(poly, -1, axis=0) - poly
        for k in range(4):
            side = d[k, 0] * (pts[:, 1] - poly[k, 1]) - d[k, 1] * (pts[:, 0] - poly[k, 0])
            if np.abs(side).min() < bar * np.hypot(*d[k]):
                return False
    return True


def edge_angle(a, b):
    """Exact angle (Fraction, rad) between the closest edge directions of a and b: ry_a - ry_b modulo pi / 2, folded to +-pi / 4."""
    d = F(float(a[6])) - F(float(b[6]))
    q = PI / 2
    d -= q * round(d / q)
    return abs(d)


# ------------------------------------------------------------------------------------------------ the pair set
def _draw_box(rng, lo=1.5, hi=5.0):
    return np.array([rng.uniform(1.0, 2.5), rng.uniform(lo, hi), rng.uniform(lo, hi), rng.uniform(-52, 52), rng.uniform(-2, 2),
                     rng.uniform(-52, 52), rng.uniform(-np.pi, np.pi)])


def _lattice(v):
    return np.round(np.asarray(v) / LATTICE) * LATTICE


def _redraw(rng, make, accept=lambda a, b: True):
    while True:
        a, b = make()
        if _clear_float(a, b, 1e-7) and accept(a, b):
            return a, b


def _concentric(rng, lattice=False):
    """Two rectangles of similar size near a common centre, turned by about 45 degrees: 6, 7 and 8 vertices."""
    b = _draw_box(rng, 2.0, 4.0)
    b[2] = b[1] * rng.uniform(1.0, 1.4)
    a = b.copy()
    a[0:3] *= rng.uniform(0.8, 1.25, 3)
    a[3:6] += rng.uniform(-0.25, 0.25, 3)
    a[6] = b[6] + np.pi / 4 * rng.choice([-3, -1, 1, 3]) + rng.uniform(-0.3, 0.3)
    if lattice:
        for x in (a, b):
            x[0], x[3:6] = _lattice(x[0]), _lattice(x[3:6])
    return a, b


def _general(rng):
    """Any sizes and yaws (|ry| up to 4 pi), centres a few metres apart: 0, 3, 4, 5, 6 vertices."""
    a = _draw_box(rng, 0.3, 9.0)
    b = _draw_box(rng, 0.3, 9.0)
    a[6], b[6] = rng.uniform(-4 * np.pi, 4 * np.pi, 2)
    b[3:6] = a[3:6] + rng.uniform(-3.0, 3.0, 3) * np.array([1.0, 0.4, 1.0])
    return a, b


def _poke(rng):
    """A corner of a inside b and nothing else: triangles (and the odd quadrilateral)."""
    b = _draw_box(rng, 3.0, 6.0)
    a = _draw_box(rng, 3.0, 6.0)
    a[4] = b[4] + rng.uniform(-0.5, 0.5)
    a[6] = b[6] + np.pi / 4 + rng.uniform(-0.2, 0.2)
    c, s = np.cos(b[6]), np.sin(b[6])
    reach = 0.5 * np.hypot(a[1], a[2])
    x, z = b[2] / 2 + reach * rng.uniform(0.75, 0.95), rng.uniform(-0.2, 0.2) * b[1]      # in b's frame, beyond its +x face
    if rng.integers(2):
        x = -x
    a[3], a[5] = b[3] + c * x + s * z, b[5] - s * x + c * z
    return a, b


def _beyond(rng, face):
    """a wholly beyond one face of b (in b's frame), inside the slab of the faces clipped before it."""
    b = _draw_box(rng, 2.0, 6.0)
    a = _draw_box(rng, 1.5, 5.0)
    a[4] = b[4] + rng.uniform(-0.5, 0.5)
    reach = 0.5 * np.hypot(a[1], a[2])
    far = reach + rng.uniform(0.05, 2.0)
    x, z = {'+x': (b[2] / 2 + far, rng.uniform(-3, 3)), '-x': (-b[2] / 2 - far, rng.uniform(-3, 3)),
            '+z': (rng.uniform(-0.4, 0.4) * b[2], b[1] / 2 + far), '-z': (rng.uniform(-0.4, 0.4) * b[2], -b[1] / 2 - far)}[face]
    c, s = np.cos(b[6]), np.sin(b[6])
    a[3], a[5] = b[3] + c * x + s * z, b[5] - s * x + c * z           # world offset of the local point (x, z): R = [[c, s], [-s, c]]
    return a, b


def _near_parallel(rng, eps):
    b = _draw_box(rng, 1.5, 5.0)
    a = b.copy()
    a[0:3] *= rng.uniform(0.7, 1.3, 3)
    a[3:6] += rng.uniform(-0.6, 0.6, 3) * np.array([1.0, 0.3, 1.0])
    k = int(rng.integers(-2, 3))
    if k % 2:
        a[1], a[2] = a[2], a[1]                                       # a quarter turn: keep a's extent along b's axes within 0.7 - 1.3
    a[6] = (b[6] + eps * rng.choice([-1.0, 1.0])) + k * (np.pi / 2)
    return a, b


def touching_cases():
    """Axis-aligned boxes (ry = 0: c = 1, s = 0 exactly) on the 2^-10 lattice that touch at ONE corner (n = 1) or share PART of
    an edge (n = 2): exactly zero area.  [(kind, a, b)]"""
    out = []
    u = LATTICE
    for k, (l, w, X, Z) in enumerate(((4.0, 2.0, 3.0, 17.0), (3.0 + 5 * u, 1.5, -40.0 + 3 * u, 9.0 - 7 * u), (0.5, 6.0 + 2 * u, 61.0, -50.0 + u))):
        base = np.array([1.5, w, l, X, 1.0, Z, 0.0])
        other = np.array([2.0, _lattice(w * 0.5 + 1.0), _lattice(l * 0.25 + 2.0), 0.0, 1.25, 0.0, -0.0])
        for sx, sz in ((1, 1), (1, -1), (-1, 1), (-1, -1))[k:k + 2]:
            b = other.copy()
            b[3], b[5] = X + sx * (l + b[2]) / 2, Z + sz * (w + b[1]) / 2
            out.append(('corner', base, b))
        for sx, sz, slide in ((1, 0, 0.25), (-1, 0, -0.5), (0, 1, 0.75), (0, -1, -0.25))[k:k + 2]:
            b = other.copy()
            b[3] = X + sx * (l + b[2]) / 2 + (slide if sz else 0.0)
            b[5] = Z + sz * (w + b[1]) / 2 + (slide if sx else 0.0)
            out.append(('edge', base, b))
    return out


POOLS = (('concentric', 150), ('lattice', 96), ('general', 240), ('poke', 40), ('beyond+x', 12), ('beyond-x', 12), ('beyond+z', 12),
         ('beyond-z', 12)) + tuple(('near%g' % e, 20) for e in NEAR_ANGLES)


@functools.lru_cache(maxsize=None)
def pair_set():
    """dict(a, b: (n, 7) float64; pool: n names; want_bev / want_vol: closed forms of the degenerate classes (NaN elsewhere)).
    Seeded; the random pools are redrawn pair by pair until no corner is fragile - nothing is left out afterwards."""
    rng = np.random.Generator(np.random.PCG64(2024))
    A, Bx, pool, wb, wv = [], [], [], [], []

    def add(name, a, b, bev=np.nan, vol=np.nan):
        A.append(np.array(a, np.float64)), Bx.append(np.array(b, np.float64)), pool.append(name), wb.append(bev), wv.append(vol)
    for name, count in POOLS:
        for _ in range(count):
            if name == 'concentric':
                a, b = _redraw(rng, lambda: _concentric(rng))
            elif name == 'lattice':
                a, b = _redraw(rng, lambda: _concentric(rng, True))
            elif name == 'general':
                a, b = _redraw(rng, lambda: _general(rng))
            elif name == 'poke':
                a, b = _redraw(rng, lambda: _poke(rng))
            elif name.startswith('beyond'):
                a, b = _redraw(rng, lambda: _beyond(rng, name[6:]))
            else:
                eps = float(name[4:])
                a, b = _redraw(rng, lambda: _near_parallel(rng, eps), lambda a, b: ref.overlap(a, b)[0] > 0.05 and eps / 2 <= edge_angle(a, b) <= 2 * eps)
            add(name, a, b)
    for kind, a, b in touching_cases():
        add('touch_' + kind, a, b, 0.0, 0.0)
    for _, a, b, bev, vol in cases.degenerate_cases():
        add('closed_form', a, b, bev, vol)
    out = dict(a=np.stack(A), b=np.stack(Bx), pool=np.array(pool), want_bev=np.array(wb), want_vol=np.array(wv))
    for v in out.values():
        v.setflags(write=False)
    return out


RANDOM_POOLS = tuple(n for n, _ in POOLS)


@functools.lru_cache(maxsize=None)
def yardstick():
    """The exact yardstick over pair_set(), computed once: dict(exact: {criterion: (n, 2)}, nv, new: (n,) vertex counts,
    float: {criterion: (n, 2)} of box_overlap_ref.overlap, yard_err: the largest |float - exact| over the set)."""
    ps = pair_set()
    n = len(ps['a'])
    geom = [exact_pair(ps['a'][k], ps['b'][k]) for k in range(n)]
    exact = {c: np.array([ratios(geom[k], ps['a'][k], ps['b'][k], c) for k in range(n)]) for c in CRITERIA}
    flt = {c: np.array([ref.overlap(ps['a'][k], ps['b'][k], c) for k in range(n)]) for c in CRITERIA}
    out = dict(exact=exact, float=flt, nv=np.array([g[4] for g in geom]), new=np.array([g[5] for g in geom]),
               yard_err=max(float(np.abs(flt[c] - exact[c]).max()) for c in CRITERIA))
    for v in (out['nv'], out['new'], *exact.values(), *flt.values()):
        v.setflags(write=False)
    return out


def bar():
    """Device against exact: 16 x the float yardstick's own error (another operation order, sin / cos an ulp from numpy's), with
    the floor 16 x 7e-15 (an fp64 restatement of box_geom.h against the exact yardstick)."""
    return max(16 * yardstick()['yard_err'], 1e-13)


_exact_cache = {}


def exact_cached(a, b):
    key = np.asarray(a, np.float64).tobytes() + np.asarray(b, np.float64).tobytes()
    if key not in _exact_cache:
        _exact_cache[key] = exact_pair(a, b)
    return _exact_cache[key]


LAYOUTS = ((3, 5, 13), (3, 13, 5), (1, 15, 39), (5, 6, 10), (4, 12, 16))      # 195, 195 (a and b swapped), 585, 300, 768 pairs
LAYOUT_COUNTS = {(3, 5, 13): ((5, 0, 3), (13, 13, 0)), (3, 13, 5): ((13, 13, 0), (5, 0, 3)), (1, 15, 39): ((15,), (38,)),
                 (5, 6, 10): ((6, 0, 6, 1, 3), (10, 10, 0, 7, 1)), (4, 12, 16): ((12, 0, 5, 12), (16, 16, 9, 0))}        # ragged: 0, the full count, between


@functools.lru_cache(maxsize=None)
def layout_boxes():
    """Three sites, far from each other; 5 boxes P and 13 boxes Q around each, sizes and yaws drawn so that most P x Q pairs of a
    site overlap with polygons of every vertex count.  Returns (P (3, 5, 7), Q (3, 13, 7))."""
    rng = np.random.Generator(np.random.PCG64(77))
    P, Q = np.empty((3, 5, 7)), np.empty((3, 13, 7))
    for m, (X, Z) in enumerate(((-40.0, 10.0), (5.0, 50.0), (45.0, -30.0))):
        for arr in (P, Q):
            for k in range(arr.shape[1]):
                while True:
                    box = np.array([rng.uniform(1.0, 2.5), rng.uniform(2.0, 4.0), rng.uniform(2.0, 5.0), X + rng.uniform(-1, 1), rng.uniform(-1, 1),
                                    Z + rng.uniform(-1, 1), rng.uniform(-np.pi, np.pi)])
                    others = list(P[m]) if arr is Q else []
                    if all(_clear_float(box, o, 1e-7) for o in others):
                        break
                arr[m, k] = box
    P.setflags(write=False), Q.setflags(write=False)
    return P, Q


def layout(B, ca, cb):
    """(A (B, ca, 7), Bx (B, cb, 7), na, nb) of one layout, all from layout_boxes(): (3, 5, 13) is P against Q, (3, 13, 5) Q
    against P, (1, 15, 39) all P against all Q (pairs across sites are disjoint), the others cycle through P and Q of a site."""
    P, Q = layout_boxes()
    if (B, ca, cb) == (3, 5, 13):
        A, Bx = P.copy(), Q.copy()
    elif (B, ca, cb) == (3, 13, 5):
        A, Bx = Q.copy(), P.copy()
    elif B == 1:
        A, Bx = P.reshape(1, 15, 7).copy(), Q.reshape(1, 39, 7).copy()
    else:
        A = np.stack([np.stack([(P[m % 3] if i % 2 else Q[m % 3])[(i * 3 + m) % (5 if i % 2 else 13)] for i in range(ca)]) for m in range(B)])
        Bx = np.stack([np.stack([(Q[m % 3] if j % 3 else P[m % 3])[(j * 5 + m) % (13 if j % 3 else 5)] for j in range(cb)]) for m in range(B)])
    na, nb = LAYOUT_COUNTS[(B, ca, cb)]
    return A, Bx, np.array(na, np.int32), np.array(nb, np.int32)


def extreme_boxes():
    """(n, 7) boxes for an n x n launch: sizes of 1e200 (footprint areas overflow), |ry| up to 1e6, the project's invalid boxes
    among ordinary ones.  Returns (boxes, invalid mask)."""
    ok, bad = cases.invalid_boxes()
    rng = np.random.Generator(np.random.PCG64(5))
    rows = [ok]
    for k in range(6):                                   # ordinary boxes around ok, huge yaws
        b = ok.copy()
        b[0:3] *= rng.uniform(0.7, 1.3, 3)
        b[3:6] += rng.uniform(-1, 1, 3)
        b[6] = rng.uniform(-1e6, 1e6) if k else 1e6
        rows.append(b)
    for k, ry in enumerate((0.0, 0.3, np.pi / 4, -1e6, 2.0, 1e5)):       # huge boxes: about the same centre, and far away
        b = np.array([1e200, 1e200, 1e200, 3.0, 1.0, 17.0, ry])
        if k >= 3:
            b[0:3] = (1e200, 3e199, 7e200)
        if k == 4:
            b[3], b[5] = 4e199, -1e200
        if k == 5:
            b[0] = 2.0                                   # only the footprint overflows
        rows.append(b)
    rows += list(bad)
    rows.append(np.array([1e-200, 1e-200, 1e-200, 3.0, 1.0, 17.0, 0.5]))   # footprint area underflows to 0: a valid box of no size
    boxes = np.stack(rows)
    invalid = np.array([not ref.valid(b) for b in boxes])
    return boxes, invalid


# ------------------------------------------------------------------------------------------------ NMS: host model
NMS_VARIANTS = ('no_half_round', 'no_wrap', 'rows4', 'non_survivors', 'ge', 'swapped')


def visits(nc, variant=None):
    """The (lo, hi) candidate pairs records_nms3d_kernel visits, in order of p."""
    rounds = nc >> 1
    out = []
    for p in range(rounds * nc):
        d = p // nc + 1
        i = p - (d - 1) * nc
        if nc % 2 == 0 and d == rounds and (i >= rounds or variant == 'no_half_round'):
            continue
        j = i + d
        if j >= nc:
            if variant == 'no_wrap':
                continue
            j -= nc
        out.append((min(i, j), max(i, j)))
    return out


def model_nms(rec, thresh, iou, class_aware=False, variant=None):
    """Host model of records_nms3d_kernel on one image's (topk, 32) records: compaction of the slots whose flag is exactly 2,
    the round-robin pair schedule, the bit rows over[later] |= 1 << earlier (8 words of 32 bits), the walk over the candidates
    with the kept set.  ``iou``: {(earlier slot, later slot): IoU}, 0 for every pair that is not in it.  Returns the flags."""
    rec = np.asarray(rec)
    flags = rec[:, 31].copy()
    slots = [k for k in range(rec.shape[0]) if rec[k, 31] == np.float32(2.0)]
    nc = len(slots)
    words = 4 if variant == 'rows4' else 8
    over = [0] * nc
    for lo, hi in visits(nc, variant):
        if class_aware and not rec[slots[lo], 0] == rec[slots[hi], 0]:
            continue
        v = iou.get((slots[lo], slots[hi]), 0.0)
        if (v >= thresh) if variant == 'ge' else (v > thresh):
            row, bit = (lo, hi) if variant == 'swapped' else (hi, lo)
            if bit >> 5 < words:
                over[row] |= 1 << bit
    keep = 0
    for k in range(nc):
        if not (over[k] if variant == 'non_survivors' else over[k] & keep):
            keep |= 1 << k
    for k in range(nc):
        if not (keep >> k) & 1:
            flags[slots[k]] = 1.0
    return flags


def strict_pair(rec, M, usual):
    """(i, j): slot i goes at the threshold ``usual`` because of the surviving earlier slot j, stays when the threshold is exactly
    M[j, i] and goes again at the float just under it (M: IoUs of one image, earlier slot first)."""
    base = ref.nms_flags(rec, usual, M)
    kept = np.flatnonzero(base == 2)
    for i in np.flatnonzero((rec[:, 31] == 2) & (base == 1)):
        before = kept[kept < i]
        j = int(before[np.argmax(M[before, i])])
        at, under = ref.nms_flags(rec, float(M[j, i]), M), ref.nms_flags(rec, float(np.nextafter(M[j, i], 0.0)), M)
        if M[j, i] > usual and at[i] == 2 and under[i] == 1 and at[j] == under[j] == 2:
            return int(i), j
    raise AssertionError('no pair whose own IoU decides a slot')


# ------------------------------------------------------------------------------------------------ NMS: constructed cases
def _noise(seed, B, topk):
    rng = np.random.Generator(np.random.PCG64(seed))
    rec = rng.standard_normal((B, topk, 32)).astype(np.float32)
    rec[..., 0] = 0.0
    return rec, rng


def _site(k, ry=0.0, dy=0.0):
    """The NMS box of lattice site k (a 16 x 16 grid): every value exact in fp32."""
    return np.array(NMS_BOX + ((k % 16) * PITCH - 60.0, 1.0 + dy, (k // 16) * PITCH + 6.0, ry), np.float32)


def one_factorisation(nc):
    """Rounds of the circle method on nc candidates: every pair (i < j) exactly once over the rounds; nc - 1 rounds of nc / 2
    pairs for an even count, nc rounds of (nc - 1) / 2 pairs and one bye for an odd one."""
    n = nc + (nc & 1)
    rounds = []
    for m in range(n - 1):
        pairs = [(n - 1, m)] + [((m + k) % (n - 1), (m - k) % (n - 1)) for k in range(1, n // 2)]
        rounds.append(sorted((min(p), max(p)) for p in pairs if max(p) < nc))
    return rounds


def _case(name, rec, thresh=0.5, metric='bev', aware=False, ious=None, want=None, **more):
    B = rec.shape[0]
    ious = ious if ious is not None else [{} for _ in range(B)]
    if want is None:
        want = np.stack([model_nms(rec[b], thresh, ious[b], aware) for b in range(B)])
    c = dict(name=name, rec=rec, thresh=thresh, metric=metric, aware=aware, ious=ious, want=want, **more)
    rec.setflags(write=False), want.setflags(write=False)
    return c


def every_pair_case(nc, metric):
    """Image m plants round m of the 1-factorisation: the later box of each pair is a copy of the earlier one.  topk = nc, every
    slot a candidate; the expected flags are written from the construction (the later slot of each planted pair goes)."""
    rounds = one_factorisation(nc)
    rec, rng = _noise(1000 + nc, len(rounds), nc)
    want = np.full((len(rounds), nc), 2.0, np.float32)
    ious = []
    for m, pairs in enumerate(rounds):
        ry = rng.uniform(-np.pi, np.pi, nc).astype(np.float32)
        for k in range(nc):
            rec[m, k, 24:31] = _site(k, ry[k])
        for i, j in pairs:
            rec[m, j, 24:31] = rec[m, i, 24:31]
            want[m, j] = 1.0
        ious.append({p: 1.0 for p in pairs})
    rec[..., 31] = 2.0
    return _case('every_pair_nc%d_%s' % (nc, metric), rec, 0.5, metric, False, ious, want, nc=nc, rounds=rounds)


def _line_iou(d, delta):
    gap = d * delta
    return (4.0 - gap) / (4.0 + gap) if gap < 4.0 else 0.0


def line_case(delta, interleaved, metric='bev'):
    """A line of equal axis-aligned boxes of length 4 stepped by delta along their own axis; 256 candidates in 256 slots, or 128
    candidates interleaved among flag-0 and flag-1 slots of topk = 256 (candidate number != slot)."""
    rec, rng = _noise(int(delta * 10) + 2 * interleaved, 1, 256)
    if interleaved:
        slots = sorted(rng.permutation(256)[:128].tolist())
        rec[0, :, 31] = rng.integers(0, 2, 256).astype(np.float32)
        for k in range(256):                                       # the slots between hold copies of candidate boxes: no candidates
            rec[0, k, 24:31] = (1.5, 2.0, 4.0, np.float32(delta * (k % 7)), 1.0, 10.0, 0.0)
    else:
        slots = list(range(256))
    for n, k in enumerate(slots):
        rec[0, k, 24:31] = (1.5, 2.0, 4.0, np.float32(delta * n), 1.0, 10.0, 0.0)
        rec[0, k, 31] = 2.0
    iou = {(slots[i], slots[j]): _line_iou(j - i, delta) for i in range(len(slots)) for j in range(i + 1, min(i + 8, len(slots)))}
    period = 2 if delta == 1.0 else 3
    want = rec[0, :, 31].copy()
    for n, k in enumerate(slots):
        want[k] = 2.0 if n % period == 0 else 1.0
    return _case('line_d%g_%s_%s' % (delta, 'interleaved' if interleaved else 'full', metric), rec, 0.5, metric, False, [iou], want[None],
                 slots=slots, period=period)


COUNT_NC = (0, 1, 2, 3, 63, 64, 65, 128, 255, 256)
COUNT_TOPK = (1, 63, 64, 65, 255, 256)
NOT_CANDIDATE = (np.float32(2.0000002), np.float32(3.0), np.float32(np.nan), np.float32(-2.0), np.float32(0.0), np.float32(1.0))


def counts_case(topk):
    """One launch per topk: an image for every nc of COUNT_NC that fits, candidates spread over the slots, every third candidate
    a copy of the one before; the other slots hold flags that are no candidates (2.0000002, 3, NaN, -2, 0, 1) and copies of
    candidate boxes.  topk = 256 adds an image whose candidates all sit in the last wave of slots (192 ..)."""
    ncs = [nc for nc in COUNT_NC if nc <= topk]
    spreads = [(nc, 0) for nc in ncs] + ([(40, 192), (64, 192)] if topk == 256 else [])
    rec, rng = _noise(3000 + topk, len(spreads), topk)
    want = np.empty((len(spreads), topk), np.float32)
    ious = []
    for m, (nc, first) in enumerate(spreads):
        slots = sorted((first + rng.permutation(topk - first)[:nc]).tolist())
        for k in range(topk):
            rec[m, k, 24:31] = _site(int(rng.integers(256)))
            rec[m, k, 31] = NOT_CANDIDATE[int(rng.integers(len(NOT_CANDIDATE)))]
        want[m] = rec[m, :, 31]
        site = rng.permutation(256)
        iou = {}
        for n, k in enumerate(slots):
            dup = n % 3 == 1
            rec[m, k, 24:31] = _site(int(site[n - 1 if dup else n]))
            rec[m, k, 31] = 2.0
            want[m, k] = 1.0 if dup else 2.0
            if dup:
                iou[(slots[n - 1], k)] = 1.0
        ious.append(iou)
    return _case('counts_topk%d' % topk, rec, 0.5, 'bev', False, ious, want, spreads=spreads)


def threshold_images():
    """(1, 24, 32) records: pairs of equal axis-aligned boxes at lattice sites - identical, sharing an edge (IoU exactly 0),
    overlapping by 2^-10 m, half overlapping - then two invalid candidates and a lone one; classes 0 / 1 alternate by pair."""
    rec, _ = _noise(41, 1, 24)
    rec[0, :, 31] = 0.0
    shifts = (0.0, 4.0, 4.0 - LATTICE, 2.0)
    iou = {}
    for p, dx in enumerate(shifts):
        for q in range(2):
            k = 2 * p + q
            rec[0, k, 24:31] = _site(2 * p)
            rec[0, k, 27] += np.float32(dx * q)
            rec[0, k, 0] = float(p % 2)
            rec[0, k, 31] = 2.0
        iou[(2 * p, 2 * p + 1)] = _line_iou(1, dx) if dx < 4.0 else 0.0
    rec[0, 8, 24:31], rec[0, 9, 24:31], rec[0, 10, 24:31] = _site(8), _site(9), _site(10)
    rec[0, 8, 25], rec[0, 9, 27] = 0.0, np.nan                        # w = 0; a NaN centre
    rec[0, 8:11, 31] = 2.0
    rec[0, 8:11, 0] = (0.0, 1.0, 1.0)
    return rec, iou


def threshold_case(thresh, aware):
    rec, iou = threshold_images()
    return _case('thresh_%g_%s' % (thresh, 'aware' if aware else 'blind'), rec, thresh, 'bev', aware, [iou])


def odd_case(metric, thresh, aware):
    """Flag-2 slots whose boxes are NaN, infinite or of zero size, each a copy of / copied by a valid candidate at the same site;
    two identical boxes of NaN class; two boxes of equal footprint and disjoint vertical extents."""
    rec, _ = _noise(43, 1, 20)
    rec[0, :, 31] = 2.0
    iou = {}
    for p, (idx, v) in enumerate(((24, np.nan), (26, np.inf), (25, 0.0), (30, np.inf), (24, -1.0), (28, np.nan))):
        for q in range(3):                                            # valid, invalid, valid at one site
            rec[0, 3 * p + q, 24:31] = _site(p)
        rec[0, 3 * p + 1, idx] = v
        iou[(3 * p, 3 * p + 2)] = 1.0
    rec[0, 18, 24:31] = rec[0, 19, 24:31] = _site(40)
    rec[0, 19, 28] += 1.5                                             # h = 1.5: the vertical extents touch, footprints equal
    iou[(18, 19)] = 1.0 if metric == 'bev' else 0.0
    if aware:
        rec[0, 0, 0] = rec[0, 2, 0] = np.nan                          # NaN equals nothing: neither suppresses the other
    return _case('odd_%s_%g_%s' % (metric, thresh, 'aware' if aware else 'blind'), rec, thresh, metric, aware, [iou])


EVEN_NC, ODD_NC = (2, 4, 8, 64, 256), (3, 7, 65, 255)


@functools.lru_cache(maxsize=None)
def nms_case(name):
    return NMS_CASES[name]()


NMS_CASES = {}
for _nc in EVEN_NC + ODD_NC:
    for _metric in ('bev', '3d'):
        NMS_CASES['every_pair_nc%d_%s' % (_nc, _metric)] = functools.partial(every_pair_case, _nc, _metric)
for _delta in (1.0, 0.6):
    for _inter in (False, True):
        NMS_CASES['line_d%g_%s_bev' % (_delta, 'interleaved' if _inter else 'full')] = functools.partial(line_case, _delta, _inter)
NMS_CASES['line_d1_full_3d'] = functools.partial(line_case, 1.0, False, '3d')
for _topk in COUNT_TOPK:
    NMS_CASES['counts_topk%d' % _topk] = functools.partial(counts_case, _topk)
for _thr in (0.0, 1.5, -1.0, float('inf')):
    for _aware in (False, True):
        NMS_CASES['thresh_%g_%s' % (_thr, 'aware' if _aware else 'blind')] = functools.partial(threshold_case, _thr, _aware)
for _metric, _thr, _aware in (('bev', 0.0, False), ('bev', 0.5, True), ('3d', 0.0, False), ('3d', 0.5, False)):
    NMS_CASES['odd_%s_%g_%s' % (_metric, _thr, 'aware' if _aware else 'blind')] = functools.partial(odd_case, _metric, _thr, _aware)
NMS_NAMES = tuple(NMS_CASES)
