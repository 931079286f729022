"""Inputs of the box-overlap tests (seeded, host only): the closed-form degenerate pairs, the random ragged pair set and
the detection records of the NMS tests.  Shared by tests/test_box_overlap_cpu.py (which checks the yardstick and the
conditions the inputs must meet) and tests/test_gpu_box_overlap.py."""
import numpy as np

from tests import box_overlap_ref as ref

MIN_EDGE_ANGLE = 1e-3          # rad: within a random pair no two edges are closer to parallel than this
IOU_GAP = 1e-6                 # no pairwise IoU of the NMS inputs lies this close to the threshold
NMS_THRESH = {'bev': 0.5, '3d': 0.4}
NMS_SHAPES = (100, 7, 130)     # the shipped topk; less than a wave; slots past 128.  In CANDIDATES (the bit rows are indexed by
#                                candidate number, not slot) these reach 66 / 66, 6 / 0 and 78 / 84 per image: no candidate >= 84, words
#                                3 .. 7 of a bit row never set.  tests/box_overlap_regimes.py holds the cases up to 256 candidates.


def _shift(box, dx_local, dz_local, dy=0.0):
    """box moved by (dx, dz) along its OWN axes (and dy vertically)."""
    h, w, l, X, Y, Z, ry = box
    c, s = np.cos(ry), np.sin(ry)
    return np.array([h, w, l, X + c * dx_local + s * dz_local, Y + dy, Z - s * dx_local + c * dz_local, ry])


def degenerate_cases():
    """[(name, a, b, expected BEV IoU, expected 3D IoU)] - exactly parallel edges on purpose, values from closed forms."""
    out = []
    for ry in (0.0, 0.3, -2.1):
        base = np.array([1.5, 2.0, 4.0, 3.0, 1.0, 17.0, ry])
        small = base * np.array([0.5, 0.5, 0.25, 1, 1, 1, 1])
        out += [
            ('identical ry=%g' % ry, base, base.copy(), 1.0, 1.0),
            ('turned by pi ry=%g' % ry, base, base + np.array([0, 0, 0, 0, 0, 0, np.pi]), 1.0, 1.0),
            ('half a length along its axis ry=%g' % ry, base, _shift(base, 2.0, 0.0), 1.0 / 3.0, 1.0 / 3.0),
            ('nested ry=%g' % ry, small, base, (1.0 * 1.0) / (4.0 * 2.0), (1.0 * 1.0 * 0.75) / (4.0 * 2.0 * 1.5)),
            ('shared edge ry=%g' % ry, base, _shift(base, 4.0, 0.0), 0.0, 0.0),
            ('shared corner ry=%g' % ry, base, _shift(base, 4.0, 2.0), 0.0, 0.0),
            ('disjoint ry=%g' % ry, base, _shift(base, 9.0, -5.0), 0.0, 0.0),
            ('half vertical overlap ry=%g' % ry, base, _shift(base, 0.0, 0.0, 0.75), 1.0, 1.0 / 3.0),
        ]
    return out


def invalid_boxes():
    """Boxes that overlap nothing: w = 0, a NaN centre, l = -1 (and an infinite yaw, a zero height)."""
    ok = np.array([1.5, 2.0, 4.0, 3.0, 1.0, 17.0, 0.3])
    bad = []
    for idx, v in ((1, 0.0), (3, np.nan), (2, -1.0), (6, np.inf), (0, 0.0)):
        b = ok.copy()
        b[idx] = v
        bad.append(b)
    return ok, np.array(bad)


def random_pairs(seed=20, B=3, cap=17, na=(17, 0, 5), nb=(17, 4, 0)):
    """Ragged random boxes: centres within +-40 m, sizes 0.3 - 12 m, any ry in [-4 pi, 4 pi]; half of b's boxes lie near one of
    a's so that a good share of the pairs overlaps.  Redrawn until within every counted pair no two edges are closer to
    parallel than MIN_EDGE_ANGLE.  Entries beyond the counts hold boxes too (they must be ignored)."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def draw(n):
        b = np.empty((n, 7))
        b[:, 0:3] = rng.uniform(0.3, 12.0, (n, 3))
        b[:, 3:6] = rng.uniform(-40.0, 40.0, (n, 3))
        b[:, 4] = rng.uniform(-3.0, 3.0, n)
        b[:, 6] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
        return b
    A = np.stack([draw(cap) for _ in range(B)])
    Bx = np.stack([draw(cap) for _ in range(B)])
    for m in range(B):
        for j in range(0, cap, 2):
            Bx[m, j, 3:6] = np.clip(A[m, j, 3:6] + rng.uniform(-3.0, 3.0, 3), -40.0, 40.0)
        for j in range(cap):
            while min(ref.min_edge_angle(A[m, i], Bx[m, j]) for i in range(cap)) < MIN_EDGE_ANGLE:
                Bx[m, j, 6] = rng.uniform(-4 * np.pi, 4 * np.pi)
    return A, Bx, np.array(na, np.int32), np.array(nb, np.int32)


def nms_records(topk, seed=7, B=2):
    """(B, topk, 32) fp32 records built on the host: clusters of near-duplicate boxes around well separated sites, one pair of
    different classes at the same place per populated image, flag-0 and flag-1 slots interleaved with the flag-2 ones, the
    other fields arbitrary; with topk < 64 the last image has no flag-2 slot at all."""
    rng = np.random.Generator(np.random.PCG64(seed + topk))
    rec = rng.standard_normal((B, topk, 32)).astype(np.float32)
    nsite = max(2, topk // 6)
    for b in range(B):
        sites = np.empty((nsite, 7))
        sites[:, 0] = rng.uniform(1.4, 2.0, nsite)
        sites[:, 1] = rng.uniform(1.5, 2.1, nsite)
        sites[:, 2] = rng.uniform(3.2, 4.8, nsite)
        sites[:, 3] = (np.arange(nsite) % 6) * 9.0 - 22.0
        sites[:, 4] = rng.uniform(0.8, 1.2, nsite)
        sites[:, 5] = (np.arange(nsite) // 6) * 9.0 + 8.0
        sites[:, 6] = rng.uniform(-np.pi, np.pi, nsite)
        for k in range(topk):
            s = sites[rng.integers(nsite)]
            box = s.copy()
            box[0:3] *= rng.uniform(0.85, 1.15, 3)
            box[3:6] += rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 0.3, 1.0]) * rng.choice([0.15, 1.0])
            box[6] += rng.uniform(-0.3, 0.3)
            rec[b, k, 24:31] = box.astype(np.float32)
            rec[b, k, 0] = float(rng.integers(3))
            rec[b, k, 31] = float(rng.choice([0, 1, 2, 2, 2, 2]))
        rec[b, :, 1] = np.sort(rng.uniform(0.4, 0.99, topk).astype(np.float32))[::-1]
        # two flag-2 slots of different classes at the same place (the Pedestrian / Cyclist pair)
        i, j = topk // 3, topk // 3 + 2
        rec[b, i, 27], rec[b, i, 29] = 35.0, 70.0                     # a site of their own: only the two meet
        rec[b, j, 24:31] = rec[b, i, 24:31]
        rec[b, i, 0], rec[b, j, 0] = 1.0, 2.0
        rec[b, i, 31] = rec[b, j, 31] = 2.0
    if topk < 64:
        rec[B - 1, :, 31] = np.where(rec[B - 1, :, 31] == 2, 1, rec[B - 1, :, 31])
    return rec
