"""Generated multi-camera records for the rig-fusion tests (seeded, nothing from outside): objects placed in the rig frame, seen
by some of the rig's cameras with a little noise, each view written into that camera's (topk, 32) fp32 records in the camera's
own coordinates.  Between them the cases hold: yaw-only extrinsics and extrinsics with pitch and roll, all three metrics, both
merges, class_aware and cross_only on and off, exactly equal scores across cameras, junk slots (flag 0, flag 1 carrying a box,
flag 2 below min_score, flag 2 with a NaN score), a camera and a rig without a detection, twins seen from opposite ends, the
A-B-C chain, two boxes of one camera joining a representative of another, a box that is not finite, and more clusters than cap.
``cases()`` returns the table; a case is reseeded until the yardstick's own decision margin is >= MARGIN, so that no near-tie
lets two correct implementations differ.  ``reference(case)`` is the yardstick's result, computed once per process."""
import numpy as np

from tests import rig_ref as ref

MARGIN = 1e-6
MIN_SCORE = 0.3
_cache = {}


def ext_matrix(yaw, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """(3, 4) [R | t], camera -> rig: yaw about y, pitch about x, roll about z, R = R_yaw R_pitch R_roll."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    Rp = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], np.float64)
    Rr = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]], np.float64)
    return np.concatenate([Ry @ Rp @ Rr, np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def to_camera(pos, ry, E):
    """A rig-frame centre and heading in the coordinates of the camera with extrinsic E (3, 4)."""
    R, t = E[:, :3], E[:, 3]
    p = R.T @ (np.asarray(pos, np.float64) - t)
    h = R.T @ np.array([np.cos(ry), 0.0, -np.sin(ry)])
    return p, np.arctan2(-h[2], h[0])


def obj(pos, views, rng, cls=0, ry=None, dims=None, flips=(), noise=0.03):
    """views: {camera: score}; flips: the cameras that report the heading from the other end."""
    return dict(pos=np.asarray(pos, np.float64), views=dict(views), cls=cls, ry=rng.uniform(-3.1, 3.1) if ry is None else ry,
                dims=rng.uniform(0.9, 1.1, 3) * np.array([1.6, 1.8, 4.0]) if dims is None else np.asarray(dims, np.float64),
                flips=set(flips), noise=noise)


def site(i, rng, spacing=9.0, per_row=8):
    """Grid site i in the rig frame, spacing metres apart (a car's footprint diagonal is 4.4 m: neighbours never touch)."""
    return np.array([(i % per_row - per_row / 2) * spacing, 1.0, (i // per_row) * spacing + 6.0]) + rng.uniform(-0.5, 0.5, 3) * np.array([1, 0.1, 1])


def render(objs, ext, topk, rng, junk=True):
    """(C, topk, 32) records of one rig."""
    C = ext.shape[0]
    out = np.zeros((C, topk, 32), np.float32)
    for c in range(C):
        rows = []
        for o in objs:
            if c not in o['views']:
                continue
            p, ry = to_camera(o['pos'], o['ry'], ext[c])
            r = np.zeros(32)
            r[0], r[1] = o['cls'], o['views'][c]
            r[2:24] = rng.uniform(0, 300, 22)
            r[24:27] = o['dims'] + rng.normal(0, 0.01, 3) * (o['noise'] > 0)
            r[27:30] = p + rng.normal(0, 1.0, 3) * o['noise']
            r[30] = ry + rng.normal(0, 0.6) * o['noise'] + (np.pi if c in o['flips'] else 0.0)
            if 'raw' in o:
                r[24:31] = o['raw']
            r[31] = 2
            rows.append(r)
        rows.sort(key=lambda r: -r[1])
        rows = rows[:topk]
        slots, j = [], 0
        for n, r in enumerate(rows):
            room = topk - len(slots) - (len(rows) - n)
            if junk and n % 3 == 1 and room > 0:
                bad = r.copy()
                kind = j % 4
                j += 1
                if kind == 0:
                    bad[31] = 1                                  # a 2D-only slot carrying a box
                elif kind == 1:
                    bad[:] = 0                                   # an empty slot
                elif kind == 2:
                    bad[1] = MIN_SCORE * 0.5                     # a kept slot below min_score
                else:
                    bad[1] = np.nan                              # a kept slot whose score is not a number
                slots.append(bad)
            slots.append(r)
        if slots:
            out[c, :len(slots)] = np.array(slots, np.float32).reshape(-1, 32)
    return out


def ring(C, rng, tilt=False):
    """C cameras looking outwards, 360 / C degrees apart, 1 m off the rig's centre."""
    ext = []
    for c in range(C):
        yaw = 2.0 * np.pi * c / C
        t = (np.sin(yaw), -0.2 * (c % 2), np.cos(yaw))
        ext.append(ext_matrix(yaw, rng.uniform(-0.1, 0.1) if tilt else 0.0, rng.uniform(-0.05, 0.05) if tilt else 0.0, t))
    return np.stack(ext)


def scores(rng, n):
    return list(np.round(rng.uniform(0.35, 0.99, n), 4))


def build(name, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = dict(name=name, seed=seed, R=1, cap=None)
    if name == 'one_camera_passthrough':
        # C = 1, topk = 4: nothing can link under cross_only, the output is the kept slots in order (identity extrinsic, best)
        c.update(C=1, topk=4, params=ref.params(metric='bev', merge='best', min_score=MIN_SCORE))
        ext = np.stack([ext_matrix(0.0)])[None]
        objs = [[obj(site(i, rng), {0: s}, rng) for i, s in enumerate([0.9, 0.8, 0.7])]]
    elif name == 'two_cameras_ties_and_flip':
        # C = 2, topk = 8, yaw only: twins with exactly equal scores (camera 0 is the representative), two unrelated objects with
        # equal scores in different cameras, twins seen from opposite ends (the heading fold of the mean)
        c.update(C=2, topk=8, params=ref.params(metric='bev', thresh=0.1, merge='mean', min_score=MIN_SCORE))
        ext = np.stack([ext_matrix(0.3, t=(0.5, 0.0, 0.2)), ext_matrix(-0.4, t=(-0.5, 0.0, 0.1))])[None]
        objs = [[obj(site(0, rng), {0: 0.85, 1: 0.85}, rng), obj(site(1, rng), {0: 0.8}, rng), obj(site(2, rng), {1: 0.8}, rng),
                 obj(site(3, rng), {0: 0.6, 1: 0.7}, rng, flips={0}), obj(site(4, rng), {1: 0.95, 0: 0.5}, rng),
                 obj(site(5, rng), {0: 0.45}, rng, cls=1)]]
    elif name == 'three_cameras_chain_dist':
        # C = 3, topk = 7 (N = 21), pitch and roll, centre distance, class blind: the chain A - B - C (A-B and B-C within 1.5 m, A-C
        # not: C is its own representative), two boxes of camera 0 joining a representative of camera 1, a box that is not finite
        c.update(C=3, topk=7, params=ref.params(metric='dist', thresh=-1.5, class_aware=False, merge='mean', min_score=MIN_SCORE))
        ext = np.stack([ext_matrix(0.1, 0.05, -0.03, (0.3, 0.0, 0.0)), ext_matrix(-0.7, -0.08, 0.02, (-0.4, 0.1, 0.2)),
                        ext_matrix(0.9, 0.03, 0.04, (0.0, -0.1, -0.3))])[None]
        z = 30.0
        objs = [[obj((0.0, 1.0, z), {0: 0.90}, rng, noise=0), obj((1.0, 1.0, z), {1: 0.88}, rng, cls=1, noise=0), obj((2.0, 1.0, z), {2: 0.86}, rng, noise=0),
                 obj((15.0, 1.0, z), {1: 0.84}, rng, noise=0), obj((14.2, 1.0, z), {0: 0.82}, rng, noise=0), obj((15.9, 1.0, z), {0: 0.80}, rng, noise=0),
                 obj((-15.0, 1.0, z), {2: 0.7, 1: 0.6}, rng), obj((-25.0, 1.0, z), {0: 0.5}, rng)]]
        bad = obj((-15.2, 1.0, z), {0: 0.75}, rng)
        bad['raw'] = np.array([1.5, 1.7, 4.0, np.inf, 1.0, 20.0, 0.3])
        objs[0].append(bad)
    elif name == 'six_cameras_two_rigs':
        # C = 6, topk = 100, R = 2 (N = 600: three 256-lane passes over the slots, ten 64-bit mask words), 3D IoU, two classes
        c.update(R=2, C=6, topk=100, params=ref.params(metric='iou3d', thresh=0.05, merge='mean', min_score=MIN_SCORE))
        ext = np.stack([ring(6, rng), ring(6, rng)])
        objs = []
        for r in range(2):
            lst = []
            for i in range(64):
                cams = rng.choice(6, size=int(rng.integers(1, 4)), replace=False)
                lst.append(obj(site(i, rng) - np.array([0, 0, 36.0]), dict(zip([int(v) for v in cams], scores(rng, len(cams)))), rng,
                               cls=int(i % 2), flips={int(cams[0])} if i % 9 == 0 and len(cams) > 1 else ()))
            # one place, two classes: class_aware keeps them apart
            lst.append(obj(lst[5]['pos'] + np.array([0.2, 0.0, 0.1]), {0: 0.91, 3: 0.77}, rng, cls=1 - lst[5]['cls'], ry=lst[5]['ry'], dims=lst[5]['dims']))
            objs.append(lst)
    elif name == 'sixteen_cameras_overflow':
        # C = 16, topk = 128, cap = 256 (N = 2048, the limit): 300 objects, more clusters than cap; same-camera links allowed
        c.update(C=16, topk=128, cap=256, params=ref.params(metric='bev', thresh=0.2, class_aware=False, cross_only=False, merge='mean',
                                                           min_score=MIN_SCORE))
        ext = ring(16, rng)[None]
        lst = []
        for i in range(300):
            cams = rng.choice(16, size=int(rng.integers(1, 3)), replace=False)
            lst.append(obj(site(i, rng, per_row=20) - np.array([0, 0, 60.0]), dict(zip([int(v) for v in cams], scores(rng, len(cams)))), rng))
        # a duplicate inside one camera: with cross_only off the two link
        lst.append(obj(lst[7]['pos'] + np.array([0.1, 0.0, 0.1]), {list(lst[7]['views'])[0]: 0.34}, rng, ry=lst[7]['ry'], dims=lst[7]['dims']))
        objs = [lst]
    elif name == 'three_rigs_own_extrinsics':
        # R = 3, C = 2, topk = 8, every rig its own extrinsics (pitch and roll); rig 1 sees nothing, camera 1 of rig 2 sees nothing
        c.update(R=3, C=2, topk=8, params=ref.params(metric='bev', thresh=0.1, cross_only=False, merge='best', min_score=MIN_SCORE))
        ext = np.stack([np.stack([ext_matrix(rng.uniform(-1, 1), rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(-1, 1, 3))
                                  for _ in range(2)]) for _ in range(3)])
        objs = [[obj(site(i, rng), {0: s0, 1: s1}, rng, cls=i % 2) for i, (s0, s1) in enumerate(zip(scores(rng, 4), scores(rng, 4)))],
                [],
                [obj(site(i, rng), {0: s0}, rng) for i, s0 in enumerate(scores(rng, 3))]]
    else:
        raise KeyError(name)
    c['ext'] = np.ascontiguousarray(ext[..., :3, :].reshape(c['R'], c['C'], 12))
    c['objs'] = objs
    c['rec'] = np.ascontiguousarray(np.concatenate([render(objs[r], ext[r], c['topk'], rng, junk=True) for r in range(c['R'])]))
    if c['cap'] is None:
        c['cap'] = min(256, c['C'] * c['topk'])
    return c


NAMES = ('one_camera_passthrough', 'two_cameras_ties_and_flip', 'three_cameras_chain_dist', 'six_cameras_two_rigs', 'sixteen_cameras_overflow',
         'three_rigs_own_extrinsics')


def case(name):
    """The case and the yardstick's result; reseeded until the margin is >= MARGIN."""
    if name not in _cache:
        for seed in range(100 * NAMES.index(name), 100 * NAMES.index(name) + 100):
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
