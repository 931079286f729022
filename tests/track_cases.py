"""Generated record sequences for the tracking tests (seeded, nothing from outside): objects that move at constant velocity in
camera coordinates, seen with a little noise, written as (B, topk, 32) fp32 records per frame.  Events: late arrivals and
departures, detection gaps, a heading seen from the other end, two objects crossing, two classes at one place, more objects than
track slots, frames without a detection, junk slots (flag 0, flag 1, flag 2 below min_score) between the kept ones.
``cases()`` returns the table; a case is reseeded until the yardstick's own decision margin is >= MARGIN in every frame of every
stream, so that no near-tie lets two correct implementations differ.  ``reference(case)`` is the yardstick's result, computed
once per process."""
import numpy as np

from tests import track_ref as ref

MARGIN = 1e-6
FRAMES = 12
_cache = {}


def obj(i, rng, **kw):
    """One object: grid site i (9 m apart), car-sized, slow."""
    o = dict(cls=0, dims=rng.uniform(0.9, 1.1, 3) * np.array([1.6, 1.8, 4.0]),
             pos=np.array([(i % 6) * 9.0 - 22.0, 1.0, (i // 6) * 9.0 + 8.0]) + rng.uniform(-0.5, 0.5, 3),
             vel=rng.uniform(-0.3, 0.3, 3) * np.array([1.0, 0.02, 1.0]), ry=rng.uniform(-3.1, 3.1), score=0.95 - 0.005 * i,
             frames=set(range(FRAMES)), flips=set())
    o.update(kw)
    return o


def ego_matrix(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, 0, s, t[0]], [0, 1, 0, t[1]], [-s, 0, c, t[2]]], np.float64).reshape(12)


def render(objs, topk, egos, rng, min_score, noise=0.03):
    """(FRAMES, topk, 32) records of one stream.  The true state moves as the filter predicts (step, then ego motion)."""
    out = np.zeros((FRAMES, topk, 32), np.float32)
    state = [np.concatenate([np.zeros(7), o['dims'], o['pos'], [o['ry']], o['vel'], np.zeros(7)]) for o in objs]
    for f in range(FRAMES):
        rows = []
        for o, s in zip(objs, state):
            if f > 0:
                ref.predict(s, 1.0, None if egos is None else egos[f])
            if f in o['frames']:
                r = np.zeros(32)
                r[0], r[1] = o['cls'], o['score']
                r[2:24] = rng.uniform(0, 300, 22)
                r[24:27] = s[7:10] + rng.normal(0, 0.01, 3)
                r[27:30] = s[10:13] + rng.normal(0, noise, 3)
                r[30] = s[13] + rng.normal(0, 0.02) + (np.pi if f in o['flips'] else 0.0)
                r[31] = 2
                rows.append(r)
        rows.sort(key=lambda r: -r[1])
        rows = rows[:topk]
        # junk between the kept ones while there is room: a 2D-only slot carrying a box, an empty slot, a kept slot below min_score
        slots, j = [], 0
        for n, r in enumerate(rows):
            room = topk - len(slots) - (len(rows) - n)
            if n % 3 == 1 and room > 0:
                junk = r.copy()
                kind = j % 3
                j += 1
                if kind == 0:
                    junk[31] = 1
                elif kind == 1:
                    junk[:] = 0
                else:
                    junk[1] = min_score * 0.5
                slots.append(junk)
            slots.append(r)
        out[f, :len(slots)] = np.array(slots, np.float32).reshape(-1, 32)
    return out


def build(name, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = dict(name=name, seed=seed, dt=1.0, egos=None, T=128, topk=100)
    streams = []
    if name == 'dense_3d':
        # 74 objects on 128 slots: 70+ live tracks and detections in most frames, every cross-wave prefix is crossed
        c.update(params=ref.params(metric='3d', min_score=0.3))
        objs = [obj(i, rng) for i in range(74)]
        objs[3]['frames'] = set(range(FRAMES)) - {4, 5}               # a gap of max_misses frames: the id survives
        objs[9]['frames'] = set(range(FRAMES)) - {3, 4, 5}            # one more: it does not
        objs[9]['vel'] = np.zeros(3)
        objs[3]['vel'] = np.zeros(3)
        objs[12]['flips'] = {6}                                       # seen from the other end once
        objs[20]['frames'] = set(range(5, FRAMES))                    # arrives late
        objs[21]['frames'] = set(range(0, 6))                         # leaves
        for i in range(60, 74):
            objs[i]['frames'] = set(range(1, FRAMES))                 # frame 1: more detections than tracks
        for i in range(40, 50):
            objs[i]['frames'] = set(range(0, 8))                      # frame 8: more tracks than detections
        streams = [objs]
    elif name == 'overflow_bev':
        # 12 objects on 8 slots: the lowest scores are dropped and counted, a slot freed by a departure is taken again
        c.update(T=8, params=ref.params(metric='bev', thresh=0.05, min_score=0.3, max_misses=1))
        objs = [obj(i, rng) for i in range(12)]
        objs[2]['frames'] = set(range(0, 4))
        streams = [objs]
    elif name == 'three_streams_classes':
        # B = 3, topk = 7: two classes at one place (class_aware), a frame without detections, an empty stream start
        c.update(T=8, topk=7, params=ref.params(metric='3d', class_aware=True, min_score=0.3, min_hits=2))
        for b in range(3):
            objs = [obj(i + b, rng) for i in range(4)]
            twin = dict(objs[0], cls=1, score=objs[0]['score'] - 0.002, pos=objs[0]['pos'] + np.array([0.15, 0.0, 0.1]))
            objs.append(twin)
            if b == 1:
                for o in objs:
                    o['frames'] = set(range(FRAMES)) - {5}            # a frame with no detection at all
            if b == 2:
                for o in objs:
                    o['frames'] = set(range(3, FRAMES))               # nothing in the first three frames
            streams.append(objs)
    elif name == 'twins_class_blind':
        # the same two classes at one place with class_aware off: the two tracks compete for the two detections
        c.update(T=8, topk=7, params=ref.params(metric='bev', class_aware=False, min_score=0.3))
        objs = [obj(i, rng) for i in range(3)]
        objs.append(dict(objs[0], cls=1, score=objs[0]['score'] - 0.002, pos=objs[0]['pos'] + np.array([0.6, 0.0, 0.4])))
        streams = [objs]
    elif name == 'crossing_dist_ego':
        # centre distance, ego yaw and translation per frame, two objects crossing in neighbouring lanes, B = 3
        c.update(T=128, topk=100, params=ref.params(metric='dist', thresh=-3.0, min_score=0.3))
        c['egos'] = np.stack([np.stack([ego_matrix(rng.uniform(-0.04, 0.04), rng.uniform(-0.4, 0.4, 3) * np.array([1, 0.05, 1]))
                                        for _ in range(3)]) for _ in range(FRAMES)])
        for b in range(3):
            objs = [obj(i, rng) for i in range(6 + 5 * b)]
            a = obj(40, rng, pos=np.array([-6.0, 1.0, 60.0]), vel=np.array([1.0, 0.0, 0.0]), ry=0.0)
            d = obj(41, rng, pos=np.array([6.0, 1.0, 62.2]), vel=np.array([-1.0, 0.0, 0.0]), ry=3.0)
            streams.append(objs + [a, d])
    else:
        raise KeyError(name)
    c['objs'] = streams
    egos = c['egos']
    per = [render(objs, c['topk'], None if egos is None else egos[:, b], rng, c['params']['min_score']) for b, objs in enumerate(streams)]
    c['frames'] = [np.ascontiguousarray(np.stack([p[f] for p in per])) for f in range(FRAMES)]
    return c


NAMES = ('dense_3d', 'overflow_bev', 'three_streams_classes', 'twins_class_blind', 'crossing_dist_ego')


def case(name):
    """The case and the yardstick's result [(ids, tables, margins)] per frame; reseeded until every margin is >= MARGIN."""
    if name not in _cache:
        for seed in range(100 * NAMES.index(name), 100 * NAMES.index(name) + 100):
            c = build(name, seed)
            res = ref.run(c['frames'], c['T'], c['params'], c['dt'], c['egos'])
            if min(float(r[2].min()) for r in res) >= MARGIN:
                _cache[name] = (c, res)
                break
        else:
            raise RuntimeError('no seed gives case %s a decision margin of %g' % (name, MARGIN))
    return _cache[name]


def cases():
    return [case(n)[0] for n in NAMES]


def reference(c):
    return case(c['name'])[1]
