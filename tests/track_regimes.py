"""Generated record sequences that take the tracker (csrc/track.hip) into every regime of its two kernels - the cases of
tests/test_track_regimes.py (CPU: the conditions, the yardstick against a matrix filter, mutants) and of
tests/test_gpu_track_regimes.py (the device against the yardstick).  Host only, seeded, nothing from outside.

What tests/track_cases.py leaves out and a case here reaches (every case lists its regime keys; REGIMES of
tests/test_track_regimes.py maps each key to what must be seen on the yardstick's result, and asserts it):
  sizes       T = topk = 256 with live tracks, detections, matches, births and frees in all four 64-slot ranges of the workgroup
              (full_256); a displacement chain and a cascade of mutual-best rounds in slots >= 192 (chain_upper); T = 256 over
              topk = 5 (tall); T = 3 under topk = 256 with hundreds of dropped births (wide); T = topk = 1 (one_by_one); B = 3,
              T = 193, topk = 129 - odd sizes, a block of the affinity kernel that spans two streams (ragged_streams).
  arithmetic  dt = 0.1, 2.5 and a dt drawn per frame, with all four process-noise terms, the three measurement noises and the four
              initial variances non-default and pairwise different (dt_small, dt_large, dt_varying); ego motion with yaw, pitch
              and roll, so all twelve entries of [R | t] count (ego_general); max_misses = 0 with min_hits = 0, min_hits = 1 with
              max_misses = 3, four classes at one site under class_aware, scores of exactly 0 at min_score = 0, yaws written
              outside [-pi, pi) (life_*).
              exact ties of the greedy order in the slots >= 192 (ties_upper; greedy only).
  edges       kept records whose box is not finite or not valid (nonfinite_boxes), pinned to the header's sentence: such a box is
              born, matches nothing and dies of its misses, and its finite neighbours are treated as if it were not there.

A case: name, T, topk, params, ``dts`` (the dt of every call; the truth moves by it, so the filter's model holds), egos or None,
frames [(B, topk, 32) fp32] x 12, regimes.  ``case(name)`` reseeds it (100 seeds) until the decision margin of BOTH yardsticks -
tests/track_ref.py (greedy) and tests/track_assign_ref.py (optimal) - is >= track_cases.MARGIN in every frame of every stream,
and returns (case, {'greedy': result, 'optimal': result}), result = [(ids, tables, margins)] per frame, computed once per
process.  ``run`` is track_ref.run / track_assign_ref.run with the dt of each frame in place of one dt for all."""
import numpy as np

from tests import track_ref as ref
from tests import track_cases as tc
from tests import track_assign_ref as ar

MARGIN, FRAMES = tc.MARGIN, tc.FRAMES
ASSIGNMENTS = ('greedy', 'optimal')
# q_* pairwise different and non-zero, r_* pairwise different and not 1, p0_* pairwise different
NOISE = dict(q_pos=0.03, q_vel=0.07, q_ry=0.011, q_dim=0.005, r_pos=0.6, r_ry=0.3, r_dim=1.7, p0_pos=7.0, p0_vel=900.0, p0_ry=3.0, p0_dim=5.0)
CHAIN = 20
_cache = {}


def rigid(yaw, pitch, roll, t):
    """Row-major [R | t] (12,), R = Ry(yaw) Rx(pitch) Rz(roll): no entry of it is 0 or 1 for non-zero angles."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return np.concatenate([Ry @ Rx @ Rz, np.asarray(t, np.float64).reshape(3, 1)], 1).reshape(12)


def obj(i, rng, **kw):
    """track_cases.obj with a score that stays above min_score for 256 objects (0.002 apart: distinct in fp32)."""
    o = tc.obj(i, rng, score=0.95 - 0.002 * i, turns=0)
    o.update(kw)
    return o


def render(objs, topk, egos, rng, min_score, dts, noise=0.03, junk=True):
    """track_cases.render with the dt of every frame: (FRAMES, topk, 32) records of one stream.  The true state moves as the
    filter predicts (a step of dts[f], then ego motion).  An object's 'turns' adds whole turns to the yaw that is written."""
    out = np.zeros((FRAMES, topk, 32), np.float32)
    state = [np.concatenate([np.zeros(7), o['dims'], o['pos'], [o['ry']], o['vel'], np.zeros(7)]) for o in objs]
    for f in range(FRAMES):
        rows = []
        for o, s in zip(objs, state):
            if f > 0:
                ref.predict(s, dts[f], None if egos is None else egos[f])
            if f in o['frames']:
                r = np.zeros(32)
                r[0], r[1] = o['cls'], o['score']
                r[2:24] = rng.uniform(0, 300, 22)
                r[24:27] = s[7:10] + rng.normal(0, 0.01, 3)
                r[27:30] = s[10:13] + rng.normal(0, noise, 3)
                r[30] = s[13] + rng.normal(0, 0.02) + (np.pi if f in o['flips'] else 0.0) + 2.0 * np.pi * o['turns']
                r[31] = 2
                rows.append(r)
        rows.sort(key=lambda r: -r[1])
        rows = rows[:topk]
        slots, j = [], 0
        for n, r in enumerate(rows):
            room = topk - len(slots) - (len(rows) - n)
            if junk and n % 3 == 1 and room > 0:
                bad = r.copy()
                kind = j % 3
                j += 1
                if kind == 0:
                    bad[31] = 1
                elif kind == 1:
                    bad[:] = 0
                else:
                    bad[1] = min_score * 0.5 if min_score > 0 else -0.25
                slots.append(bad)
            slots.append(r)
        out[f, :len(slots)] = np.array(slots, np.float32).reshape(-1, 32)
    return out


def _absent(o, *frames):
    o['frames'] = set(range(FRAMES)) - set(frames)


def _chain_upper(rng):
    """Hand-placed: 192 static far-away objects hold the slots 0..191.  Chain A, slots 192..211, is tests/track_assign_ref's
    chain_dist - every detection 1.505 m right of its own track and 1.495 m left of the next one - with the track slots in
    descending x, so that the last row's augmenting path runs through all of them; it is displaced in frame 1 and, on top of the
    constant velocity it then has, again in frame 6.  Chain B, slots 212..231: unequal gaps, the distances along the path
    track 0 - detection 0 - track 1 - ... strictly decreasing, so each round of mutual best matches exactly one pair."""
    topk = 256
    frames = []
    fill = np.array([[(i % 16) * 9.0 - 70.0, 100.0 + (i // 16) * 9.0] for i in range(192)]) + rng.uniform(-0.5, 0.5, (192, 2))
    w = 1.9 - 0.02 * np.arange(2 * CHAIN)
    a, gaps = w[0::2], w[0::2] + w[1::2]
    xb = np.concatenate([[0.0], np.cumsum(gaps)[:-1]])
    for f in range(FRAMES):
        rec = np.zeros((1, topk, 32), np.float32)
        rows = [(s, fill[s, 0], fill[s, 1]) for s in range(192)]
        rows += [(192 + j, 3.0 * (CHAIN - 1 - j) + 1.505 * (f + (1 if f >= 6 else 0)), 20.0) for j in range(CHAIN)]
        rows += [(192 + CHAIN + j, xb[j] + a[j] * f, 40.0) for j in range(CHAIN)]
        for s, x, z in rows:
            rec[0, s, 0], rec[0, s, 1] = 0.0, 0.9 - 0.001 * s
            rec[0, s, 24:31] = (1.5, 1.75, 4.0, x + rng.normal(0, 0.0003), 1.0, z + rng.normal(0, 0.0003), 0.0)
            rec[0, s, 31] = 2.0
        frames.append(rec)
    return frames


def _ties_upper():
    """Hand-placed, every coordinate a multiple of 0.5, so the centre distances below are exactly 2.5 on both sides: the greedy
    rule's tie order (the lower track slot, then the lower record slot) in the slots >= 192.  200 static objects hold the slots
    0..199.  Frame 0 opens five tracks in the slots 200..204; frame 1 brings
      one detection (record slot 210) 2.5 m from the tracks 200 and 201: the lower track slot takes it;
      two detections (220, 215) 2.5 m from track 202: it takes the lower record slot, the other is born;
      detections x (230) and y (231), tracks A (203) and B (204), A-x = B-x = B-y = 2.5: A-x first, so B takes y in a second round;
    after that only the 200 stay, and the five die of their misses."""
    fill = [((i % 16) * 9.0 - 70.0, 200.0 + (i // 16) * 9.0) for i in range(200)]
    first = [(200, -1.5, 10.0), (201, 1.5, 10.0), (202, 0.0, 60.0), (203, -1.5, 110.0), (204, 1.5, 110.0)]
    second = [(210, 0.0, 12.0), (220, -1.5, 62.0), (215, 1.5, 62.0), (230, 0.0, 112.0), (231, 3.0, 112.0)]
    frames = []
    for f in range(FRAMES):
        rec = np.zeros((1, 256, 32), np.float32)
        for s, x, z in [(i, x, z) for i, (x, z) in enumerate(fill)] + (first if f == 0 else second if f == 1 else []):
            rec[0, s, 0], rec[0, s, 1] = 0.0, 0.9 - 0.001 * s
            rec[0, s, 24:31] = (1.5, 1.75, 4.0, x, 1.0, z, 0.0)
            rec[0, s, 31] = 2.0
        frames.append(rec)
    return frames


def _nonfinite(frames, rng):
    """The finite records of every frame move to the odd record slots.  The even ones of the frames 2, 3, 6 and 8 get kept records
    (flag 2, score above min_score) whose box is not finite or not valid: a NaN centre, an infinite yaw, no width - at the very
    place of finite object 1 - and a negative length; the last two come again a frame later, unchanged, and still match nothing.
    A record with a NaN score at the very box of finite object 0 is no detection at all."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    far = np.array([1.5, 1.7, 4.1, 3.0, 1.0, 30.0, 0.4], np.float32)
    out = []
    for f, rec in enumerate(frames):
        new = np.zeros_like(rec)
        new[0, 1::2] = rec[0, :4]

        def bad(slot, score, box, **kw):
            new[0, slot, 0], new[0, slot, 1], new[0, slot, 31] = 0.0, score, 2.0
            new[0, slot, 2:24] = rng.uniform(0, 300, 22)
            new[0, slot, 24:31] = box
            for k, v in kw.items():
                new[0, slot, 24 + 'hwlXYZr'.index(k)] = v
        if f in (2, 6):
            bad(0, 0.99, far, X=nan)
            bad(2, 0.98, far, r=inf, Z=45.0)
            bad(4, 0.97, rec[0, 1, 24:31], w=0.0)
            bad(6, 0.96, far, l=-4.1, Z=75.0)
            bad(7, nan, rec[0, 0, 24:31])
        if f in (3, 8):
            bad(0, 0.96, far, l=-4.1, Z=75.0)
            bad(2, nan, rec[0, 0, 24:31])
            bad(4, 0.97, frames[f - 1][0, 1, 24:31], w=0.0)
        out.append(new)
    return out


def build(name, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = dict(name=name, seed=seed, egos=None, T=16, topk=12, dts=[1.0] * FRAMES, regimes=(), tie_frames=())
    junk = True
    small = lambda n: [obj(i, rng) for i in range(n)]
    if name == 'full_256':
        c.update(T=256, topk=256, params=ref.params(metric='3d', min_score=0.3, max_misses=2))
        objs = [obj(i, rng) for i in range(236)]
        # 200 at once; 18 in frame 1, 18 in frame 5, both with scores that spread them over the record slots
        for n, i in enumerate(range(200, 236)):
            objs[i]['score'] = 0.95 - 0.002 * (11 * (n % 18) + 4.5 + (n // 18))
            objs[i]['frames'] = set(range(1 if i < 218 else 5, FRAMES))
        # leave after frame 2, freed in frame 5: free slots in all four ranges when the second group is born; 195, 196 taken again
        for i in (5, 6, 7, 70, 71, 72, 135, 136, 137, 195, 196):
            objs[i]['frames'] = {0, 1, 2}
        # gaps of max_misses frames (the id survives) and of one more (it does not), on tracks in the slots >= 128 and >= 192
        for i, gap in ((140, (4, 5)), (150, (3, 4, 5)), (210, (0, 7, 8)), (212, (0, 7, 8, 9))):
            _absent(objs[i], *gap)
            objs[i]['vel'] = np.zeros(3)
        objs[160]['flips'] = {6}
        objs[215]['flips'] = {9}
        streams = [objs]
        c['regimes'] = ('live_all_ranges', 'dets_all_ranges', 'matches_upper', 'births_frees_three_ranges', 'slot_192_reused', 'gaps_upper')
    elif name == 'chain_upper':
        c.update(T=256, topk=256, params=ref.params(metric='dist', thresh=-2.0))
        c['frames'] = _chain_upper(rng)
        c['regimes'] = ('matches_upper', 'greedy_rounds', 'long_path_upper')
        return c
    elif name == 'ties_upper':
        c.update(T=256, topk=256, params=ref.params(metric='dist', thresh=-4.0), frames=_ties_upper(), tie_frames=(1,))
        c['regimes'] = ('ties_upper',)
        return c
    elif name == 'tall':
        # two objects stay; three new ones in every frame, seen once, coast for max_misses frames: 20 rows over 5 columns
        c.update(T=256, topk=5, params=ref.params(metric='bev', thresh=0.05, min_score=0.3, max_misses=5))
        objs = [obj(i, rng) for i in range(2 + 3 * FRAMES)]
        for i in range(2, len(objs)):
            objs[i]['frames'] = {(i - 2) // 3}
        streams = [objs]
        c['regimes'] = ('tall',)
    elif name == 'wide':
        c.update(T=3, topk=256, params=ref.params(metric='3d', min_score=0.3, max_misses=1))
        objs = [obj(i, rng) for i in range(200)]
        objs[1]['frames'] = set(range(0, 5))                 # its slot is freed and taken by the best of the waiting ones
        streams = [objs]
        c['regimes'] = ('wide_dropped',)
    elif name == 'one_by_one':
        c.update(T=1, topk=1, params=ref.params(metric='dist', thresh=-3.0, min_score=0.3, max_misses=2))
        first, second = obj(0, rng), obj(7, rng)
        first['frames'], second['frames'] = {0, 1, 2, 3}, set(range(5, FRAMES))      # born while the first still holds the slot: dropped
        streams, junk = [[first, second]], False
        c['regimes'] = ('one_by_one',)
    elif name == 'ragged_streams':
        c.update(T=193, topk=129, params=ref.params(metric='3d', min_score=0.3, max_misses=4))
        # stream 0: 100 stay; 29 new ones in each of the frames 0..3, seen once: their slots stay held for four more frames, so the
        # births reach slot 192 and the last group is partly dropped; stream 1: a few; stream 2: nothing for three frames
        objs = [obj(i, rng) for i in range(100 + 29 * 4 + 20)]
        for g in range(4):
            for i in range(100 + 29 * g, 129 + 29 * g):
                objs[i]['frames'] = {g}
        for i in range(216, 236):
            objs[i]['frames'] = set(range(6, FRAMES))
        mid = [obj(i, rng) for i in range(40)]
        _absent(mid[3], 4, 5)
        few = [obj(i, rng) for i in range(8)]
        for o in few:
            o['frames'] = set(range(3, FRAMES))
        streams = [objs, mid, few]
        c['regimes'] = ('ragged', 'empty_stream_start', 'slot_T_minus_1')
    elif name in ('dt_small', 'dt_large', 'dt_varying'):
        c.update(params=ref.params(metric='3d', min_score=0.3, **NOISE))
        c['dts'] = {'dt_small': [0.1] * FRAMES, 'dt_large': [2.5] * FRAMES,
                    'dt_varying': [float(v) for v in rng.choice([0.04, 0.1, 0.5], FRAMES)]}[name]
        objs = small(8)
        for o in objs:
            o['vel'] = o['vel'] * (0.4 if name == 'dt_large' else 3.0)
        _absent(objs[2], 4, 5)                               # two predictions in a row without an update
        streams = [objs]
        c['regimes'] = (name, 'noise_all')
    elif name == 'ego_general':
        c.update(params=ref.params(metric='3d', min_score=0.3, **NOISE))
        c['dts'] = [0.7] * FRAMES
        c['egos'] = np.stack([np.stack([rigid(*rng.uniform(0.02, 0.05, 3) * rng.choice([-1.0, 1.0], 3), rng.uniform(-0.4, 0.4, 3))
                                        for _ in range(2)]) for _ in range(FRAMES)])
        streams = [small(7), small(5)]
        _absent(streams[0][1], 5, 6)
        c['regimes'] = ('ego_general', 'noise_all')
    elif name == 'life_misses0':
        c.update(params=ref.params(metric='3d', min_score=0.3, max_misses=0, min_hits=0))
        objs = small(6)
        _absent(objs[1], 4)                                  # one frame away: a new id
        objs[4]['frames'] = set(range(5, FRAMES))
        streams = [objs]
        c['regimes'] = ('max_misses_0', 'min_hits_0')
    elif name == 'life_hits1':
        c.update(params=ref.params(metric='3d', min_score=0.3, max_misses=3, min_hits=1))
        objs = small(6)
        _absent(objs[1], 4, 5, 6)                            # three frames away: the id survives
        objs[2].update(frames=set(range(0, 3)), vel=np.zeros(3))               # four: it does not, and comes back as a new object
        objs.append(dict(objs[2], frames=set(range(7, FRAMES))))
        objs[4]['frames'] = set(range(5, FRAMES))
        streams = [objs]
        c['regimes'] = ('min_hits_1', 'max_misses_3')
    elif name == 'life_classes4':
        c.update(params=ref.params(metric='3d', class_aware=True, min_score=0.3))
        objs = []
        for site in range(3):
            base = obj(site, rng)
            for cls in range(4):
                objs.append(dict(base, cls=cls, score=base['score'] - 0.0004 * cls, frames=set(range(FRAMES)), flips=set(),
                                 pos=base['pos'] + np.array([0.12 * cls, 0.0, 0.09 * cls])))
        _absent(objs[5], 3, 4)
        streams = [objs]
        c['regimes'] = ('classes_4',)
    elif name == 'life_score0':
        c.update(params=ref.params(metric='bev', thresh=0.05, min_score=0.0))
        objs = small(9)
        for i in (2, 5):
            objs[i]['score'] = 0.0
        streams = [objs]
        c['regimes'] = ('score_0',)
    elif name == 'life_yaw_wide':
        c.update(params=ref.params(metric='3d', min_score=0.3))
        objs = small(6)
        objs[0].update(ry=7.0 - 2.0 * np.pi, turns=1)        # written as 7.0
        objs[1].update(ry=-9.5 + 4.0 * np.pi, turns=-2)      # written as -9.5
        objs[2].update(ry=3.13, turns=3)                     # at the seam, three turns on
        objs[1]['flips'] = {5}
        streams = [objs]
        c['regimes'] = ('yaw_outside',)
    elif name == 'nonfinite_boxes':
        c.update(T=8, topk=8, params=ref.params(metric='3d', min_score=0.3, max_misses=1))
        objs = small(3)
        objs[2]['frames'] = set(range(6, FRAMES))            # a finite box born in a frame that has bad ones before and after it
        per = render(objs, 8, None, rng, 0.3, c['dts'], junk=False)
        c['frames'] = _nonfinite([per[f][None] for f in range(FRAMES)], rng)
        c['regimes'] = ('nonfinite',)
        return c
    else:
        raise KeyError(name)
    egos = c['egos']
    per = [render(objs, c['topk'], None if egos is None else egos[:, b], rng, c['params']['min_score'], c['dts'], junk=junk)
           for b, objs in enumerate(streams)]
    c['frames'] = [np.ascontiguousarray(np.stack([p[f] for p in per])) for f in range(FRAMES)]
    return c


SIZES = ('full_256', 'chain_upper', 'tall', 'wide', 'one_by_one', 'ragged_streams')
ARITHMETIC = ('dt_small', 'dt_large', 'dt_varying', 'ego_general', 'life_misses0', 'life_hits1', 'life_classes4', 'life_score0', 'life_yaw_wide')
EDGES = ('nonfinite_boxes',)
NAMES = SIZES + ARITHMETIC + EDGES
GREEDY_ONLY = ('ties_upper',)        # exact ties: the greedy rule orders them; under the optimal rule any optimum may be returned
ALL = NAMES + GREEDY_ONLY


def run(c, assignment):
    """[(ids (B, topk), tables (B, HEADER + SLOT * T), margins (B,))] per frame: the loop of track_ref.run (greedy) or
    track_assign_ref.run (optimal) with dts[f] as the dt of frame f."""
    B = c['frames'][0].shape[0]
    streams = [ref.Stream(c['T']) for _ in range(B)]
    out = []
    with np.errstate(invalid='ignore'):                      # wrap(inf) of nonfinite_boxes: NaN, as on the device
        for f, rec in enumerate(c['frames']):
            res = []
            for b in range(B):
                ego = None if c['egos'] is None else c['egos'][f][b]
                if assignment == 'greedy':
                    res.append(ref.step(streams[b], rec[b], c['dts'][f], ego, c['params']))
                else:
                    res.append(ar.step(streams[b], rec[b], c['dts'][f], ego, c['params'])[:2])
            out.append((np.stack([r[0] for r in res]), np.stack([s.table() for s in streams]), np.array([r[1] for r in res])))
    return out


def case(name):
    if name in GREEDY_ONLY and name not in _cache:
        c = build(name, 0)                                   # hand-placed: its margin is 0 in c['tie_frames'], on purpose
        _cache[name] = (c, {'greedy': run(c, 'greedy')})
    if name not in _cache:
        first = 100 * (10 + NAMES.index(name))
        for seed in range(first, first + 100):
            c = build(name, seed)
            res = {}
            for a in ASSIGNMENTS:
                res[a] = run(c, a)
                if min(float(r[2].min()) for r in res[a]) < MARGIN:
                    break
            else:
                _cache[name] = (c, res)
                break
        else:
            raise RuntimeError('no seed gives case %s a decision margin of %g under both assignments' % (name, MARGIN))
    return _cache[name]


def reference(name, assignment):
    return case(name)[1][assignment]


# ------------------------------------------------------------------------------------------ what a result shows
def slots_of(c, res):
    """(FRAMES, B, T, SLOT) of a result."""
    B = c['frames'][0].shape[0]
    return np.stack([r[1][:, ref.HEADER:].reshape(B, c['T'], ref.SLOT) for r in res])


def detections(c):
    """[frame][stream] -> record slots of the detections."""
    return [[ref.detections(rec[b], c['params']['min_score']) for b in range(rec.shape[0])] for rec in c['frames']]


def events(c, res, b=0):
    """Per frame of stream b: dict(live, matched, born, freed: track slots; unmatched: record slots of the detections no live track
    took, dropped births included; free: the slots that were free when the births were placed)."""
    s = slots_of(c, res)[:, b]
    dets = detections(c)
    out = []
    for f in range(len(res)):
        before = set(np.flatnonzero(s[f - 1][:, 0] != 0).tolist()) if f else set()
        live = set(np.flatnonzero(s[f][:, 0] != 0).tolist())
        born = {t for t in live if s[f][t, 2] == 1}
        matched = {t for t in live - born if s[f][t, 6] >= 0}
        freed = {t for t in before if t not in live or (t in born)}
        taken = {int(s[f][t, 6]) for t in matched}
        out.append(dict(live=live, matched=matched, born=born, freed=freed, unmatched=[k for k in dets[f][b] if k not in taken],
                        free=sorted((set(range(c['T'])) - before) | freed)))
    return out


def candidates(c, res, f, b=0):
    """[(affinity, t, k)] of frame f of stream b, from the yardstick's table after frame f - 1."""
    P, rec = c['params'], c['frames'][f][b]
    s = slots_of(c, res)[f - 1, b].copy()
    box = rec[:, 24:31].astype(np.float64)
    ego = None if c['egos'] is None else c['egos'][f][b]
    cand = []
    for t in np.flatnonzero(s[:, 0] != 0):
        ref.predict(s[t], c['dts'][f], ego)
        for k in ref.detections(rec, P['min_score']):
            if not (P['class_aware'] and s[t, 1] != np.float64(rec[k, 0])):
                a = ref.affinity(s[t], box[k], ref.METRICS[P['metric']])
                if a > P['thresh']:
                    cand.append((a, int(t), k))
    return cand


def greedy_rounds(cand):
    """The rounds of mutual best (csrc/track.hip) that match at least one pair, and the pairs of each."""
    left, rounds = list(cand), []
    while left:
        order = sorted(left, key=lambda c: (-c[0], c[1], c[2]))
        row, col = {}, {}
        for a, t, k in order:
            row.setdefault(t, k)
            col.setdefault(k, t)
        took = [(t, k) for t, k in row.items() if col[k] == t]
        rounds.append(took)
        ts, ks = {t for t, _ in took}, {k for _, k in took}
        left = [c for c in left if c[1] not in ts and c[2] not in ks]
    return rounds


def path_steps(cand, thresh):
    """Rows added in slot order, as the kernel does: for each row, 1 + the number of earlier rows whose detection changes when
    it joins (the optimum is unique by the case's margin, and an augmentation changes the rows on its path only): the length
    of its augmenting path.  {row: steps}."""
    rows = sorted({c[1] for c in cand})
    prev, out = {}, {}
    for n, r in enumerate(rows):
        m = ar.optimal_match([(a - thresh, t, k) for a, t, k in cand if t in rows[:n + 1]], with_margin=False)[0]
        out[r] = 1 + sum(1 for t in rows[:n] if m.get(t) != prev.get(t))
        prev = m
    return out
