"""The yardstick of the optimal association (include/rtm3d_hip.h, "tracking", step 3b): the frame step of tests/track_ref.py
with a pluggable matcher.  Steps 1, 2 and 4 are tests.track_ref's own functions (predict, predict_cov, affinity, update,
detections), imported; the births and ids of steps 5 and 6 are restated here from the header, because track_ref.step has them
inline - tests/test_track_assign_cpu.py holds this file's step with the greedy matcher against track_ref.step, bit for bit.

The optimal matcher is a small Hungarian method of its own, written from the header text and not from the kernel: the classic
potentials form on the cost matrix -(affinity - thresh) with one zero column per row appended ("stay unmatched"), solved per
connected component of the candidate graph.  tests/test_track_assign_cpu.py checks it against scipy and against brute force.

``step`` returns (ids, margin, gain): gain is the sum of affinity - thresh over the matched pairs, margin the smaller of
  (a) tests.track_ref's threshold and heading margins (how far any affinity is from the threshold, how far a matched heading
      difference is from pi / 2), and
  (b) the uniqueness margin of the optimum: the optimum minus the best value with one matched pair forbidden, minimised over the
      matched pairs - 0 when a second matching attains the maximum.
Two correct implementations can only be compared on frames whose margin is well above their arithmetic difference."""
import itertools

import numpy as np

from tests import track_ref as ref
from tests import track_cases as tc

HEADER, SLOT = ref.HEADER, ref.SLOT


# ------------------------------------------------------------------------------------------------------------ matchers
def hungarian(G):
    """G (n, m) gains, NaN where the pair is no candidate.  The matching of largest summed gain, rows and columns free to stay
    unmatched: (col (n,) int, -1 unmatched; total).  Potentials form, one row added at a time, columns 1-based with column 0 the
    virtual start; the m real columns are followed by n private zero columns."""
    G = np.asarray(G, np.float64)
    n, m = G.shape
    M = m + n
    C = np.full((n, M), np.inf)
    C[:, :m] = np.where(np.isnan(G), np.inf, -G)
    C[np.arange(n), m + np.arange(n)] = 0.0
    u, v = np.zeros(n + 1), np.zeros(M + 1)
    p, way = np.zeros(M + 1, np.int64), np.zeros(M + 1, np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(M + 1, np.inf)
        used = np.zeros(M + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = C[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            free = np.flatnonzero(~used[1:]) + 1
            j1 = int(free[np.argmin(minv[free])])
            delta = minv[j1]
            assert np.isfinite(delta)                        # the private column of the first row is always there
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = np.full(n, -1, np.int64)
    for j in range(1, m + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    total = float(sum(G[i, col[i]] for i in range(n) if col[i] >= 0))
    return col, total


def components(pairs):
    """Connected components of the candidate graph: [[(g, t, k)]]."""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for _, t, k in pairs:
        parent[find(('t', t))] = find(('k', k))
    comp = {}
    for c in pairs:
        comp.setdefault(find(('t', c[1])), []).append(c)
    return list(comp.values())


def solve_component(pairs, forbid=None):
    ts, ks = sorted({c[1] for c in pairs}), sorted({c[2] for c in pairs})
    G = np.full((len(ts), len(ks)), np.nan)
    for g, t, k in pairs:
        if (t, k) != forbid:
            G[ts.index(t), ks.index(k)] = g
    col, total = hungarian(G)
    return {ts[i]: ks[col[i]] for i in range(len(ts)) if col[i] >= 0}, total


def optimal_match(pairs, with_margin=True):
    """pairs: [(gain, t, k)] of the candidates.  ({t: k}, total gain, uniqueness margin)."""
    det_of, total, margin = {}, 0.0, np.inf
    for comp in components(pairs):
        m, val = solve_component(comp)
        det_of.update(m)
        total += val
        if with_margin:
            for t, k in m.items():
                margin = min(margin, val - solve_component(comp, forbid=(t, k))[1])
    return det_of, total, margin


def optimal(cand, thresh):
    """The matcher of step 3b on the candidates [(affinity, t, k)]."""
    return optimal_match([(a - thresh, t, k) for a, t, k in cand])


def greedy(cand, thresh):
    """The matcher of step 3 (tests.track_ref's, restated): no uniqueness margin of its own."""
    det_of, trk_of = {}, {}
    for a, t, k in sorted(cand, key=lambda c: (-c[0], c[1], c[2])):
        if t not in det_of and k not in trk_of:
            det_of[t], trk_of[k] = k, t
    return det_of, float(sum(a - thresh for a, t, k in cand if det_of.get(t) == k)), np.inf


def brute_force(G):
    """The largest summed gain over ALL matchings of a small gain matrix (NaN = no candidate)."""
    G = np.asarray(G, np.float64)
    n, m = G.shape
    best = 0.0
    for r in range(1, min(n, m) + 1):
        for rows in itertools.combinations(range(n), r):
            for cols in itertools.permutations(range(m), r):
                g = [G[i, j] for i, j in zip(rows, cols)]
                if not np.isnan(g).any():
                    best = max(best, float(sum(g)))
    return best


# ------------------------------------------------------------------------------------------------------------ the frame step
def step(st, rec, dt=1.0, ego=None, P=None, matcher=optimal):
    """One frame of one stream: st (track_ref.Stream) is updated in place.  Returns (ids (topk,) int32, margin, gain)."""
    P = ref.params() if P is None else P
    metric = ref.METRICS[P['metric']]
    rec = np.asarray(rec, np.float32)
    topk = rec.shape[0]
    frame = st.header[1] + 1.0
    margin = np.inf
    live = st.live()
    for t in live:
        ref.predict(st.slots[t], dt, ego)
        ref.predict_cov(st.slots[t], dt, P)
        st.slots[t, 6] = -1.0
    dets = ref.detections(rec, P['min_score'])
    box = rec[:, 24:31].astype(np.float64)
    cand = []
    for t in live:
        for k in dets:
            if P['class_aware'] and st.slots[t, 1] != np.float64(rec[k, 0]):
                continue
            a = ref.affinity(st.slots[t], box[k], metric)
            if not (metric != 2 and a == 0.0 and P['thresh'] >= 0.0) and a == a:
                margin = min(margin, abs(a - P['thresh']))
            if a > P['thresh']:
                cand.append((a, t, k))
    det_of, gain, unique = matcher(cand, np.float64(P['thresh']))
    margin = min(margin, unique)
    trk_of = {k: t for t, k in det_of.items()}
    assert len(trk_of) == len(det_of) and all(any(c[1] == t and c[2] == k for c in cand) for t, k in det_of.items())
    owner = {}
    for t in live:
        s = st.slots[t]
        if t in det_of:
            k = det_of[t]
            margin = min(margin, ref.update(s, box[k], np.float64(rec[k, 1]), k, P))
            owner[k] = t
        else:
            s[3] = 0.0
            s[4] += 1.0
            if s[4] > P['max_misses']:
                s[:] = 0.0
    # 5 BIRTHS: the unmatched detections in slot order into the free slots in slot order; the n-th gets id header[0] + n
    free = [t for t in range(st.T) if st.slots[t, 0] == 0]
    births = [k for k in dets if k not in trk_of]
    born = min(len(births), len(free))
    for n in range(born):
        k, s = births[n], st.slots[free[n]]
        s[:] = 0.0
        s[0] = st.header[0] + (n + 1)
        s[1] = rec[k, 0]
        s[2], s[3], s[4], s[5], s[6] = 1.0, 1.0, 0.0, rec[k, 1], k
        s[7:13] = box[k, :6]
        s[13] = ref.wrap(box[k, 6])
        s[17], s[18], s[19], s[20], s[21] = P['p0_pos'], 0.0, P['p0_vel'], P['p0_ry'], P['p0_dim']
        owner[k] = free[n]
    st.header[0] += born
    st.header[1] = frame
    st.header[2] += len(births) - born
    # 6 IDS: +id confirmed (hits >= min_hits or frame <= min_hits), -id tentative
    ids = np.zeros(topk, np.int32)
    for k, t in owner.items():
        s = st.slots[t]
        confirmed = s[3] >= P['min_hits'] or frame <= P['min_hits']
        ids[k] = int(s[0]) if confirmed else -int(s[0])
    return ids, margin, gain


def run(sequence, T, P=None, dt=1.0, egos=None, matcher=optimal):
    """A whole sequence of (B, topk, 32) frames: [(ids (B, topk), tables (B, HEADER + SLOT * T), margins (B,), gains (B,))]."""
    B = sequence[0].shape[0]
    streams = [ref.Stream(T) for _ in range(B)]
    out = []
    for f, rec in enumerate(sequence):
        ego = None if egos is None else egos[f]
        res = [step(streams[b], rec[b], dt, None if ego is None else ego[b], P, matcher) for b in range(B)]
        out.append((np.stack([r[0] for r in res]), np.stack([s.table() for s in streams]), np.array([r[1] for r in res]),
                    np.array([r[2] for r in res])))
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
_cache = {}
CHAIN = 40


def _records(B, topk, frames):
    """frames: per frame, per stream, [(slot, x, z, score)] - car-sized boxes at height 1, heading 0, class 0."""
    out = []
    for per in frames:
        rec = np.zeros((B, topk, 32), np.float32)
        for b, rows in enumerate(per):
            for slot, x, z, score in rows:
                rec[b, slot, 0], rec[b, slot, 1] = 0.0, score
                rec[b, slot, 24:31] = (1.5, 1.75, 4.0, x, 1.0, z, 0.0)
                rec[b, slot, 31] = 2.0
        out.append(rec)
    return out


def chain_dist():
    """The case the greedy rule gets wrong: 40 tracks 3 m apart, every detection 1.505 m right of its own track and 1.495 m left of
    the next one.  Stream 1 holds the same chain with the record slots in reversed x order."""
    order = [list(range(CHAIN)), list(range(CHAIN - 1, -1, -1))]
    frames = [[[(s, 3.0 * i + off, 20.0, 0.9 - 0.001 * s) for s, i in enumerate(o)] for o in order] for off in (0.0, 1.505)]
    return dict(name='chain_dist', T=64, topk=48, dt=1.0, egos=None, frames=_records(2, 48, frames),
                params=ref.params(metric='dist', thresh=-2.0, class_aware=False))


def exact_ties():
    """Two tracks at x = -1.5 and 1.5, z = 10; two detections at x = 0, z = 12 and z = 8: all four distances are exactly 2.5."""
    frames = [[[(0, -1.5, 10.0, 0.9), (1, 1.5, 10.0, 0.8)]], [[(0, 0.0, 12.0, 0.9), (1, 0.0, 8.0, 0.8)]]]
    return dict(name='exact_ties', T=8, topk=8, dt=1.0, egos=None, frames=_records(1, 8, frames),
                params=ref.params(metric='dist', thresh=-4.0))


def no_candidates():
    """Five tracks, then five detections 100 m from all of them."""
    frames = [[[(s, 4.0 * s + off, 15.0, 0.9 - 0.01 * s) for s in range(5)]] for off in (0.0, 100.0)]
    return dict(name='no_candidates', T=8, topk=8, dt=1.0, egos=None, frames=_records(1, 8, frames),
                params=ref.params(metric='dist', thresh=-2.0, max_misses=2))


def case(name):
    """A tests.track_cases sequence under the optimal rule: (case, [(ids, tables, margins, gains)] per frame), reseeded - over
    the seeds track_cases itself would try - until this file's margin is >= track_cases.MARGIN in every frame of every stream."""
    if name not in _cache:
        first = 100 * tc.NAMES.index(name)
        for seed in range(first, first + 100):
            c = tc.build(name, seed)
            res = run(c['frames'], c['T'], c['params'], c['dt'], c['egos'])
            if min(float(r[2].min()) for r in res) >= tc.MARGIN:
                _cache[name] = (c, res)
                break
        else:
            raise RuntimeError('no seed gives case %s an optimal-rule margin of %g' % (name, tc.MARGIN))
    return _cache[name]


def fixed(name):
    """One of the hand-made cases above with its yardstick result, computed once per process."""
    if name not in _cache:
        c = dict(chain_dist=chain_dist, exact_ties=exact_ties, no_candidates=no_candidates)[name]()
        _cache[name] = (c, run(c['frames'], c['T'], c['params'], c['dt'], c['egos']))
    return _cache[name]
