"""The yardstick of the tracking tests: a numpy fp64 statement of the rule in include/rtm3d_hip.h, "tracking", written from that
comment (sequential greedy match over a sorted pair list, scalar filter arithmetic in the order the comment gives).  The IoUs
come from tests/box_overlap_ref.py, which clips in world coordinates - not the device's arithmetic, agreeing with it to ~1e-14.
tests/test_track_cpu.py checks this file against closed forms before any device result is compared with it.

``Stream`` is one stream's table; ``step`` runs one frame and returns (ids, margin): margin is the smallest decision margin of the
frame - how far any affinity is from the threshold, how far apart two candidate pairs that share a track or a detection are,
and how far a matched heading difference is from the pi/2 at which the track is turned round.  A comparison with another
implementation is only meaningful on frames whose margin is well above the arithmetic difference of the two."""
import numpy as np

from tests import box_overlap_ref as bo

PI, TWO_PI, HALF_PI = 3.141592653589793, 6.283185307179586, 1.5707963267948966
HEADER, SLOT = 8, 24
METRICS = {'bev': 0, '3d': 1, 'dist': 2}
DEFAULTS = dict(metric='3d', class_aware=False, max_misses=2, min_hits=3, thresh=0.01, min_score=0.0, p0_pos=10.0, p0_vel=1e4,
                p0_ry=10.0, p0_dim=10.0, q_pos=0.0, q_vel=0.01, q_ry=0.0, q_dim=0.0, r_pos=1.0, r_ry=1.0, r_dim=1.0)


def wrap(a):
    a = np.float64(a)
    return a - np.float64(TWO_PI) * np.floor((a + np.float64(PI)) / np.float64(TWO_PI))


def params(**kw):
    assert not set(kw) - set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


class Stream(object):
    def __init__(self, T):
        self.T = T
        self.header = np.zeros(HEADER)
        self.slots = np.zeros((T, SLOT))

    def table(self):
        return np.concatenate([self.header, self.slots.reshape(-1)])

    def live(self):
        return [t for t in range(self.T) if self.slots[t, 0] != 0]

    def by_id(self, i):
        t = [t for t in self.live() if self.slots[t, 0] == i]
        return self.slots[t[0]] if t else None


def detections(rec, min_score):
    rec = np.asarray(rec, np.float32)
    return [k for k in range(rec.shape[0]) if rec[k, 31] == 2 and np.float64(rec[k, 1]) >= min_score]


def predict(s, dt, ego):
    """Step 1 on one slot, in place."""
    dt = np.float64(dt)
    x, y, z = s[10] + dt * s[14], s[11] + dt * s[15], s[12] + dt * s[16]
    vx, vy, vz = s[14], s[15], s[16]
    ry = s[13]
    if ego is not None:
        e = np.asarray(ego, np.float64).reshape(12)
        x, y, z = (((e[0] * x + e[1] * y) + e[2] * z) + e[3], ((e[4] * x + e[5] * y) + e[6] * z) + e[7],
                   ((e[8] * x + e[9] * y) + e[10] * z) + e[11])
        vx, vy, vz = ((e[0] * vx + e[1] * vy) + e[2] * vz, (e[4] * vx + e[5] * vy) + e[6] * vz, (e[8] * vx + e[9] * vy) + e[10] * vz)
        c, sn = np.cos(ry), np.sin(ry)
        ry = np.arctan2(-(e[8] * c - e[10] * sn), e[0] * c - e[2] * sn)
    s[10:13] = x, y, z
    s[14:17] = vx, vy, vz
    s[13] = wrap(ry)
    s[2] += 1.0
    return s


def predict_cov(s, dt, P):
    dt = np.float64(dt)
    a, b = s[17] + dt * s[18], s[18] + dt * s[19]
    s[17] = (a + dt * b) + np.float64(P['q_pos']) * dt
    s[18] = b
    s[19] = s[19] + np.float64(P['q_vel']) * dt
    s[20] = s[20] + np.float64(P['q_ry']) * dt
    s[21] = s[21] + np.float64(P['q_dim']) * dt


def affinity(s, z, metric):
    """Step 2 for one (predicted slot, detection box z) pair."""
    ex, ey, ez = s[10] - z[3], s[11] - z[4], s[12] - z[5]
    if metric == 2:
        return -np.sqrt((ex * ex + ey * ey) + ez * ez)
    with np.errstate(invalid='ignore', over='ignore'):
        reach = 0.5 * np.sqrt(s[8] * s[8] + s[9] * s[9]) + 0.5 * np.sqrt(z[1] * z[1] + z[2] * z[2])
        if ex * ex + ez * ez > reach * reach:
            return 0.0
    bev, vol = bo.overlap(s[7:14], z)
    return bev if metric == 0 else vol


def update(s, z, score, k, P):
    """Step 4 on a matched slot, in place; returns the heading margin."""
    zry = wrap(z[6])
    Ppp, Ppv, Pvv = s[17], s[18], s[19]
    S = Ppp + np.float64(P['r_pos'])
    Kp, Kv = Ppp / S, Ppv / S
    for a in range(3):
        y = z[3 + a] - s[10 + a]
        s[10 + a] = s[10 + a] + Kp * y
        s[14 + a] = s[14 + a] + Kv * y
    s[17], s[18], s[19] = Ppp - Kp * Ppp, Ppv - Kp * Ppv, Pvv - Kv * Ppv
    d = abs(wrap(zry - s[13]))
    if d > HALF_PI:
        s[13] = wrap(s[13] + np.float64(PI))
    y = wrap(zry - s[13])
    K = s[20] / (s[20] + np.float64(P['r_ry']))
    s[13] = wrap(s[13] + K * y)
    s[20] = s[20] - K * s[20]
    K = s[21] / (s[21] + np.float64(P['r_dim']))
    for a in range(3):
        s[7 + a] = s[7 + a] + K * (z[a] - s[7 + a])
    s[21] = s[21] - K * s[21]
    s[3] += 1.0
    s[4] = 0.0
    s[5] = score
    s[6] = k
    return abs(d - HALF_PI)


def step(st, rec, dt=1.0, ego=None, P=None):
    """One frame of one stream: st (Stream) is updated in place; rec (topk, 32) records.  Returns (ids (topk,) int32, margin)."""
    P = params() if P is None else P
    metric = METRICS[P['metric']]
    rec = np.asarray(rec, np.float32)
    topk = rec.shape[0]
    frame = st.header[1] + 1.0
    margin = np.inf
    live = st.live()
    for t in live:
        predict(st.slots[t], dt, ego)
        predict_cov(st.slots[t], dt, P)
        st.slots[t, 6] = -1.0
    dets = detections(rec, P['min_score'])
    box = rec[:, 24:31].astype(np.float64)
    # candidates
    cand = []
    for t in live:
        for k in dets:
            if P['class_aware'] and st.slots[t, 1] != np.float64(rec[k, 0]):
                continue
            a = affinity(st.slots[t], box[k], metric)
            if not (metric != 2 and a == 0.0 and P['thresh'] >= 0.0) and a == a:
                margin = min(margin, abs(a - P['thresh']))
            if a > P['thresh']:
                cand.append((a, t, k))
    for i in range(len(cand)):
        for j in range(i + 1, len(cand)):
            if cand[i][1] == cand[j][1] or cand[i][2] == cand[j][2]:
                margin = min(margin, abs(cand[i][0] - cand[j][0]))
    # sequential greedy
    cand.sort(key=lambda c: (-c[0], c[1], c[2]))
    trk_of, det_of = {}, {}
    for a, t, k in cand:
        if t not in det_of and k not in trk_of:
            det_of[t], trk_of[k] = k, t
    owner = {}
    for t in live:
        s = st.slots[t]
        if t in det_of:
            k = det_of[t]
            margin = min(margin, update(s, box[k], np.float64(rec[k, 1]), k, P))
            owner[k] = t
        else:
            s[3] = 0.0
            s[4] += 1.0
            if s[4] > P['max_misses']:
                s[:] = 0.0
    # births
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
        s[13] = wrap(box[k, 6])
        s[17], s[18], s[19], s[20], s[21] = P['p0_pos'], 0.0, P['p0_vel'], P['p0_ry'], P['p0_dim']
        owner[k] = free[n]
    st.header[0] += born
    st.header[1] = frame
    st.header[2] += len(births) - born
    ids = np.zeros(topk, np.int32)
    for k, t in owner.items():
        s = st.slots[t]
        confirmed = s[3] >= P['min_hits'] or frame <= P['min_hits']
        ids[k] = int(s[0]) if confirmed else -int(s[0])
    return ids, margin


def run(sequence, T, P=None, dt=1.0, egos=None):
    """A whole sequence of (B, topk, 32) frames: [(ids (B, topk), tables (B, HEADER + SLOT * T), margins (B,))] per frame."""
    B = sequence[0].shape[0]
    streams = [Stream(T) for _ in range(B)]
    out = []
    for f, rec in enumerate(sequence):
        ego = None if egos is None else egos[f]
        res = [step(streams[b], rec[b], dt, None if ego is None else ego[b], P) for b in range(B)]
        out.append((np.stack([r[0] for r in res]), np.stack([s.table() for s in streams]), np.array([r[1] for r in res])))
    return out
