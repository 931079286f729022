"""CPU: the cases of tests/track_regimes.py really reach the regimes they are named for (asserted on the yardstick's own result),
the yardstick's filter arithmetic against an independent matrix-form Kalman filter in long double, and mutants of the rule that
the new cases catch and the five sequences of tests/track_cases.py cannot see.  No device is used.

The filter check.  tests/track_ref.py restates the scalar lines of include/rtm3d_hip.h, so a mistake shared by the header, the
yardstick and the kernel would pass every comparison between them.  ``matrix_filter`` below is written from the model instead -
F = [[1, dt], [0, 1]], Q = diag(q_pos dt, q_vel dt), H = [1, 0], P' = (I - K H) P, numpy matrices in np.longdouble - and one
track is run through 12 matched frames at dt = 0.1, 2.5 and the per-frame dt of dt_varying with the non-default noise of
track_regimes.NOISE.  Measured here (x86-64, 80-bit long double), the largest relative disagreement of X, v, Ppp, Ppv, Pvv, ry,
Pry, the dimensions, Pdim and the two scalar gains: 6.2e-15 at dt = 0.1, 2.3e-14 at the varying dt, 2.5e-13 at dt = 2.5 (in Ppp
of the first update, where Ppp - Kp Ppp cancels three digits of the 5600 that dt * dt * p0_vel has put there).  Bar = 10 x the
largest = 2.5e-12 relative, far inside the 1e-9 it may never exceed."""
import numpy as np
import pytest

from tests import track_ref as ref
from tests import track_cases as tc
from tests import track_assign_ref as ar
from tests import track_regimes as tr

FILTER_BAR = 2.5e-12
RANGES = 4


def span(slots):
    """The 64-slot ranges (waves of the step kernel) a set of slots lies in."""
    return {int(s) // 64 for s in slots}


# ------------------------------------------------------------------------------------------ the regimes, one check per key
def live_all_ranges(c, res):
    ev = tr.events(c, res)
    assert max(max(e['live']) for e in ev) >= 220 and any(span(e['live']) == set(range(RANGES)) for e in ev)


def dets_all_ranges(c, res):
    dets = tr.detections(c)
    assert max(max(d[0]) for d in dets) == 255 and all(span(d[0]) == set(range(RANGES)) for d in dets)


def matches_upper(c, res):
    s = tr.slots_of(c, res)[:, 0]
    ev = tr.events(c, res)
    # a matched track in a slot >= 192 holding a record slot >= 192, and in every frame 30 matched tracks in the slots >= 128
    assert any(any(t >= 192 and s[f][t, 6] >= 192 for t in e['matched']) for f, e in enumerate(ev))
    assert all(len([t for t in e['matched'] if t >= 128]) >= 30 for e in ev[1:])


def births_frees_three_ranges(c, res):
    ev = tr.events(c, res)
    good = [f for f, e in enumerate(ev) if f > 0 and len(span(e['unmatched'])) >= 3 and len(span(e['free'])) >= 3
            and len(span(e['freed'])) >= 3 and len(span(e['born'])) >= 3]
    assert good, [(len(span(e['unmatched'])), len(span(e['free']))) for e in ev]


def slot_192_reused(c, res):
    ev = tr.events(c, res)
    s = tr.slots_of(c, res)[:, 0]
    assert any(t >= 192 and t in e['freed'] and t in e['born'] and s[f][t, 0] != s[f - 1][t, 0] for f, e in enumerate(ev) for t in e['born'])


def gaps_upper(c, res):
    """A track in a slot >= 128 comes back after max_misses frames with its id, another after max_misses + 1 with a new one."""
    s = tr.slots_of(c, res)[:, 0]
    m = c['params']['max_misses']
    kept = lost = False
    for t in range(128, c['T']):
        for f in range(1, tr.FRAMES - m - 1):
            if s[f][t, 0] != 0 and s[f][t, 4] == 0 and s[f + m][t, 4] == m and s[f + m][t, 0] == s[f][t, 0]:
                kept = kept or (s[f + m + 1][t, 0] == s[f][t, 0] and s[f + m + 1][t, 3] == 1)
                lost = lost or s[f + m + 1][t, 0] != s[f][t, 0]
    assert kept and lost


def greedy_rounds(c, res):
    """A frame whose mutual-best rounds go on for CHAIN rounds, the pairs of the later rounds in slots >= 192."""
    assert all(set(range(192)) <= e['matched'] for e in tr.events(c, res)[1:])        # the lower slots: held and matched throughout
    rounds = tr.greedy_rounds(tr.candidates(c, res, 1))
    assert len(rounds) == tr.CHAIN and all(len(r) == 1 and r[0][0] >= 192 and r[0][1] >= 192 for r in rounds[1:])


def long_path_upper(c, res):
    """Greedy and optimal differ, and under the optimal rule rows >= 192 have augmenting paths of more than one step whose columns
    are record slots >= 192 (lanes >= 48 of the solver's wave); every identity of the chain is kept."""
    g, o = tr.reference(c['name'], 'greedy'), tr.reference(c['name'], 'optimal')
    assert any((a[0] != b[0]).any() for a, b in zip(g, o))
    for f in (1, 6):
        cand = tr.candidates(c, o, f)
        steps = tr.path_steps([x for x in cand if x[1] >= 192], c['params']['thresh'])
        assert max(steps.values()) == tr.CHAIN and min(x[2] for x in cand if x[1] >= 192) >= 192, (f, steps)
        assert np.array_equal(o[f][0], o[0][0]) and not np.array_equal(g[f][0], g[0][0])


def tall(c, res):
    assert c['T'] == 256 and c['topk'] == 5 and all(len(d[0]) == 5 for d in tr.detections(c))
    ev = tr.events(c, res)
    assert max(len(e['live']) for e in ev) == 20 and any(e['born'] and e['matched'] and e['freed'] for e in ev)


def ties_upper(c, res):
    """The header's tie order, read off the yardstick: margin exactly 0 in frame 1, and who got what."""
    assert res[1][2][0] == 0.0 and all(r[2][0] >= tc.MARGIN for f, r in enumerate(res) if f != 1)
    cand = [x for x in tr.candidates(c, res, 1) if x[1] >= 200]
    assert sorted((t, k) for _, t, k in cand) == [(200, 210), (201, 210), (202, 215), (202, 220), (203, 230), (204, 230), (204, 231)]
    assert all(a == -2.5 for a, _, _ in cand) and [len(r) for r in tr.greedy_rounds(tr.candidates(c, res, 1))] == [203, 1]
    ids = res[1][0][0]
    assert [int(ids[k]) for k in (210, 215, 220, 230, 231)] == [201, 203, 206, 204, 205]
    s = tr.slots_of(c, res)[1, 0]
    assert s[201, 6] == -1 and s[201, 4] == 1 and s[205, 0] == 206 and tuple(res[-1][1][0, :3]) == (206.0, 12.0, 0.0)


def wide_dropped(c, res):
    assert c['T'] == 3 and c['topk'] == 256 and res[-1][1][0, 2] >= 1000 and max(max(d[0]) for d in tr.detections(c)) >= 200
    assert any(e['freed'] and e['born'] for e in tr.events(c, res)[1:])           # a slot is freed and taken again


def one_by_one(c, res):
    assert c['T'] == 1 and c['topk'] == 1 and tuple(res[-1][1][0, :3]) == (2.0, 12.0, 1.0)
    assert [int(r[0][0, 0]) for r in res] == [1, 1, 1, 1, 0, 0, -2, -2, 2, 2, 2, 2]     # dropped in frame 6, born in frame 7


def ragged(c, res):
    B, T, topk = c['frames'][0].shape[0], c['T'], c['topk']
    assert B == 3 and all(v % n for v in (T, topk) for n in (4, 32, 64)) and (T * topk) % 256
    fill = [max(len(e['live']) for e in tr.events(c, res, b)) for b in range(B)]
    assert fill[0] == T and fill[0] > 4 * fill[1] > 0 and fill[1] > 4 * fill[2] > 0 and res[-1][1][0, 2] > 0


def empty_stream_start(c, res):
    assert all(not r[0][2].any() and not r[1][2][ref.HEADER:].any() for r in res[:3]) and res[3][0][2].any() and res[0][0][0].any()


def slot_T_minus_1(c, res):
    ev = tr.events(c, res)
    assert any(c['T'] - 1 in e['born'] for e in ev) and any(c['T'] - 1 in e['freed'] for e in ev)


def dt_is(values):
    def check(c, res):
        assert sorted(set(c['dts'])) == sorted(values)
    return check


def noise_all(c, res):
    P = c['params']
    q, r, p0 = [P[k] for k in ('q_pos', 'q_vel', 'q_ry', 'q_dim')], [P[k] for k in ('r_pos', 'r_ry', 'r_dim')], \
        [P[k] for k in ('p0_pos', 'p0_vel', 'p0_ry', 'p0_dim')]
    assert len(set(q)) == 4 and min(q) > 0 and len(set(r)) == 3 and 1.0 not in r and len(set(p0)) == 4
    s = tr.slots_of(c, res)
    assert ((s[..., 0] != 0) & (s[..., 4] == 2)).any()                          # two predictions in a row somewhere
    assert all(d != 1.0 for d in c['dts'])


def ego_general(c, res):
    e = c['egos']
    assert e.shape == (tr.FRAMES, 2, 12) and (np.abs(e) > 1e-4).all() and (np.abs(e - 1.0) > 1e-6).all()
    R = e.reshape(tr.FRAMES, 2, 3, 4)[..., :3]
    assert np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-12 and np.abs(R[..., 0, 1] - R[..., 1, 0]).min() > 0.02


def max_misses_0(c, res):
    s = tr.slots_of(c, res)[:, 0]
    assert c['params']['max_misses'] == 0 and not ((s[..., 0] != 0) & (s[..., 4] > 0)).any() and res[-1][1][0, 0] == 7
    assert any(e['freed'] for e in tr.events(c, res))


def min_hits_0(c, res):
    assert c['params']['min_hits'] == 0 and all((r[0] >= 0).all() for r in res) and any((r[0] > 0).any() for r in res)


def min_hits_1(c, res):
    # confirmed at birth, in a late frame too
    assert c['params']['min_hits'] == 1 and all((r[0] >= 0).all() for r in res) and any(e['born'] for e in tr.events(c, res)[5:])


def max_misses_3(c, res):
    s = tr.slots_of(c, res)[:, 0]
    assert ((s[..., 0] != 0) & (s[..., 4] == 3)).any() and res[-1][1][0, 0] == 7 and len(tr.events(c, res)[7]['born']) == 1
    back = [t for t in range(c['T']) if s[6][t, 4] == 3 and s[7][t, 4] == 0 and s[7][t, 0] == s[6][t, 0] != 0]
    assert back


def classes_4(c, res):
    s = tr.slots_of(c, res)[:, 0]
    assert c['params']['class_aware'] and set(s[-1][s[-1][:, 0] != 0][:, 1].tolist()) == {0.0, 1.0, 2.0, 3.0}
    blind = tr.run(dict(c, params=dict(c['params'], class_aware=False)), 'greedy')
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(res, blind))      # the classes decide here
    assert res[-1][1][0, 0] == 12                                               # and with them every object keeps its one id


def score_0(c, res):
    rec = c['frames'][5][0]
    zero = [k for k in range(c['topk']) if rec[k, 31] == 2 and rec[k, 1] == 0]
    assert c['params']['min_score'] == 0 and len(zero) == 2 and all(res[5][0][0][k] > 0 for k in zero)
    assert ((rec[:, 31] == 2) & (rec[:, 1] < 0)).any()                          # and one below it


def yaw_outside(c, res):
    ry = np.concatenate([f[0, f[0, :, 31] == 2, 30] for f in c['frames']])
    assert (ry > 6.5).any() and (ry < -9.0).any() and (ry > 20.0).any() and res[-1][1][0, 0] == 6
    s = tr.slots_of(c, res)[:, 0]
    assert (s[..., 13] >= -np.pi).all() and (s[..., 13] < np.pi).all()


def nonfinite(c, res):
    """The header's sentence, on the yardstick: every bad box is born, is never matched, is freed after max_misses + 1 frames,
    ids keep counting, and the finite objects keep one id each."""
    s = tr.slots_of(c, res)[:, 0]
    m = c['params']['max_misses']
    bad_born = 0
    for f in range(tr.FRAMES):
        for t in range(c['T']):
            v = s[f][t]
            if v[0] != 0 and not (np.isfinite(v[7:14]).all() and (v[7:10] > 0).all()):
                assert v[6] == -1 or v[2] == 1, (f, t)                       # matched to nothing after its birth
                assert v[2] <= m + 1
                bad_born += v[2] == 1
                if v[2] == m + 1:
                    assert s[f + 1][t, 0] != v[0]                            # freed in the next frame
    assert bad_born == 4 + 2 + 4 + 2 and res[-1][1][0, 0] == 3 + bad_born and res[-1][1][0, 2] == 0
    ids = np.stack([r[0][0] for r in res])
    assert (ids[:, 1] == ids[0, 1]).all() and (ids[:, 3] == ids[0, 3]).all() and ids[0, 1] > 0 and ids[0, 3] > 0
    assert ids[6, 5] != 0 and (np.abs(ids[6:, 5]) == abs(ids[6, 5])).all() and abs(ids[6, 5]) == 12     # born between bad ones
    assert not ids[2, 7] and not ids[3, 2]                                   # a NaN score is no detection
    assert np.isnan(s[2][:, 10]).any() and np.isnan(s[2][:, 13]).any() and (s[2][:, 8] == 0).any() and (s[2][:, 9] < 0).any()


REGIMES = {
    'live_all_ranges': live_all_ranges, 'dets_all_ranges': dets_all_ranges, 'matches_upper': matches_upper,
    'births_frees_three_ranges': births_frees_three_ranges, 'slot_192_reused': slot_192_reused, 'gaps_upper': gaps_upper,
    'greedy_rounds': greedy_rounds, 'long_path_upper': long_path_upper, 'tall': tall, 'ties_upper': ties_upper, 'wide_dropped': wide_dropped,
    'one_by_one': one_by_one, 'ragged': ragged, 'empty_stream_start': empty_stream_start, 'slot_T_minus_1': slot_T_minus_1,
    'dt_small': dt_is([0.1]), 'dt_large': dt_is([2.5]), 'dt_varying': dt_is([0.04, 0.1, 0.5]), 'noise_all': noise_all,
    'ego_general': ego_general, 'max_misses_0': max_misses_0, 'min_hits_0': min_hits_0, 'min_hits_1': min_hits_1,
    'max_misses_3': max_misses_3, 'classes_4': classes_4, 'score_0': score_0, 'yaw_outside': yaw_outside, 'nonfinite': nonfinite,
}


def test_every_regime_has_a_case():
    keys = {n: tr.case(n)[0]['regimes'] for n in tr.ALL}
    table = {k: [n for n in tr.ALL if k in keys[n]] for k in REGIMES}
    assert all(table.values()), [k for k, v in table.items() if not v]
    assert all(keys[n] and set(keys[n]) <= set(REGIMES) for n in tr.ALL)
    assert set(tr.ALL) == {n for v in table.values() for n in v}


@pytest.mark.parametrize('name', tr.ALL)
def test_case_reaches_its_regimes(name):
    c, res = tr.case(name)
    assert len(c['frames']) == tr.FRAMES == 12 and len(c['dts']) == 12
    assert sorted(res) == (['greedy'] if name in tr.GREEDY_ONLY else ['greedy', 'optimal'])
    for a in res:
        assert len(res[a]) == 12 and min(float(r[2].min()) for f, r in enumerate(res[a]) if f not in c['tie_frames']) >= tc.MARGIN, (name, a)
    for key in c['regimes']:
        REGIMES[key](c, res['greedy'])
        if key != 'long_path_upper' and 'optimal' in res:
            REGIMES[key](c, res['optimal'])
    sizes = dict(full_256=(1, 256, 256), chain_upper=(1, 256, 256), ties_upper=(1, 256, 256), tall=(1, 256, 5), wide=(1, 3, 256), one_by_one=(1, 1, 1),
                 ragged_streams=(3, 193, 129), ego_general=(2, 16, 12), nonfinite_boxes=(1, 8, 8))
    assert (c['frames'][0].shape[0], c['T'], c['topk']) == sizes.get(name, (1, 16, 12))
    assert all(f.shape == (sizes.get(name, (1, 16, 12))[0], c['topk'], 32) and f.dtype == np.float32 for f in c['frames'])


def test_run_is_the_yardsticks_own_run_at_one_dt():
    c = tr.case('dt_large')[0]
    for a, want in (('greedy', ref.run(c['frames'], c['T'], c['params'], 2.5, None)), ('optimal', ar.run(c['frames'], c['T'], c['params'], 2.5, None))):
        for g, w in zip(tr.reference('dt_large', a), want):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(g, w[:3]))


# ------------------------------------------------------------------------------------------ the independent filter
def matrix_filter(z, dts, P):
    """Textbook constant-velocity Kalman filters in long double: per position axis the state (x, v) with the shared 2 x 2 covariance,
    a scalar random-walk filter for ry and one for the dimensions.  z (F, 7) = h w l X Y Z ry per frame.  Per frame the values
    compared: X Y Z, vx vy vz, Ppp Ppv Pvv, ry, Pry, h w l, Pdim, gain of ry, gain of the dimensions."""
    L = np.longdouble
    I, H = np.eye(2, dtype=L), np.array([[1, 0]], L)
    x = np.array([[z[0][3 + a], 0] for a in range(3)], L).T                   # (2, 3): the three axes side by side
    C = np.array([[P['p0_pos'], 0], [0, P['p0_vel']]], L)
    ry, Cry, dim, Cdim = L(z[0][6]), L(P['p0_ry']), np.array(z[0][:3], L), L(P['p0_dim'])
    out = []
    for f in range(1, len(z)):
        dt = L(dts[f])
        F = np.array([[1, dt], [0, 1]], L)
        Q = np.array([[L(P['q_pos']) * dt, 0], [0, L(P['q_vel']) * dt]], L)
        x, C = F @ x, F @ C @ F.T + Q
        Cry, Cdim = Cry + L(P['q_ry']) * dt, Cdim + L(P['q_dim']) * dt
        K = C @ H.T / (H @ C @ H.T + L(P['r_pos']))
        x = x + K @ (np.array([z[f][3:6]], L) - H @ x)
        C = (I - K @ H) @ C
        Kr, Kd = Cry / (Cry + L(P['r_ry'])), Cdim / (Cdim + L(P['r_dim']))
        ry, Cry = ry + Kr * (L(z[f][6]) - ry), (1 - Kr) * Cry
        dim, Cdim = dim + Kd * (np.array(z[f][:3], L) - dim), (1 - Kd) * Cdim
        out.append(np.concatenate([x[0], x[1], [C[0, 0], C[0, 1], C[1, 1], ry, Cry], dim, [Cdim, Kr, Kd]]))
    return np.array(out)


@pytest.mark.parametrize('which', ['dt_small', 'dt_large', 'dt_varying'])
def test_yardstick_filter_equals_a_matrix_kalman_filter_in_long_double(which):
    assert np.finfo(np.longdouble).eps < 1e-18, 'long double is no wider than double here'
    c = tr.case(which)[0]
    dts = c['dts']
    P = ref.params(metric='dist', thresh=-1e3, **tr.NOISE)
    rng = np.random.Generator(np.random.PCG64(7))
    pos, vel = np.array([2.0, 1.0, 20.0]), np.array([0.8, -0.3, 1.1])
    rec, t = [], 0.0
    for f in range(12):
        t += dts[f] if f else 0.0
        r = np.zeros((1, 32), np.float32)
        r[0, 1], r[0, 31] = 0.9, 2
        r[0, 24:31] = np.concatenate([[1.5, 1.7, 4.0] + rng.normal(0, 0.02, 3), pos + vel * t + rng.normal(0, 0.03, 3), [0.5 + 0.02 * f]])
        rec.append(r)
    z = [r[0, 24:31].astype(np.float64) for r in rec]
    want = matrix_filter(z, dts, P)
    st = ref.Stream(1)
    worst, where = 0.0, None
    names = 'X Y Z vx vy vz Ppp Ppv Pvv ry Pry h w l Pdim Kry Kdim'.split()
    for f in range(12):
        pre = st.slots[0].copy()
        ids, _ = ref.step(st, rec[f], dts[f], None, P)
        assert abs(int(ids[0])) == 1
        if f == 0:
            continue
        ref.predict_cov(pre, dts[f], P)                                        # the yardstick's own predicted variances: its gains
        s = st.slots[0]
        got = np.concatenate([s[10:13], s[14:17], s[17:20], [s[13], s[20]], s[7:10], [s[21]], [pre[20] / (pre[20] + P['r_ry']),
                                                                                            pre[21] / (pre[21] + P['r_dim'])]])
        rel = np.abs((got.astype(np.longdouble) - want[f - 1]) / want[f - 1]).astype(np.float64)
        assert np.all(want[f - 1] != 0)
        if rel.max() > worst:
            worst, where = float(rel.max()), (f, names[int(rel.argmax())])
        assert rel.max() <= FILTER_BAR, (which, f, names[int(rel.argmax())], float(rel.max()))
    print('%s: largest relative disagreement of track_ref with the long-double matrix filter %.3g at %s (bar %g)' % (which, worst, where, FILTER_BAR))
    assert FILTER_BAR <= 1e-9


# ------------------------------------------------------------------------------------------ mutants
class Rule(object):
    """A copy of the yardstick's frame step (greedy), cut into the functions a mutant overrides.  Unmutated it is tests/track_ref.step
    bit for bit (test_the_copy_of_the_rule_is_the_yardstick)."""

    def predict(self, s, dt, ego):
        ref.predict(s, dt, ego)

    def predict_cov(self, s, dt, P):
        ref.predict_cov(s, dt, P)

    def candidate(self, t, k):
        return True

    def free_slots(self, st):
        return [t for t in range(st.T) if st.slots[t, 0] == 0]

    def placements(self, births, free):
        """[(record slot, track slot, rank)]: the n-th unmatched detection into the n-th free slot."""
        return [(k, free[n], n) for n, k in enumerate(births) if n < len(free)]

    def step(self, st, rec, dt, ego, P):
        metric = ref.METRICS[P['metric']]
        rec = np.asarray(rec, np.float32)
        frame = st.header[1] + 1.0
        live = st.live()
        for t in live:
            self.predict(st.slots[t], dt, ego)
            self.predict_cov(st.slots[t], dt, P)
            st.slots[t, 6] = -1.0
        dets = ref.detections(rec, P['min_score'])
        box = rec[:, 24:31].astype(np.float64)
        cand = []
        for t in live:
            for k in dets:
                if (P['class_aware'] and st.slots[t, 1] != np.float64(rec[k, 0])) or not self.candidate(t, k):
                    continue
                a = ref.affinity(st.slots[t], box[k], metric)
                if a > P['thresh']:
                    cand.append((a, t, k))
        det_of = ar.greedy(cand, np.float64(P['thresh']))[0]
        trk_of = {k: t for t, k in det_of.items()}
        owner = {}
        for t in live:
            s = st.slots[t]
            if t in det_of:
                ref.update(s, box[det_of[t]], np.float64(rec[det_of[t], 1]), det_of[t], P)
                owner[det_of[t]] = t
            else:
                s[3] = 0.0
                s[4] += 1.0
                if s[4] > P['max_misses']:
                    s[:] = 0.0
        free = self.free_slots(st)
        births = [k for k in dets if k not in trk_of]
        born = min(len(births), len(free))
        for k, t, n in self.placements(births, free):
            s = st.slots[t]
            s[:] = 0.0
            s[0] = st.header[0] + (n + 1)
            s[1] = rec[k, 0]
            s[2], s[3], s[4], s[5], s[6] = 1.0, 1.0, 0.0, rec[k, 1], k
            s[7:13] = box[k, :6]
            s[13] = ref.wrap(box[k, 6])
            s[17], s[18], s[19], s[20], s[21] = P['p0_pos'], 0.0, P['p0_vel'], P['p0_ry'], P['p0_dim']
            owner[k] = t
        st.header[0] += born
        st.header[1] = frame
        st.header[2] += len(births) - born
        ids = np.zeros(rec.shape[0], np.int32)
        for k, t in owner.items():
            s = st.slots[t]
            if s[6] == k:                                                       # (a mutant may place two births in one slot)
                ids[k] = int(s[0]) if (s[3] >= P['min_hits'] or frame <= P['min_hits']) else -int(s[0])
        return ids

    def differs(self, c, want, same=False):
        """Run the sequence frame by frame against the yardstick's result.  same = False: the first frame whose ids differ or whose
        table differs by more than 1e-6 (None if there is none); same = True: assert that every frame is equal bit for bit."""
        B = c['frames'][0].shape[0]
        dts = c.get('dts', [c.get('dt', 1.0)] * len(c['frames']))
        streams = [ref.Stream(c['T']) for _ in range(B)]
        with np.errstate(invalid='ignore'):
            for f, rec in enumerate(c['frames']):
                ids = np.stack([self.step(streams[b], rec[b], dts[f], None if c['egos'] is None else c['egos'][f][b], c['params'])
                                for b in range(B)])
                table = np.stack([s.table() for s in streams])
                if same:
                    assert ids.tobytes() == want[f][0].tobytes() and table.tobytes() == want[f][1].tobytes(), (c['name'], f)
                elif not np.array_equal(ids, want[f][0]) or not np.array_equal(np.isnan(table), np.isnan(want[f][1])) \
                        or np.nanmax(np.abs(table - want[f][1])) > 1e-6:
                    return f
        return None


class QposDtSquared(Rule):
    def predict_cov(self, s, dt, P):
        ref.predict_cov(s, dt, dict(P, q_pos=np.float64(P['q_pos']) * np.float64(dt)))


class QryWithoutDt(Rule):
    def predict_cov(self, s, dt, P):
        ref.predict_cov(s, dt, dict(P, q_ry=0.0))
        s[20] = s[20] + np.float64(P['q_ry'])


class StepWithoutDt(Rule):
    def predict(self, s, dt, ego):
        ref.predict(s, 1.0, ego)                                                # X + 1.0 * vx is X + vx


class EgoSwapped(Rule):
    def predict(self, s, dt, ego):
        if ego is not None:
            ego = np.array(ego, np.float64)
            ego[[1, 4]] = ego[[4, 1]]
        ref.predict(s, dt, ego)


class UpperRecordsNoCandidates(Rule):
    def candidate(self, t, k):
        return k < 128


class UpperSlotsNotFree(Rule):
    def free_slots(self, st):
        return [t for t in Rule.free_slots(self, st) if t < 192]


class BirthRankPerRange(Rule):
    """The rank of a birth without the births of the third 64-slot range: the prefix over the waves stops after two.  (Ranked
    within its own range from the second range on, the mutant is caught by dense_3d of the old suite, whose births of frame 0 lie
    in the record slots 0..98; what the old suite cannot see starts at record slot 128.)"""

    def placements(self, births, free):
        out = []
        for k in births:
            n = sum(1 for j in births if j < k and not (k // 64 == 3 and j // 64 == 2))
            if n < len(free):
                out.append((k, free[n], n))
        return out


MUTANTS = {          # mutant -> the new cases that must catch it
    QposDtSquared: ('dt_small', 'dt_large', 'dt_varying'), QryWithoutDt: ('dt_small', 'dt_large', 'dt_varying'),
    StepWithoutDt: ('dt_small', 'dt_large', 'dt_varying', 'ego_general'), EgoSwapped: ('ego_general',),
    UpperRecordsNoCandidates: ('full_256', 'chain_upper'), UpperSlotsNotFree: ('full_256', 'chain_upper'),
    BirthRankPerRange: ('full_256',),
}


@pytest.mark.parametrize('name', tr.ALL)
def test_the_copy_of_the_rule_is_the_yardstick(name):
    Rule().differs(tr.case(name)[0], tr.reference(name, 'greedy'), same=True)


@pytest.mark.parametrize('mutant', list(MUTANTS), ids=[m.__name__ for m in MUTANTS])
def test_mutants_are_caught_by_the_new_cases_and_missed_by_the_old(mutant):
    for name in MUTANTS[mutant]:
        f = mutant().differs(tr.case(name)[0], tr.reference(name, 'greedy'))
        assert f is not None, (mutant.__name__, name)
        print('%s: caught by %s in frame %d' % (mutant.__name__, name, f))
    for name in tc.NAMES:                                                       # what the old suite could not see
        c, want = tc.case(name)
        mutant().differs(c, want, same=True)
