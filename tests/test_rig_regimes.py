"""CPU: the cases of tests/rig_regimes.py really are in the regimes of csrc/rig.hip they are named for - asserted on
``schedule(case)``, the host model of the three kernels - the model agrees with the yardstick tests/rig_ref.py on every case
(which positions are representatives, who joins whom, the map, the counters), and deliberately wrong variants of the model
disagree with the yardstick on the cases that are there to tell them apart.  No device is used, and nothing broken is built for
one: the variants exist in the host model only."""
import numpy as np
import pytest

from tests import rig_ref as ref
from tests import rig_regimes as rr

SORT = {1: (64, 1), 63: (64, 1), 64: (64, 1), 65: (128, 1), 128: (128, 1), 129: (256, 1), 256: (256, 1), 257: (512, 1), 512: (512, 1),
        513: (1024, 2), 1024: (1024, 2), 1025: (2048, 4), 2047: (2048, 4), 2048: (2048, 4)}
N_OF = {'sort_n1_63_64_65': [1, 63, 64, 65], 'sort_n128_to_513': [128, 129, 256, 257, 512, 513], 'sort_n1024': [1024],
        'star_dense_2048_mean': [2048, 2048, 2047, 300], 'star_n1025_best': [2048, 1025]}


def bits(x):
    return bin(x).count('1')


def kept(c, r=0):
    """(C, topk) bool: the candidates of rig r, by the header's sentence."""
    rec = c['rec'][r * c['C']:(r + 1) * c['C']]
    with np.errstate(invalid='ignore'):
        return (rec[..., 31] == 2) & (rec[..., 1].astype(np.float64) >= c['params']['min_score'])


def scores(c, s, r=0):
    rec = c['rec'][r * c['C']:(r + 1) * c['C']]
    return [rec[cam, k, 1] for cam, k in s['order']]


# ------------------------------------------------------------------------------------------ the regimes, one check per key
def sort_sizes(c, sch, want):
    assert [s['n'] for s in sch] == N_OF[c['name']]
    for s in sch:
        if s['n'] in SORT:
            assert (s['M'], s['pairs']) == SORT[s['n']], (c['name'], s['n'])
    if c['name'] == 'star_dense_2048_mean':
        assert c['C'] * c['topk'] == 2048 and kept(c, 0).all() and kept(c, 1).all() and int((~kept(c, 2)).sum()) == 1     # n = N: nothing padded


def scattered(c, sch, want):
    """Candidates and slots that are none in every 64-slot range (wave of the ballot compaction) of several 256-slot passes."""
    N = c['C'] * c['topk']
    assert N > 256
    some = [r for r in range(c['R']) if 64 <= sch[r]['n'] < N - 64]
    assert some
    for r in some:
        k = kept(c, r).reshape(N)
        full = range(N // 64)
        assert all(k[64 * w:64 * w + 64].any() and not k[64 * w:64 * w + 64].all() for w in full), (c['name'], r)
        # and the order is no copy of the slot order: neighbours in the order come from other waves
        q = np.array([cam * c['topk'] + slot for cam, slot in sch[r]['order']])
        assert (np.abs(np.diff(q)) >= 64).mean() > 0.5


def odd_stride(c, sch, want):
    assert (c['C'] * c['topk']) % 2 == 1 and c['R'] >= 2 and sum(s['n'] > 0 for s in sch) >= 2


def star(c, sch, want):
    s = sch[0]
    assert s['n'] == 2048 and s['ncl'] == 1 and s['largest'] == 2048 and s['rep_of'] == [0] * 2048
    assert s['rounds'] == [64] + [0] * 31 and max(s['chunk_dist']) == 31 and s['taken'].count('push') == 1984 and s['taken'].count('settle') == 63
    assert all(s['rows'][i] == (1 << i) - 1 for i in range(2048))                 # every link word of every row is set
    assert tuple(want['info'][0, 0, 2:]) == (2048, 0xffff) and tuple(want['n'][0]) == (1, 0)
    assert c['params']['merge'] == ('mean' if c['name'].endswith('mean') else 'best')


def dense_2048(c, sch, want):
    s = sch[1] if c['name'] == 'star_dense_2048_mean' else sch[0]
    links = sum(bits(x) for x in s['rows'])
    on = c['params']['class_aware']
    assert s['n'] == 2048 and c['params']['cross_only'] == on
    assert (1300 if on else 3000) <= links <= 5000 and s['ncl'] >= 600 and s['largest'] >= (5 if on else 9) and max(s['chunk_dist']) == 31
    assert {1, 2} <= set(s['rounds']) and s['taken'].count('push') > 800 and s['taken'].count('settle') >= 20
    if on:
        rec = c['rec'].reshape(-1, 32)
        assert set(rec[rec[:, 31] == 2][:, 0].tolist()) == {0.0, 1.0}


def capacity_overflow(c, sch, want):
    assert any(s['ncl'] > s['cap'] + 100 for s in sch) and (want['map'] == -2).any() and (want['n'][:, 1] > 100).any()


def ties(c, sch, want):
    s = sch[0]
    sc = np.array(scores(c, s))
    cam = np.array([o[0] for o in s['order']])
    tied = np.array([np.sum(sc == v) > 1 for v in sc])
    assert tied.sum() >= s['n'] / 8 and tied.sum() >= 60
    same = sc[1:] == sc[:-1]
    assert (same & (cam[1:] == cam[:-1])).sum() >= 5 and (same & (cam[1:] != cam[:-1])).sum() >= 5      # within a camera, across cameras
    assert any(len(cl) > 1 and len({c['rec'][m[0], m[1], 1] for m in cl}) < len(cl) for cl in s['clusters'])   # a tie inside a cluster


def keys_special(c, sch, want):
    s = sch[0]
    sc = np.array(scores(c, s))
    q = [cam * c['topk'] + k for cam, k in s['order']]
    assert c['params']['min_score'] == -np.inf and c['params']['merge'] == 'best'
    assert sc[0] == np.inf and sc[1] == np.inf and q[:2] == [40, 105] and sc[-1] == -np.inf and sc[-2] == -np.inf and q[-2:] == [41, 100]
    assert (sc < 0).sum() >= 30 and (sc > 0).sum() >= 30 and list(sc) == sorted(sc, reverse=True)
    zero = [i for i in range(s['n']) if sc[i] == 0]
    assert [q[i] for i in zero] == [3, 5, 7, 9] and [bool(np.signbit(sc[i])) for i in zero] == [True, False, False, True]
    tiny = np.float32(2.0 ** -126)
    assert ((sc > 0) & (sc < tiny)).any() and ((sc < 0) & (sc > -tiny)).any()     # denormals of both signs
    rec = c['rec'].reshape(-1, 32)
    assert ((rec[:, 31] == 2) & np.isnan(rec[:, 1])).any() and s['n'] == int(((rec[:, 31] == 2) & ~np.isnan(rec[:, 1])).sum())
    assert np.isinf(want['out'][0, 0, 1]) and np.isfinite(want['box'][0]).all()


def min_score_edge(c, sch, want):
    ms = c['params']['min_score']
    rec = c['rec'].reshape(-1, 32)
    at, under = (rec[:, 31] == 2) & (rec[:, 1].astype(np.float64) == ms), (rec[:, 31] == 2) & (rec[:, 1] == rr.below(ms))
    assert at.sum() >= 5 and under.sum() >= 5 and np.float64(rr.below(ms)) < ms == np.float64(np.nextafter(rr.below(ms), np.float32(1)))
    m = want['map'].reshape(-1)
    assert (m[at] >= 0).all() and (m[under] == -1).all()


def min_score_inf(c, sch, want):
    rec = c['rec'].reshape(-1, 32)
    assert c['params']['min_score'] == np.inf and sch[0]['n'] == 0 and sch[0]['rounds'] == []
    assert ((rec[:, 31] == 2) & np.isfinite(rec[:, 1])).sum() >= 10 and rec[:, 1][np.isfinite(rec[:, 1])].max() == np.finfo(np.float32).max
    assert (want['map'] == -1).all() and not want['out'].any() and not want['info'].any() and tuple(want['n'][0]) == (0, 0)


def link_every_word(c, sch, want):
    s, i = sch[0], c['row']
    row = s['rows'][i]
    words = [(row >> (64 * w)) & rr.M64 for w in range((i >> 6) + 1)]
    assert i == 329 and len(words) == 6 and all(words)
    assert all(w & 1 and (w >> 63) & 1 for w in words[:5]) and words[5] & 1 and (row >> (i - 1)) & 1
    assert s['rep_of'][i] == 0 and s['chunk_dist'][i] == 5 and all(s['rep_of'][p] == 0 for p in c['cols'])


def class_nan(c, sch, want):
    s = sch[0]
    cls = [c['rec'][cam, k, 0] for cam, k in s['order']]
    assert np.isnan(cls[0]) and np.isnan(cls[1]) and s['rows'][1] == 0 and s['sizes'] == [1, 1, 2, 1]
    a, b = s['order'][0], s['order'][1]
    assert a[0] != b[0] and c['rec'][a][24:31].tobytes() == c['rec'][b][24:31].tobytes()         # copies of one box in two cameras
    assert np.isnan(want['out'][0, 0, 0]) and np.isnan(want['out'][0, 1, 0])
    blind = ref.fuse(c['rec'], c['ext'], 1, c['C'], dict(c['params'], class_aware=False), c['cap'])
    assert [len(x) for x in blind['clusters'][0]] == [2, 3]


def cross_only_one_camera(c, sch, want):
    s = sch[0]
    assert c['params']['cross_only'] and {o[0] for o in s['order']} == {1} and s['ncl'] == s['n'] == 12 and not any(s['rows'])
    free = ref.fuse(c['rec'], c['ext'], 1, c['C'], dict(c['params'], cross_only=False), c['cap'])
    assert [len(x) for x in free['clusters'][0]] == [3, 3, 3, 3]


def iou_bad_boxes(c, sch, want):
    s = sch[0]
    assert c['params']['metric'] == 'bev' and s['sizes'] == [2] + [1] * 8
    box = np.array([c['rec'][cam, k, 24:31] for cam, k in s['order']])
    assert (box[:, 1] == 0).sum() == 2 and (box[:, 1] < 0).sum() == 2 and np.isnan(box[:, 3]).sum() == 2 and np.isinf(box[:, 2]).sum() == 2
    assert (~np.isfinite(want['box'][0])).any()


def reach_bar(c, sch, want):
    s = sch[0]
    assert s['sizes'] == [2, 1, 1, 1, 1] and bits(s['rows'][1]) == 1
    b = [ref.transform(c['rec'][cam, k, 24:31].astype(np.float64), c['ext'][0, cam]) for cam, k in s['order']]
    reach = [0.5 * np.hypot(b[i][1], b[i][2]) + 0.5 * np.hypot(b[i + 1][1], b[i + 1][2]) for i in (0, 2, 4)]
    gap = [abs(b[i][3] - b[i + 1][3]) for i in (0, 2, 4)]
    assert 0 < reach[0] - gap[0] < 0.05 and 0 < gap[1] - reach[1] < 0.05 and gap[2] < reach[2] - 0.3       # both sides of the bar, close to it
    a = [ref.affinity(b[i], b[i + 1], 0) for i in (0, 2, 4)]
    assert 2e-5 < a[0] < 1e-3 and a[1] == 0.0 and a[2] == 0.0 and c['params']['thresh'] == 1e-5


def chain_parity0(c, sch, want):
    s = sch[0]
    assert s['rounds'][:3] == [64, 64, 64] and s['n'] % 4 != 0
    assert all(s['rep_of'][p] == p - p % 2 for p in range(210)) and s['taken'][64] == 'rep' and s['taken'][128] == 'rep'
    assert (s['rows'][64] >> 63) & 1 and (s['rows'][128] >> 127) & 1              # the bit at j = i - 1 across a word boundary
    assert 'push' not in s['taken']


def chain_parity1(c, sch, want):
    s = sch[0]
    assert s['rep_of'][0] == 0 and s['rows'][1] == 0 and all(s['rep_of'][p] == p - (p + 1) % 2 for p in range(1, 211))
    assert s['taken'][63] == 'rep' and s['taken'][64] == 'push' and s['rep_of'][64] == 63 and s['taken'][128] == 'push' and s['taken'][192] == 'push'
    assert s['rounds'][:3] == [63, 63, 63] and s['taken'][65] == 'rep'


def two_reps_other_chunks(c, sch, want):
    s = sch[0]
    for x in (140, 75):
        assert (s['rows'][x] >> 3) & 1 and (s['rows'][x] >> 70) & 1 and s['rep_of'][x] == 3 and s['taken'][x] == 'push'
    assert s['rep_of'][3] == 3 and s['rep_of'][70] == 70 and s['chunk_dist'][140] == 2 and s['chunk_dist'][75] == 1
    assert max(s['rounds']) == 10


def two_reps_same_chunk(c, sch, want):
    s = sch[0]
    for x in (20, 100):
        assert (s['rows'][x] >> 5) & 1 and (s['rows'][x] >> 9) & 1 and s['rep_of'][x] == 5
    assert s['rep_of'][5] == 5 and s['rep_of'][9] == 9 and s['taken'][20] == 'settle' and s['taken'][100] == 'push'


def member_link(c, sch, want):
    s, x = sch[0], c['x']
    assert s['rows'][x] == 1 << 10 and s['rep_of'][10] == 2 and s['rep_of'][x] == x and s['taken'][x] == 'rep'
    assert (x >> 6) - (10 >> 6) == (0 if c['name'] == 'member_link_same_chunk' else 1)


def dense_300(c, sch, want):
    s = sch[0]
    assert s['n'] == 300 and c['params']['metric'] in ('bev', 'iou3d') and sum(bits(x) for x in s['rows']) >= 100
    assert s['largest'] >= 4 and max(s['chunk_dist']) == 4 and s['taken'].count('push') >= 50 and s['taken'].count('settle') >= 10
    box = c['rec'][c['rec'][..., 31] == 2][:, 24:27]
    assert (box > 1.3).all() and (box < 4.5).all()
    assert np.abs(c['ext'].reshape(-1, 3, 4)[:, :, :3] - np.eye(3)).max() > 0.5    # real extrinsics: cameras looking all round


def cap_exact(c, sch, want):
    s = sch[0]
    assert s['ncl'] == s['cap'] == 12 and tuple(want['n'][0]) == (12, 0) and not (want['map'] == -2).any() and s['n'] == 27


def cap_plus_one(c, sch, want):
    s = sch[0]
    assert s['ncl'] == s['cap'] + 1 == 13 and tuple(want['n'][0]) == (12, 1) and s['sizes'][-1] == 4 and int((want['map'] == -2).sum()) == 4


def cap_one(c, sch, want):
    s = sch[0]
    assert s['cap'] == 1 and s['ncl'] == 4 and tuple(want['n'][0]) == (1, 3) and want['out'].shape == (1, 1, 32)
    assert int((want['map'] == -2).sum()) == s['n'] - s['sizes'][0] and int((want['map'] == 0).sum()) == s['sizes'][0] and max(s['sizes'][1:]) >= 2


def cap_256_n4(c, sch, want):
    s = sch[0]
    assert s['cap'] == 256 > c['C'] * c['topk'] == 4 == s['n'] and s['ncl'] == 3 and not want['out'][0, 3:].any() and not want['info'][0, 3:].any()


def cluster_sizes(c, sch, want):
    s = sch[0]
    assert sorted(s['sizes']) == [1, 1, 1, 2, 3, 5, 70] and s['n'] % 4 == 3
    assert any(p % 4 and n > 1 for p, n in zip(s['reps'], s['sizes']))            # a representative off the int4 grid of the walk
    assert max(s['chunk_dist']) == 1


def heading_fold(c, sch, want):
    s = sch[0]
    big = max(s['clusters'], key=len)
    ry = [ref.transform(c['rec'][m][24:31].astype(np.float64), c['ext'][0, m[0]])[6] for m in big]
    d = np.array([ref.wrap(v - ry[0]) for v in ry[1:]])
    assert (d > ref.HALF_PI + 0.1).sum() >= 8 and (d < -ref.HALF_PI - 0.1).sum() >= 8 and (np.abs(d) < ref.HALF_PI - 0.1).sum() >= 8
    assert c['params']['merge'] == 'mean' and want['margin'] >= rr.MARGIN


REGIMES = {
    'sort_sizes': sort_sizes, 'scattered': scattered, 'odd_stride': odd_stride, 'star': star, 'dense_2048': dense_2048,
    'capacity_overflow': capacity_overflow, 'ties': ties, 'keys_special': keys_special, 'min_score_edge': min_score_edge,
    'min_score_inf': min_score_inf, 'link_every_word': link_every_word, 'class_nan': class_nan, 'cross_only_one_camera': cross_only_one_camera,
    'iou_bad_boxes': iou_bad_boxes, 'reach_bar': reach_bar, 'chain_parity0': chain_parity0, 'chain_parity1': chain_parity1,
    'two_reps_other_chunks': two_reps_other_chunks, 'two_reps_same_chunk': two_reps_same_chunk, 'member_link_same_chunk': member_link,
    'member_link_earlier_chunk': member_link, 'dense_300': dense_300, 'cap_exact': cap_exact, 'cap_plus_one': cap_plus_one, 'cap_one': cap_one,
    'cap_256_n4': cap_256_n4, 'cluster_sizes': cluster_sizes, 'heading_fold': heading_fold,
}


def test_every_regime_has_a_case():
    keys = {n: rr.case(n)[0]['regimes'] for n in rr.NAMES}
    table = {k: [n for n in rr.NAMES if k in keys[n]] for k in REGIMES}
    assert all(table.values()), [k for k, v in table.items() if not v]
    assert all(keys[n] and set(keys[n]) <= set(REGIMES) for n in rr.NAMES)
    for k, v in table.items():
        print('%-26s %s' % (k, ', '.join(v)))


@pytest.mark.parametrize('name', rr.NAMES)
def test_case_is_sound_and_the_schedule_agrees_with_the_yardstick(name):
    c, want = rr.case(name)
    R, C, topk, cap = c['R'], c['C'], c['topk'], c['cap']
    assert want['margin'] >= rr.MARGIN
    assert c['rec'].shape == (R * C, topk, 32) and c['rec'].dtype == np.float32 and c['ext'].shape == (R, C, 12) and c['ext'].dtype == np.float64
    assert 1 <= C <= 16 and 1 <= topk <= 256 and C * topk <= 2048 and 1 <= cap <= 256
    assert want['out'].shape == (R, cap, 32) and want['map'].shape == (R * C, topk) and want['n'].shape == (R, 2)
    sch = rr.schedule(c)
    assert len(sch) == R
    for r, s in enumerate(sch):
        assert s['n'] == int(kept(c, r).sum()) == int((want['map'][r * C:(r + 1) * C] != -1).sum())
        assert s['order'] == ref.candidates(c['rec'][r * C:(r + 1) * C], c['params']['min_score'])
        assert s['clusters'] == want['clusters'][r], (name, r)                    # the representatives, and who joins whom, in order
        assert np.array_equal(s['map'], want['map'][r * C:(r + 1) * C]) and np.array_equal(s['counts'], want['n'][r])
        assert len(s['rounds']) == (s['n'] + 63) // 64 and all(0 <= v <= 64 for v in s['rounds'])
    assert rr.same_as_yardstick(c, sch, want)


@pytest.mark.parametrize('name', rr.NAMES)
def test_case_reaches_its_regimes(name):
    c, want = rr.case(name)
    for key in c['regimes']:
        REGIMES[key](c, rr.schedule(c), want)


def test_the_cases_cover_the_table():
    all_s = [(rr.case(n)[0], s) for n in rr.NAMES for s in rr.schedule(rr.case(n)[0])]
    assert {s['n'] for _, s in all_s} >= set(rr.SORT_N) | {0} and set(SORT) == set(rr.SORT_N)
    assert {s['M'] for _, s in all_s} == {64, 128, 256, 512, 1024, 2048} and {s['pairs'] for _, s in all_s} == {1, 2, 4}
    P = [rr.case(n)[0]['params'] for n in rr.NAMES]
    assert {p['metric'] for p in P} == {'bev', 'iou3d', 'dist'} and {p['merge'] for p in P} == {'best', 'mean'}
    assert {p['class_aware'] for p in P} == {True, False} and {p['cross_only'] for p in P} == {True, False}
    rounds = {v for _, s in all_s for v in s['rounds']}
    assert {0, 1, 2, 64} <= rounds and any(8 <= v < 64 for v in rounds)
    assert {t for _, s in all_s for t in s['taken']} == {'rep', 'settle', 'push'}
    assert max(max(s['chunk_dist']) for _, s in all_s if s['n']) == 31 and max(s['largest'] for _, s in all_s) == 2048
    assert any(s['ncl'] == s['cap'] for _, s in all_s) and any(s['ncl'] == s['cap'] + 1 for _, s in all_s)
    assert {c['cap'] for c, _ in all_s} >= {1, 256} and {c['R'] for c, _ in all_s} >= {1, 3}
    assert sum(any(s['n'] > 1024 for s in rr.schedule(rr.case(n)[0])) for n in rr.NAMES) <= 3
    print('n: %s\nsettle rounds: %s' % (sorted({s['n'] for _, s in all_s}), sorted(rounds)))


# ------------------------------------------------------------------------------------------ wrong schedules
VARIANTS = {         # wrong variant of the host model -> the cases that must tell it from the yardstick
    'push_next_word': ('chain_parity1', 'two_reps_other_chunks', 'link_every_word'),     # the push reads word c + 1 of its rows, not word c
    'latest_rep': ('two_reps_same_chunk',),                                              # the latest linked representative of a chunk wins
    'push_overwrites': ('two_reps_other_chunks',),                                       # a later chunk's push takes a position again
    'slot_before_camera': ('ties',),                                                     # ties ordered by slot, then camera
    'signed_zero': ('keys_negative_special',),                                           # -0 sorted behind +0
    'no_negative_branch': ('keys_negative_special',),                                    # the key of a negative score not inverted
}


SORT_VARIANTS = {    # wrong variant of the sort network -> (case, rig) whose keys it leaves out of order; the rigs below the size are blind
    'sort_direction': (('sort_n1_63_64_65', 3), ('sort_n128_to_513', 2), ('sort_n128_to_513', 5), ('sort_n1024', 0)),      # the stages j = 64: M >= 128
    'sort_one_pair_per_lane': (('sort_n128_to_513', 5), ('sort_n1024', 0), ('star_n1025_best', 1)),    # M >= 1024
}


@pytest.mark.parametrize('variant', list(SORT_VARIANTS))
def test_wrong_sort_networks_are_caught(variant):
    for name, r in SORT_VARIANTS[variant]:
        c = rr.case(name)[0]
        n, M, net = rr.prepare(c, r)
        n2, M2, bad = rr.prepare(c, r, variant)
        assert (n2, M2) == (n, M) and net == sorted(net) and sorted(bad) == net and bad[:n] != net[:n], (variant, name, r)
        print('%s: caught by rig %d of %s (n = %d, M = %d), %d of %d positions hold another key' % (variant, r, name, n, M,
              sum(a != b for a, b in zip(bad[:n], net[:n])), n))
    c = rr.case('sort_n1_63_64_65')[0]
    assert all(rr.prepare(c, r, variant)[2] == rr.prepare(c, r)[2] for r in range(3))        # M = 64: the stages do not exist


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_wrong_schedules_are_caught(variant):
    for name in VARIANTS[variant]:
        c, want = rr.case(name)
        assert rr.same_as_yardstick(c, rr.schedule(c), want)
        assert not rr.same_as_yardstick(c, rr.schedule(c, variant), want), (variant, name)
        print('%s: caught by %s' % (variant, name))
