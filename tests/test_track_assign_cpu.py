"""CPU: the yardstick of the optimal association (tests/track_assign_ref.py) against scipy and against brute force, its frame
step against tests/track_ref.py's under the greedy matcher, the conditions of the sequences tests/test_gpu_track_assign.py runs,
and the parts of the library and binding that need no GPU: the exported symbol, the two defines, the host-side refusals."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import track_ref as ref
from tests import track_cases as tc
from tests import track_assign_ref as ar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sparse_gains(rng, n, m, density=0.3):
    G = rng.uniform(0.01, 1.0, (n, m))
    G[rng.uniform(size=(n, m)) >= density] = np.nan
    return G


def pairs_of(G):
    return [(G[t, k], t, k) for t in range(G.shape[0]) for k in range(G.shape[1]) if not np.isnan(G[t, k])]


@pytest.mark.parametrize('shape', [(8, 7), (70, 74), (128, 100)], ids=lambda s: '%dx%d' % s)
def test_matcher_equals_scipy(shape):
    lsa = pytest.importorskip('scipy.optimize').linear_sum_assignment
    n, m = shape
    G = sparse_gains(np.random.Generator(np.random.PCG64(0)), n, m)
    cost = np.full((n, m + n), np.inf)
    cost[:, :m] = np.where(np.isnan(G), np.inf, -G)
    cost[np.arange(n), m + np.arange(n)] = 0.0
    r, c = lsa(cost)
    want = -float(cost[r, c].sum())
    det_of, total, margin = ar.optimal_match(pairs_of(G))
    _, g_total, _ = ar.greedy([(g, t, k) for g, t, k in pairs_of(G)], 0.0)
    print('%dx%d: optimum %.6f, greedy %.6f, uniqueness margin %.3g' % (n, m, total, g_total, margin))
    assert abs(total - want) <= 1e-9 * max(1.0, want)
    assert len(set(det_of.values())) == len(det_of) and all(not np.isnan(G[t, k]) for t, k in det_of.items())
    assert abs(sum(G[t, k] for t, k in det_of.items()) - total) <= 1e-9
    assert total > g_total + 1e-9 and margin > 0.0             # random gains: the optimum is unique and greedy misses it
    # the margin is what forbidding a matched pair costs: every single forbidden pair loses at least that much, one exactly
    loss = []
    for t, k in list(det_of.items())[:12]:
        H = G.copy()
        H[t, k] = np.nan
        loss.append(total - ar.optimal_match(pairs_of(H), with_margin=False)[1])
    assert min(loss) >= margin - 1e-12


def test_matcher_equals_brute_force_on_4x4():
    rng = np.random.Generator(np.random.PCG64(4))
    seen = dict(empty_row=0, empty_col=0, none=0, full=0)
    for n in range(60):
        G = sparse_gains(rng, 4, 4, density=(0.0, 0.2, 0.5, 0.8, 1.0)[n % 5])
        if n % 7 == 3:
            G[rng.integers(4)] = np.nan
        if n % 7 == 5:
            G[:, rng.integers(4)] = np.nan
        c = ~np.isnan(G)
        seen['empty_row'] += bool((~c.any(1)).any() and c.any())
        seen['empty_col'] += bool((~c.any(0)).any() and c.any())
        seen['none'] += not c.any()
        seen['full'] += bool(c.all())
        det_of, total, _ = ar.optimal_match(pairs_of(G))
        assert abs(total - ar.brute_force(G)) <= 1e-12, (n, G)
        assert all(c[t, k] for t, k in det_of.items()) and len(set(det_of.values())) == len(det_of)
    assert all(v > 0 for v in seen.values()), seen
    # ties: a second optimum makes the uniqueness margin 0
    assert ar.optimal_match([(0.5, 0, 0), (0.5, 0, 1), (0.5, 1, 0), (0.5, 1, 1)])[1:] == (1.0, 0.0)
    # fewer pairs can be more gain: one pair of 1.0 against two of 0.1 + 0.8
    assert ar.optimal_match([(1.0, 0, 0), (0.1, 0, 1), (0.8, 1, 0)])[0] == {0: 0}


def test_step_with_the_greedy_matcher_is_track_ref_step():
    """The births and ids restated in track_assign_ref.step are track_ref.step's: the same ids and tables, bit for bit."""
    for name in ('twins_class_blind', 'overflow_bev', 'three_streams_classes'):
        c = tc.case(name)[0]
        want = tc.reference(c)
        got = ar.run(c['frames'], c['T'], c['params'], c['dt'], c['egos'], matcher=ar.greedy)
        for (ids, table, _, _), (w_ids, w_table, _) in zip(got, want):
            assert ids.tobytes() == w_ids.tobytes() and table.tobytes() == w_table.tobytes(), name


def test_chain_case_is_what_the_device_test_assumes():
    c, res = ar.fixed('chain_dist')
    assert c['T'] == 64 and c['topk'] == 48 and c['frames'][0].shape == (2, 48, 32) and len(c['frames']) == 2
    greedy = ar.run(c['frames'], c['T'], c['params'], matcher=ar.greedy)
    for b in range(2):
        assert np.array_equal(res[1][0][b], res[0][0][b]) and np.count_nonzero(res[0][0][b]) == ar.CHAIN
        assert res[1][1][b, 0] == ar.CHAIN and greedy[1][1][b, 0] == ar.CHAIN + 1
        assert (greedy[1][0][b] != greedy[0][0][b]).sum() == ar.CHAIN
        # 40 pairs of 0.495 against 39 of 0.505; positions are fp32, ~4e-6 each at 120 m
        assert abs(res[1][3][b] - 19.8) < 1e-3 and abs(greedy[1][3][b] - 19.695) < 1e-3 and abs(res[1][2][b] - 0.105) < 1e-3
    x = c['frames'][1][:, :ar.CHAIN, 27]
    assert (np.diff(x[0]) > 0).all() and (np.diff(x[1]) < 0).all()


def test_ties_and_no_candidate_cases():
    c, res = ar.fixed('exact_ties')
    assert res[1][3][0] == 3.0 and res[1][2][0] == 0.0 and sorted(res[1][0][0][:2].tolist()) == [1, 2]
    c, res = ar.fixed('no_candidates')
    greedy = ar.run(c['frames'], c['T'], c['params'], matcher=ar.greedy)
    assert res[1][3][0] == 0.0 and res[1][1].tobytes() == greedy[1][1].tobytes() and res[1][1][0, 2] == 2
    assert res[1][0][0][:5].tolist() == [6, 7, 8, 0, 0]


OPT_NAMES = ('dense_3d', 'overflow_bev', 'three_streams_classes', 'crossing_dist_ego')


@pytest.mark.parametrize('name', OPT_NAMES)
def test_optimal_case_conditions(name):
    c, res = ar.case(name)
    assert len(res) == 12 and min(float(r[2].min()) for r in res) >= tc.MARGIN
    B, T = c['frames'][0].shape[0], c['T']
    live = [int((r[1][:, ref.HEADER:].reshape(B, T, ref.SLOT)[..., 0] != 0).sum(1).max()) for r in res]
    if name == 'dense_3d':
        assert max(live) >= 70 and c['topk'] == 100 and T == 128
    if name == 'overflow_bev':
        assert T == 8 and res[-1][1][0, 2] > 0
    if name == 'three_streams_classes':
        assert B == 3 and c['topk'] == 7 and c['params']['class_aware'] and not res[5][0][1].any() and not res[0][0][2].any()
    if name == 'crossing_dist_ego':
        assert c['egos'] is not None and min(float(r[2].min()) for r in res[1:]) < 0.1      # the crossing pair competed


# ------------------------------------------------------------------------------------------------ library and binding
def test_header_library_and_binding_agree():
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert re.search(r'#define RTM3D_ABI_VERSION 9\b', hdr) and _lib.ABI_VERSION == 9
    name = 'rtm3d_tracks_update_assign'
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
    assert m and len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]) == 12
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert re.search(r'#define RTM3D_TRACK_ASSIGN_GREEDY 0\b', hdr) and re.search(r'#define RTM3D_TRACK_ASSIGN_OPTIMAL 1\b', hdr)
    from rtm3d_amd import track
    assert track.ASSIGNMENTS == {'greedy': 0, 'optimal': 1}


def test_assign_refusals_need_no_gpu():
    """Every argument is checked before anything is launched: the pointers below are never dereferenced."""
    lib = _lib.load()
    p = _lib.TrackParamsC()
    assert lib.rtm3d_track_default_params(ctypes.byref(p)) == 0
    fake = ctypes.c_void_p(0x1000)

    def call(assign, T=128, dt=1.0, params=p):
        rc = lib.rtm3d_tracks_update_assign(None, 1, 100, T, fake, dt, None, ctypes.byref(params), assign, fake, fake, fake)
        return rc, lib.rtm3d_last_error().decode()

    for assign in (-1, 2):
        rc, msg = call(assign)
        assert rc != 0 and msg.startswith('tracks_update_assign') and 'assign %d' % assign in msg, msg
    for assign in (0, 1):
        rc, msg = call(assign, T=257)
        assert rc != 0 and msg.startswith('tracks_update') and 'T 257' in msg, msg
        rc, msg = call(assign, dt=0.0)
        assert rc != 0 and msg.startswith('tracks_update') and 'dt' in msg, msg
    q = _lib.TrackParamsC.from_buffer_copy(p)
    q.thresh = float('-inf')
    rc, msg = call(1, params=q)
    assert rc != 0 and 'finite thresh' in msg, msg


def test_python_option():
    from rtm3d_amd import track
    sig = inspect.signature(track.Tracker.__init__)
    assert sig.parameters['assignment'].default == 'greedy' and list(sig.parameters)[-1] == 'assignment'
    src = inspect.getsource(track.Tracker.__init__)
    assert src.index('assignment not in') < src.index('_lib.load()')     # refused before anything touches the device
    with pytest.raises(ValueError, match='assignment'):
        track.Tracker(1, 8, None, 'cuda', 'auction')
    with pytest.raises(ValueError, match='assignment'):
        track.Tracker(1, assignment='auction')
