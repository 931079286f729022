"""GPU: the tracker (csrc/track.hip: track_affinity_kernel, track_step_kernel<greedy | optimal>) against the numpy yardsticks
tests/track_ref.py and tests/track_assign_ref.py over the cases of tests/track_regimes.py - every regime of the two kernels that
the sequences of tests/track_cases.py leave out: all four waves of the step kernel's workgroup and all eight words of its bit
matrices in use (T = topk = 256), chains and cascades in the slots >= 192, T >> topk, T << topk, T = topk = 1, odd sizes over three
streams, dt != 1 and a dt per frame with every noise term non-default, general ego motion, the lifecycle parameters at their
ends, exact ties of the greedy order in the upper slots, and kept records whose box is not finite.  tests/test_track_regimes.py asserts on the CPU that each case reaches its regime
and that each would catch a kernel that is wrong there.

Every case runs under both assignments, frame by frame, by the comparison rule of tests/test_gpu_track.py: ids, header and the
exact fields EQUAL, the filtered states and covariances within 1e-9 (fp64 without contraction on both sides), NaN where the
yardstick has NaN; the records are byte-identical after each call.  Then: assign = greedy through rtm3d_tracks_update_assign
against rtm3d_tracks_update, two runs of the largest cases, a workspace and ids filled with garbage before every call, and the
reset of one stream of three in mid-sequence - all bit for bit.

Measured on an MI355X (the figure each case prints; copied to profiles/track.txt), the same under greedy and optimal: 0 in full_256,
chain_upper, tall, wide, one_by_one, ragged_streams, dt_small, dt_large, dt_varying, the five life_* cases, nonfinite_boxes and ties_upper (greedy);
1.33e-15 in ego_general (cos / sin / atan2 of the heading under ego motion).  Bar 1e-9."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, track                    # noqa: E402
from tests import track_ref as ref                   # noqa: E402
from tests import track_cases as tc                  # noqa: E402
from tests import track_assign_ref as ar             # noqa: E402
from tests import track_regimes as tr                # noqa: E402

TOL = 1e-9
EXACT = [0, 1, 2, 3, 4, 5, 6, 22, 23]                 # as in tests/test_gpu_track.py: id, class, age, hits, misses, score, record slot, zeros
FLOAT = list(range(7, 22))                            # h w l X Y Z ry vx vy vz, Ppp Ppv Pvv, var ry, var dim
_runs = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def run_device(name, dev, assignment, reset=None):
    """[(ids, table)] per frame as numpy, through rtm3d_amd.track.Tracker.  reset = (calls, streams): those streams are reset
    after that many calls."""
    case = tr.case(name)[0]
    B = case['frames'][0].shape[0]
    trk = track.Tracker(B, case['T'], track.TrackParams(**case['params']), dev, assignment=assignment)
    out = []
    for f, rec in enumerate(case['frames']):
        if reset is not None and f == reset[0]:
            assert bool((trk.state[:, 1] == reset[0]).all()) and bool(trk.tracks()['live'][reset[1][0]].any())
            trk.reset(reset[1])
        d_rec = torch.from_numpy(rec).to(dev)
        ego = None if case['egos'] is None else torch.from_numpy(np.ascontiguousarray(case['egos'][f])).to(dev)
        ids = trk.update(d_rec, dt=case['dts'][f], ego=ego)
        torch.cuda.synchronize()
        assert d_rec.cpu().numpy().tobytes() == rec.tobytes()                 # the records are read only
        out.append((ids.cpu().numpy(), trk.state.cpu().numpy().copy()))
    return out


def first_run(name, dev, assignment):
    """The undisturbed run of a case, made once per module and shared by the tests that compare against it."""
    if (name, assignment) not in _runs:
        _runs[name, assignment] = run_device(name, dev, assignment)
    return _runs[name, assignment]


def same_bits(a, b, streams=None):
    for f, ((ia, ta), (ib, tb)) in enumerate(zip(a, b)):
        for s in (range(ia.shape[0]) if streams is None else streams):
            assert ia[s].tobytes() == ib[s].tobytes() and ta[s].tobytes() == tb[s].tobytes(), (f, s)


@pytest.mark.parametrize('name,assignment', [(n, a) for n in tr.NAMES for a in tr.ASSIGNMENTS] + [(n, 'greedy') for n in tr.GREEDY_ONLY])
def test_regimes_equal_the_yardstick(dev, name, assignment):
    case, want = tr.case(name)[0], tr.reference(name, assignment)
    assert len(want) == 12 and min(float(w[2].min()) for f, w in enumerate(want) if f not in case['tie_frames']) >= tc.MARGIN
    assert all(want[f][2].min() == 0.0 for f in case['tie_frames'])           # exact ties: the greedy order decides them, on both sides
    got = first_run(name, dev, assignment)
    B, T = case['frames'][0].shape[0], case['T']
    worst = 0.0
    for f, ((ids, table), (w_ids, w_table, _)) in enumerate(zip(got, want)):
        assert np.array_equal(ids, w_ids), (name, assignment, f, np.argwhere(ids != w_ids)[:8].tolist())
        assert np.array_equal(table[:, :ref.HEADER], w_table[:, :ref.HEADER]), (name, assignment, f, table[:, :3], w_table[:, :3])
        g = table[:, ref.HEADER:].reshape(B, T, ref.SLOT)
        w = w_table[:, ref.HEADER:].reshape(B, T, ref.SLOT)
        assert np.array_equal(g[..., EXACT], w[..., EXACT]), (name, assignment, f)
        gf, wf = g[..., FLOAT], w[..., FLOAT]
        assert np.array_equal(np.isnan(gf), np.isnan(wf)), (name, assignment, f)         # equal_nan: NaN where the yardstick has NaN
        inf = np.isinf(gf) | np.isinf(wf)
        assert np.array_equal(gf[inf], wf[inf]), (name, assignment, f)
        fin = np.isfinite(wf)
        err = float(np.abs(gf[fin] - wf[fin]).max()) if fin.any() else 0.0
        worst = max(worst, err)
        assert err <= TOL, (name, assignment, f, err)
    print('%s, %s: largest disagreement of a filtered state or covariance over 12 frames %.3g (bar %g)' % (name, assignment, worst, TOL))


def test_nonfinite_boxes_follow_the_headers_sentence(dev):
    """On the device's own result, not through the yardstick: "a box that is not finite makes a track that is not finite, matches
    nothing and dies of its misses"; the finite objects keep their ids as if the bad records were not there."""
    case = tr.case('nonfinite_boxes')[0]
    m = case['params']['max_misses']
    for assignment in tr.ASSIGNMENTS:
        got = first_run('nonfinite_boxes', dev, assignment)
        s = np.stack([t[0, ref.HEADER:].reshape(case['T'], ref.SLOT) for _, t in got])
        ids = np.stack([i[0] for i, _ in got])
        born = 0
        for f in range(12):
            for t in range(case['T']):
                v = s[f, t]
                if v[0] != 0 and not (np.isfinite(v[7:14]).all() and (v[7:10] > 0).all()):
                    assert (v[6] == -1 or v[2] == 1) and v[2] <= m + 1 and (v[2] <= m or s[f + 1, t, 0] != v[0]), (f, t)
                    born += int(v[2] == 1)
        assert born == 12 and got[-1][1][0, 0] == 15 and got[-1][1][0, 2] == 0
        assert (ids[:, 1] == ids[0, 1]).all() and (ids[:, 3] == ids[0, 3]).all() and ids[0, 1] > 0 and ids[0, 3] > 0
        assert (np.abs(ids[6:, 5]) == 12).all() and not ids[2, 7] and not ids[3, 2]


def test_ties_upper_under_the_optimal_rule_is_an_optimum_and_deterministic(dev):
    """Exact ties in the slots >= 192: any matching of the largest gain may be returned, the same one on every call."""
    case, g = tr.case('ties_upper')[0], tr.reference('ties_upper', 'greedy')
    thresh = case['params']['thresh']
    got = first_run('ties_upper', dev, 'optimal')
    same_bits(got, run_device('ties_upper', dev, 'optimal'))
    same_bits(got[:1], first_run('ties_upper', dev, 'greedy')[:1])              # frame 0 is births only
    cand = {(t, k): a for a, t, k in tr.candidates(case, g, 1)}
    best = ar.optimal_match([(a - thresh, t, k) for (t, k), a in cand.items()], with_margin=False)[1]
    s = got[1][1][0, ref.HEADER:].reshape(case['T'], ref.SLOT)
    pairs = [(t, int(s[t, 6])) for t in range(case['T']) if s[t, 0] != 0 and s[t, 2] > 1 and s[t, 6] >= 0]
    assert len(pairs) == 204 and all(p in cand for p in pairs) and len({k for _, k in pairs}) == 204
    assert abs(sum(cand[p] - thresh for p in pairs) - best) <= 1e-9 and best == 200 * 4.0 + 4 * 1.5
    ids = got[1][0][0]
    assert all(ids[k] == s[t, 0] for t, k in pairs) and got[1][1][0, 0] == 206


def c_run(name, dev, entry, assign, dirty):
    """The sequence through a C entry point on tensors of the test's own: entry 'update' (rtm3d_tracks_update) or 'assign'.
    dirty: the workspace is filled with 0xff bytes (NaN) and d_ids with a pattern before every call."""
    lib = _lib.load()
    case = tr.case(name)[0]
    B, topk, T = case['frames'][0].shape[0], case['topk'], case['T']
    p = track.TrackParams(**case['params']).to_c()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    state = torch.zeros(B, ref.HEADER + ref.SLOT * T, dtype=torch.float64, device=dev)
    ids = torch.zeros(B, topk, dtype=torch.int32, device=dev)
    need = int(lib.rtm3d_tracks_workspace_bytes(B, topk, T))
    assert need == B * T * topk * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = []
    for f, rec in enumerate(case['frames']):
        if dirty:
            ws.fill_(0xff)
            ids.fill_(0x5a5a5a5a)
        d_rec = torch.from_numpy(rec).to(dev)
        ego = None if case['egos'] is None else torch.from_numpy(np.ascontiguousarray(case['egos'][f])).to(dev)
        e_ptr = None if ego is None else ctypes.c_void_p(ego.data_ptr())
        args = (stream, B, topk, T, ctypes.c_void_p(d_rec.data_ptr()), float(case['dts'][f]), e_ptr, ctypes.byref(p))
        tail = (ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(ws.data_ptr()))
        if entry == 'update':
            _lib.check(lib.rtm3d_tracks_update(*(args + tail)), 'tracks_update')
        else:
            _lib.check(lib.rtm3d_tracks_update_assign(*(args + (assign,) + tail)), 'tracks_update_assign')
        torch.cuda.synchronize()
        out.append((ids.cpu().numpy().copy(), state.cpu().numpy().copy()))
    return out


def test_greedy_through_the_assign_entry_is_tracks_update_on_full_256(dev):
    a, b = c_run('full_256', dev, 'update', 0, False), c_run('full_256', dev, 'assign', 0, False)
    same_bits(a, b)
    same_bits(a, first_run('full_256', dev, 'greedy'))
    assert a[-1][1][0, 0] == 238 and int((a[-1][0] != 0).sum()) >= 220


@pytest.mark.parametrize('assignment', tr.ASSIGNMENTS)
@pytest.mark.parametrize('name', ['full_256', 'chain_upper'])
def test_two_runs_are_bit_identical(dev, name, assignment):
    same_bits(first_run(name, dev, assignment), run_device(name, dev, assignment))


@pytest.mark.parametrize('assignment', tr.ASSIGNMENTS)
def test_dirty_workspace_and_ids_change_nothing_on_ragged_streams(dev, assignment):
    same_bits(first_run('ragged_streams', dev, assignment), c_run('ragged_streams', dev, 'assign', track.ASSIGNMENTS[assignment], True))


@pytest.mark.parametrize('assignment', tr.ASSIGNMENTS)
def test_reset_of_stream_1_after_frame_6_leaves_streams_0_and_2_bit_identical(dev, assignment):
    plain = first_run('ragged_streams', dev, assignment)
    got = run_device('ragged_streams', dev, assignment, reset=(6, [1]))
    same_bits(plain, got, streams=(0, 2))
    same_bits(plain[:6], got[:6])
    # the emptied stream starts again: frame counter 1, ids from 1, all confirmed (frame <= min_hits)
    ids, table = got[6]
    n = len(ref.detections(tr.case('ragged_streams')[0]['frames'][6][1], tr.case('ragged_streams')[0]['params']['min_score']))
    assert n >= 30 and tuple(table[1, :3]) == (float(n), 1.0, 0.0) and sorted(ids[1][ids[1] != 0].tolist()) == list(range(1, n + 1))
    assert got[-1][1][1, 1] == 6.0 and plain[-1][1][1, 1] == 12.0
