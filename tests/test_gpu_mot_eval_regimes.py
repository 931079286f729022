"""GPU: the tracking evaluation (csrc/mot_eval.hip) in every regime of its six kernels, on the cases of tests/mot_eval_regimes.py
(tests/test_mot_eval_regimes.py shows on the CPU that each reaches its regime and would notice a wrong rule), compared by the rule
of tests/test_gpu_mot_eval.py: integer outputs EQUAL, potential / loc / simsum and every closing metric within 1e-9, the
yardstick's margin >= 1e-6 asserted first.
  * generated: the last sizes of the one-column solver form, the four-column form chosen by rows alone and by columns alone, both
    forms inside one sequence, 256 x 256, empty sequences, frames that are not PROCESSED, ragged id counts, 200 x 1 and 1 x 200;
  * similarities exactly at every alpha and at the CLEAR threshold and one, two, three fp64 steps below, in both solver forms;
  * the hand cases of tests/test_mot_eval_cpu.py with their literal values, the tracker-empty frames of the idcount rule among them;
  * HOTA alone and CLEAR alone equal the combined run bit for bit; two runs are byte-identical; NaN and garbage ids beyond ng / nt
    change nothing; through the C entry points, garbage in the workspace and in the WRITTEN outputs changes nothing and a second
    call doubles the ADDED-TO outputs exactly.

Measured on an MI355X (the figure each case prints; copied to profiles/mot_eval.txt): the largest disagreement of potential, loc,
simsum and of every closing metric is 0 in all ten generated cases (nc1_edge, nc4_by_rows, nc4_by_cols, mixed_forms, full_256,
empty_sequences, unprocessed, ragged_ids, tall, wide) and in edges_nc1 / edges_nc4 at both thresholds; every integer output is
equal.  The bar stays the project's 1e-9.  The whole file takes 4 s, 0.8 s of it full_256."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, kitti_eval, mot_eval                # noqa: E402
from tests import mot_eval_ref as ref                           # noqa: E402
from tests import mot_eval_regimes as mr                        # noqa: E402
from tests.test_gpu_mot_eval import FLOAT_KEYS, INT_KEYS, TOL, compare      # noqa: E402

HOTA_KEYS = ('potential', 'gcount', 'tcount', 'match', 'tp', 'fn', 'fp', 'loc', 'mc')
CLEAR_KEYS = ('clear_match', 'counts', 'simsum', 'idcount', 'matched', 'frag')
WRITTEN = ('match', 'potential', 'gcount', 'tcount', 'loc', 'simsum', 'clear_match')
ADDED_TO = ('tp', 'fn', 'fp', 'mc', 'counts', 'idcount', 'matched', 'frag')
_runs = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def run(dev, a, **kw):
    return mot_eval.run_device(torch.from_numpy(np.ascontiguousarray(a['sim'])).to(dev), a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], **kw)


def run_case(dev, name):
    """The device outputs of a generated case, computed once and shared; nobody changes them."""
    if name not in _runs:
        _runs[name] = run(dev, mr.case(name)[0])
    return _runs[name]


def device_metrics(got):
    return (mot_eval.hota_metrics(*(got[k] for k in ('tp', 'fn', 'fp', 'loc', 'mc', 'gcount', 'tcount'))),
            mot_eval.clear_metrics(*(got[k] for k in ('counts', 'simsum', 'idcount', 'matched', 'frag'))))


def compare_all(name, got, h, c):
    """The rule of tests/test_gpu_mot_eval.py on the raw outputs and on the closing metrics: the largest float disagreement."""
    worst = compare(name, got, h, c)
    hm, cm = device_metrics(got)
    want_h, want_c = ref.hota_metrics(h), ref.clear_metrics(c)
    for k in mot_eval.HOTA_FIELDS:
        worst = max(worst, float(np.abs(hm[k] - want_h[k]).max()))
    for k in mot_eval.CLEAR_FIELDS:
        assert isinstance(want_c[k], float) or cm[k] == want_c[k], (name, k, cm[k], want_c[k])
        worst = max(worst, abs(cm[k] - want_c[k]))
    assert worst <= TOL, (name, worst)
    return worst


def same_bytes(a, b, keys=None):
    return [k for k in (keys or a) if a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape]


# --------------------------------------------------------------------------------------------------------------- generated
@pytest.mark.parametrize('name', sorted(mr.CASES))
def test_generated_regimes_equal_the_yardstick(dev, name):
    a, h, c, margin = mr.case(name)
    assert margin >= mr.MARGIN, margin
    got = run_case(dev, name)
    worst = compare_all(name, got, h, c)
    cm = ref.clear_metrics(c)
    print('%s (seed %d): %d frames up to %d x %d, TP %d FN %d FP %d IDSW %d Frag %d; largest disagreement of potential / loc / simsum / any '
          'metric %.3g (bar %g)' % (name, mr.SEEDS[name], len(a['ng']), a['ng'].max(), a['nt'].max(), cm['TP'], cm['FN'], cm['FP'], cm['IDSW'],
                                    cm['Frag'], worst, TOL))


def test_empty_sequences_stay_zero_and_unused_blocks_are_written(dev):
    got = run_case(dev, 'empty_sequences')
    for s in (0, 2, 3, 5):
        assert all(not got[k][s].any() for k in got if k not in ('match', 'clear_match')), s
    a = mr.case('mixed_forms')[0]
    got = run_case(dev, 'mixed_forms')
    for k in ('match', 'clear_match'):
        assert all((got[k][f, a['ng'][f]:] == -1).all() for f in range(len(a['ng']))) and (got[k][4, :2] >= 0).any()


# ------------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize('name', sorted(mr.EDGES))
def test_similarities_at_the_decisions_and_a_few_steps_below(dev, name):
    a, values = mr.edges(mr.EDGES[name])
    K = len(values)
    for thr in mr.EDGE_THRS:
        h = ref.hota(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], with_margin=False)
        c = ref.clear(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], thr, with_margin=False)
        got = run(dev, a, clear_thresh=thr)
        worst = compare_all(name, got, h, c)
        at = 4 * (len(mr.EDGES[name]) + mr.EDGE_THRS.index(thr))
        assert (got['clear_match'][0, at:at + 4] >= 0).tolist() == [True, True, True, thr <= 0.5]
        assert got['match'][0].tolist() == [K - 1 - g for g in range(K)]
        for i, k in enumerate(mr.EDGES[name]):                # at alpha_k: counted with the steps within EPS of it, and not at k + 1
            counted = [bool(got['mc'][0, k, 4 * i + j, K - 1 - (4 * i + j)]) for j in range(4)]
            assert counted == [True, True, True, 0.05 + k * 0.05 <= 0.5], (k, counted)
        print('%s, thr %g: %d isolated pairs, TP per alpha %s, CLEAR TP %d; largest disagreement %.3g' % (name, thr, K, got['tp'][0].tolist(),
                                                                                                          got['counts'][0, 0], worst))


# -------------------------------------------------------------------------------------------------------------- hand cases
def hand_on_device(dev, name):
    got = run(dev, mr.hand(name))
    hm, cm = device_metrics(got)
    return got, hm, cm


def test_hand_perfect_tracker(dev):
    got, hm, cm = hand_on_device(dev, 'perfect')
    assert all(np.array_equal(hm[k], np.ones(19)) for k in mot_eval.HOTA_FIELDS)
    assert cm['MOTA'] == 1.0 and cm['MOTP'] == 1.0 and cm['IDSW'] == 0 and cm['Frag'] == 0 and cm['MT'] == 2 and (cm['TP'], cm['FN'], cm['FP']) == (10, 0, 0)


def test_hand_ids_that_swap_halfway(dev):
    got, hm, cm = hand_on_device(dev, 'swap_halfway')
    assert np.array_equal(got['potential'][0], np.full((2, 2), 2.0)) and np.array_equal(got['mc'][0, 7], np.full((2, 2), 2))
    assert np.array_equal(hm['DetA'], np.ones(19)) and np.allclose(hm['AssA'], 1.0 / 3.0, rtol=0, atol=1e-15)
    assert np.allclose(hm['HOTA'], np.sqrt(1.0 / 3.0), rtol=0, atol=1e-15) and np.allclose(hm['AssRe'], 0.5) and np.allclose(hm['AssPr'], 0.5)
    assert cm['IDSW'] == 2 and cm['MOTA'] == (8 - 0 - 2) / 8 and cm['Frag'] == 0 and cm['TP'] == 8


@pytest.mark.parametrize('new_id', [False, True])
def test_hand_track_lost_for_two_frames(dev, new_id):
    got, hm, cm = hand_on_device(dev, 'lost_new_id' if new_id else 'lost_same_id')
    assert cm['Frag'] == 1 and cm['IDSW'] == (1 if new_id else 0) and (cm['TP'], cm['FN'], cm['FP']) == (10, 2, 0)
    assert got['frag'][0].tolist() == [2, 1] and got['matched'][0].tolist() == [4, 6] and got['idcount'][0].tolist() == [6, 6]
    assert abs(cm['MOTP'] - (4 * 0.9 + 6 * 0.8) / 10) < 1e-14


def test_hand_empty_frames_leave_the_carried_state_alone(dev):
    got, hm, cm = hand_on_device(dev, 'empty_frames')
    assert got['clear_match'][4, 0] == 1 and cm['IDSW'] == 0 and cm['Frag'] == 0 and got['frag'][0, 0] == 1
    assert (cm['TP'], cm['FN'], cm['FP']) == (2, 1, 2) and abs(got['simsum'][0] - 1.3) < 1e-15
    assert got['match'][4, 0] in (0, 1) and got['gcount'][0, 0] == 3 and got['tcount'][0].tolist() == [2, 2]
    assert got['idcount'][0, 0] == 3 and got['matched'][0, 0] == 2 and (cm['MT'], cm['PT'], cm['ML']) == (0, 1, 0)
    got, hm, cm = hand_on_device(dev, 'gap_processed')        # the gap PROCESSED: prev is cleared, the better overlap wins
    assert got['clear_match'][2, 0] == 0 and got['counts'][0, 3] == 1 and got['frag'][0, 0] == 2


def test_hand_frames_with_an_empty_tracker_count_in_the_life_of_an_object(dev):
    got, hm, cm = hand_on_device(dev, 'empty_tracker_8_of_10')
    assert got['idcount'][0, 0] == 10 and got['matched'][0, 0] == 2 and got['gcount'][0, 0] == 10
    assert (cm['MT'], cm['PT'], cm['ML']) == (0, 1, 0) and (cm['TP'], cm['FN'], cm['FP'], cm['IDSW'], cm['Frag']) == (2, 8, 0, 0, 0)
    got, hm, cm = hand_on_device(dev, 'empty_tracker_9_of_11')
    assert got['idcount'][0, 0] == 11 and got['matched'][0, 0] == 2 and (cm['MT'], cm['PT'], cm['ML']) == (0, 0, 1)
    assert (cm['TP'], cm['FN'], cm['FP'], cm['IDSW'], cm['Frag']) == (2, 9, 0, 0, 0) and abs(cm['MOTP'] - 0.7) < 1e-15


# ------------------------------------------------------------------------------------------------ the header's statements
@pytest.mark.parametrize('name', ['mixed_forms', 'unprocessed', 'empty_sequences'])
def test_hota_alone_and_clear_alone_equal_the_combined_run(dev, name):
    a = mr.case(name)[0]
    full, h_only, c_only = run_case(dev, name), run(dev, a, clear=False), run(dev, a, hota=False)
    assert sorted(h_only) == sorted(HOTA_KEYS) and sorted(c_only) == sorted(CLEAR_KEYS)
    assert same_bytes(h_only, full) == [] and same_bytes(c_only, full) == []


@pytest.mark.parametrize('name', ['full_256', 'mixed_forms'])
def test_two_runs_are_byte_identical(dev, name):
    assert same_bytes(run(dev, mr.case(name)[0]), run_case(dev, name)) == []


@pytest.mark.parametrize('name', ['nc1_edge', 'nc4_by_rows', 'nc4_by_cols', 'mixed_forms', 'unprocessed', 'empty_sequences', 'tall', 'wide'])
def test_entries_beyond_ng_and_nt_are_never_read(dev, name):
    a = mr.case(name)[0]
    bad = {k: np.array(v, copy=True) for k, v in a.items()}
    touched = 0
    for f in range(len(a['ng'])):
        n, m = int(a['ng'][f]), int(a['nt'][f])
        bad['sim'][f, n:, :], bad['sim'][f, :, m:] = np.nan, np.nan
        bad['gid'][f, n:] = np.where(np.arange(bad['gid'].shape[1] - n) % 2 == 0, 2 ** 30 + f, -7)
        bad['tid'][f, m:] = np.where(np.arange(bad['tid'].shape[1] - m) % 2 == 0, -7, 2 ** 30 + f)
        touched += bad['sim'][f].size - n * m
    assert touched > 0 and np.isnan(bad['sim']).sum() == touched
    assert same_bytes(run(dev, bad), run_case(dev, name)) == []


def raw_calls(dev, a, thr=0.5):
    """rtm3d_mot_hota and rtm3d_mot_clear through ctypes on arrays of the caller (tools/gpu_mot_eval_time.py shows the call), twice
    on the same outputs: the workspace and the WRITTEN outputs hold garbage before each call (another garbage the second time),
    the ADDED-TO outputs are zeroed once.  Returns the outputs after the first and after the second call."""
    lib = _lib.load()
    F, cap_g, cap_t = a['sim'].shape
    S = len(a['seq_start']) - 1
    vg, vt = np.arange(cap_g)[None, :] < a['ng'][:, None], np.arange(cap_t)[None, :] < a['nt'][:, None]
    n_gid, n_tid = max(int(a['gid'][vg].max(initial=-1)) + 1, 1), max(int(a['tid'][vt].max(initial=-1)) + 1, 1)
    up = lambda x, dt=np.int32: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)     # noqa: E731
    d = {k: up(v) for k, v in dict(seq=a['seq_start'], ng=a['ng'], nt=a['nt'], gid=a['gid'], tid=a['tid'], gslot=mot_eval.slot_tables(a['gid'], a['ng'], n_gid),
                                   tslot=mot_eval.slot_tables(a['tid'], a['nt'], n_tid)).items()}
    sim = up(a['sim'], np.float64)
    need = int(lib.rtm3d_mot_workspace_bytes(S, F, cap_g, cap_t, n_gid, n_tid))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)                # noqa: E731
    t = dict(potential=z(S, n_gid, n_tid, dt=torch.float64), gcount=z(S, n_gid), tcount=z(S, n_tid), match=z(F, cap_g), tp=z(S, 19), fn=z(S, 19),
             fp=z(S, 19), loc=z(S, 19, dt=torch.float64), mc=z(S, 19, n_gid, n_tid), clear_match=z(F, cap_g), counts=z(S, 4),
             simsum=z(S, dt=torch.float64), idcount=z(S, n_gid), matched=z(S, n_gid), frag=z(S, n_gid))
    stream = kitti_eval._stream(dev)
    p = {k: v.data_ptr() for k, v in dict(d, **t).items()}
    out = []
    for byte, integer, real in ((0xA5, -123456789, float('nan')), (0x3C, 2 ** 31 - 1, float('inf'))):
        for k in WRITTEN:
            t[k].fill_(real if t[k].dtype == torch.float64 else integer)
        ws.fill_(byte)
        _lib.check(lib.rtm3d_mot_hota(stream, S, F, cap_g, cap_t, n_gid, n_tid, p['seq'], p['ng'], p['nt'], p['gid'], p['tid'], p['gslot'], p['tslot'],
                                      sim.data_ptr(), p['potential'], p['gcount'], p['tcount'], p['match'], p['tp'], p['fn'], p['fp'], p['loc'], p['mc'],
                                      ws.data_ptr()), 'mot_hota')
        ws.fill_(byte ^ 0xFF)
        _lib.check(lib.rtm3d_mot_clear(stream, S, F, cap_g, cap_t, n_gid, n_tid, p['seq'], p['ng'], p['nt'], p['gid'], p['tid'], sim.data_ptr(), thr,
                                       p['clear_match'], p['counts'], p['simsum'], p['idcount'], p['matched'], p['frag'], ws.data_ptr()), 'mot_clear')
        torch.cuda.synchronize()
        out.append({k: v.cpu().numpy() for k, v in t.items()})
    return out


@pytest.mark.parametrize('name', ['mixed_forms', 'unprocessed', 'ragged_ids', 'empty_sequences'])
def test_written_outputs_are_written_and_added_outputs_are_added_to(dev, name):
    assert sorted(WRITTEN + ADDED_TO) == sorted(INT_KEYS + FLOAT_KEYS)
    first, second = raw_calls(dev, mr.case(name)[0])
    assert same_bytes(first, run_case(dev, name)) == []       # garbage in the workspace and in the WRITTEN outputs changes nothing
    assert same_bytes(second, first, WRITTEN) == []
    for k in ADDED_TO:
        assert np.array_equal(second[k], 2 * first[k]) and first[k].any(), k
