"""CPU: the cases of tests/mot_eval_regimes.py reach the regimes of csrc/mot_eval.hip they are named for, on the yardstick alone -
sizes, matched rows and columns in the index ranges, every event, the margin - and each would notice a wrong kernel: variants of
the yardstick written here (prev cleared on frames that are not PROCESSED, the 1000 bonus dropped, "> alpha" in the place of
">= alpha - EPS", "< thr" in the place of "< thr - EPS", the idcount rule without the tracker-empty frames) each change an output of
the case that targets them.  tests/test_gpu_mot_eval_regimes.py then compares the device on the same cases."""
import numpy as np
import pytest

from tests import mot_eval_ref as ref
from tests import mot_eval_regimes as mr

CLEAR_KEYS = ('clear_match', 'counts', 'simsum', 'idcount', 'matched', 'frag')


def sizes(a):
    return list(zip(a['ng'].tolist(), a['nt'].tolist()))


def nc4(a):
    """The frames that run the four-columns-per-lane form of the solver."""
    return [f for f, (n, m) in enumerate(sizes(a)) if n > 64 or m > 64]


# -------------------------------------------------------------------------------------------------------- wrong yardsticks
def clear_variant(a, thr=0.5, clear_prev_on_gap=False, bonus=1000.0, eps=ref.EPS, count_empty_tracker=True):
    """ref.clear without the margin, with one rule at a time made wrong."""
    sim, ng, nt, gid, tid, seq_start = (a[k] for k in ('sim', 'ng', 'nt', 'gid', 'tid', 'seq_start'))
    F, cap_g, _ = sim.shape
    S = len(seq_start) - 1
    n_gid = max(max([int(gid[f, :ng[f]].max(initial=-1)) for f in range(F)], default=-1) + 1, 1)
    match = np.full((F, cap_g), -1, np.int32)
    counts, simsum = np.zeros((S, 4), np.int32), np.zeros(S)
    idcount, matched, frag = (np.zeros((S, n_gid), np.int32) for _ in range(3))
    for s in range(S):
        last, prev = {}, {}
        for f in range(int(seq_start[s]), int(seq_start[s + 1])):
            n, m = int(ng[f]), int(nt[f])
            if n == 0 or m == 0:
                counts[s, 1] += n if m == 0 else 0
                counts[s, 2] += m if n == 0 else 0
                if count_empty_tracker:
                    for g in range(n):
                        idcount[s, gid[f, g]] += 1
                if clear_prev_on_gap:
                    prev = {}
                continue
            w = np.zeros((n, m))
            for g in range(n):
                for t in range(m):
                    if not sim[f, g, t] < thr - eps:
                        w[g, t] = (bonus if prev.get(int(gid[f, g])) == int(tid[f, t]) else 0.0) + sim[f, g, t]
            col = ref.assign(w, with_margin=False)[0]
            match[f, :n] = col
            new_prev = {}
            for g in range(n):
                i = int(gid[f, g])
                idcount[s, i] += 1
                if col[g] < 0:
                    continue
                t = int(tid[f, col[g]])
                matched[s, i] += 1
                counts[s, 3] += 1 if i in last and last[i] != t else 0
                frag[s, i] += 0 if i in prev else 1
                last[i] = new_prev[i] = t
                simsum[s] = simsum[s] + sim[f, g, col[g]]
            k = int((col >= 0).sum())
            counts[s, 0] += k
            counts[s, 1] += n - k
            counts[s, 2] += m - k
            prev = new_prev
    return dict(clear_match=match, counts=counts, simsum=simsum, idcount=idcount, matched=matched, frag=frag)


def hota_counts(a, h, strict=False):
    """Steps 4 and 5 of HOTA from the yardstick's match: (tp, fn, fp, mc); strict: "> alpha" in the place of ">= alpha - EPS"."""
    S = len(a['seq_start']) - 1
    tp, fn, fp = (np.zeros((S, ref.N_ALPHA), np.int32) for _ in range(3))
    mc = np.zeros_like(h['mc'])
    for s in range(S):
        for f in range(int(a['seq_start'][s]), int(a['seq_start'][s + 1])):
            n, m = int(a['ng'][f]), int(a['nt'][f])
            for k in range(ref.N_ALPHA):
                counted = 0
                for g in range(n):
                    col = h['match'][f, g]
                    v = a['sim'][f, g, col] if col >= 0 else -1.0
                    if col >= 0 and (v > ref.ALPHAS[k] if strict else v >= ref.ALPHAS[k] - ref.EPS):
                        counted += 1
                        mc[s, k, a['gid'][f, g], a['tid'][f, col]] += 1
                tp[s, k] += counted
                fn[s, k] += n - counted
                fp[s, k] += m - counted
    return tp, fn, fp, mc


def differs(got, want):
    return [k for k in CLEAR_KEYS if not np.array_equal(got[k], want[k])]


def test_the_variant_with_nothing_wrong_is_the_yardstick():
    for name in ('unprocessed', 'empty_sequences', 'nc4_by_cols'):
        a, h, c, _ = mr.case(name)
        assert differs(clear_variant(a), c) == [], name
        tp, fn, fp, mc = hota_counts(a, h)
        assert all(np.array_equal(x, h[k]) for x, k in ((tp, 'tp'), (fn, 'fn'), (fp, 'fp'), (mc, 'mc'))), name
    for name in ('empty_frames', 'empty_tracker_8_of_10'):
        a = mr.hand(name)
        assert differs(clear_variant(a), ref.clear(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'])) == []


# ------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize('name', sorted(mr.CASES))
def test_generated_cases_have_a_margin_and_every_event(name):
    a, h, c, margin = mr.case(name)
    cm = ref.clear_metrics(c)
    assert margin >= mr.MARGIN, margin
    assert cm['IDSW'] > 0 and cm['FN'] > 0 and cm['FP'] > 0 and cm['Frag'] > 0 and cm['TP'] > 0
    assert sizes(a) == [fr for q in mr.CASES[name] for fr in q['frames']]
    assert a['sim'].shape == (len(a['ng']), max(int(a['ng'].max()), 1), max(int(a['nt'].max()), 1))
    assert a['seq_start'].tolist() == np.cumsum([0] + [len(q['frames']) for q in mr.CASES[name]]).tolist()
    for s in range(len(a['seq_start']) - 1):                 # ids are dense per sequence, in order of first appearance
        lo, hi = a['seq_start'][s:s + 2]
        for ids, cnt in ((a['gid'], a['ng']), (a['tid'], a['nt'])):
            flat = np.concatenate([ids[f, :cnt[f]] for f in range(lo, hi)] + [np.zeros(0, np.int32)])
            first = flat[np.sort(np.unique(flat, return_index=True)[1])]
            assert first.tolist() == list(range(len(first)))
    print('%s (seed %d): margin %.3g, TP %d FN %d FP %d IDSW %d Frag %d' % (name, mr.SEEDS[name], margin, cm['TP'], cm['FN'], cm['FP'], cm['IDSW'], cm['Frag']))


@pytest.mark.parametrize('name', sorted(set(mr.CASES) - {'full_256'}))       # full_256 takes seconds per seed; its seed is the first one
def test_the_recorded_seed_is_what_the_search_settles_on(name):
    assert mr.find_seed(name) == mr.SEEDS[name]


def test_nc1_edge_runs_the_last_sizes_of_the_one_column_form():
    a, h, c, _ = mr.case('nc1_edge')
    assert sizes(a) == [(64, 64), (63, 64), (64, 1), (1, 64)] and nc4(a) == []
    for match in (h['match'], c['clear_match']):
        rows, cols = mr.matched_slots(a, match)
        assert 63 in rows and 63 in cols and 0 in rows and 0 in cols
        assert all((match[f, :a['ng'][f]] >= 0).any() for f in range(4))                  # the single column / the single row matched too


def test_nc4_by_rows_and_by_columns():
    a, h, c, _ = mr.case('nc4_by_rows')
    assert sizes(a) == [(65, 3), (70, 40), (66, 64), (65, 64)] and nc4(a) == [0, 1, 2, 3] and int(a['nt'].max()) <= 64
    assert a['sim'].shape[1] == 70                            # a second, partly filled block of 64 in the count loops
    for match in (h['match'], c['clear_match']):
        rows, cols = mr.matched_slots(a, match)
        assert max(rows) >= 64 and {t % 4 for t in cols} == {0, 1, 2, 3} and max(cols) == 63
        assert (match[0, :65] >= 0).any() and all((match[f, 64:a['ng'][f]] >= 0).any() for f in (1, 2, 3))
    a, h, c, _ = mr.case('nc4_by_cols')
    assert sizes(a) == [(3, 65), (40, 70), (64, 65), (30, 67)] and nc4(a) == [0, 1, 2, 3] and int(a['ng'].max()) <= 64
    assert sorted({m % 4 for _, m in sizes(a)}) == [1, 2, 3]
    for match in (h['match'], c['clear_match']):
        rows, cols = mr.matched_slots(a, match)
        assert 64 in cols and max(cols) > 64 and {t % 4 for t in cols} == {0, 1, 2, 3}
        assert {t % 4 for t in cols if t >= 64} >= {0, 1}


def test_mixed_forms_changes_the_form_inside_one_sequence():
    a, h, c, _ = mr.case('mixed_forms')
    assert sizes(a) == [(5, 5), (130, 129), (64, 64), (65, 65), (2, 130), (130, 2)] and a['seq_start'].tolist() == [0, 6]
    assert nc4(a) == [1, 3, 4, 5] and a['sim'].shape[1:] == (130, 129 + 1)
    for match in (h['match'], c['clear_match']):
        assert all((match[f, :a['ng'][f]] >= 0).any() for f in range(6))
        assert max(mr.matched_slots(a, match, [1])[0]) >= 128 and max(mr.matched_slots(a, match, [1])[1]) >= 128
        assert (match[0, 5:] == -1).all() and (match[4, 2:] == -1).all()                # whole blocks of 64 beyond ng
    # the carried state crosses from one form to the other: the bonus decides in a frame of each form that follows one of the other
    decided = mr.bonus_decided(a, c)
    assert differs(clear_variant(a, bonus=0.0), c) != [] and decided != []
    ids_before = set(a['gid'][1, :130].tolist())
    assert ids_before & set(a['gid'][2, :64].tolist()) and set(a['gid'][2, :64].tolist()) & set(a['gid'][3, :65].tolist())


def test_full_256_fills_every_lane_and_column():
    a, h, c, _ = mr.case('full_256')
    assert sizes(a)[:2] == [(256, 256), (256, 250)] and len(sizes(a)) == 3 and a['sim'].shape[1:] == (256, 256)
    n_gid, n_tid = h['potential'].shape[1:]
    assert n_gid * n_tid > 256 * 256                         # more than 256 blocks of the alignment kernel
    for match in (h['match'], c['clear_match']):
        for f in (0, 1):
            rows, cols = mr.matched_slots(a, match, [f])
            assert max(rows) >= 192 and max(cols) >= 192 and {t % 4 for t in cols if t >= 192} == {0, 1, 2, 3}
            assert all(any(lo <= r < lo + 64 for r in rows) for lo in (0, 64, 128, 192))


def test_empty_sequences_keep_every_frame_in_its_own_sequence():
    a, h, c, _ = mr.case('empty_sequences')
    assert a['seq_start'].tolist() == [0, 0, 3, 3, 3, 7, 7] and int(a['ng'].max()) <= 8 and int(a['nt'].max()) <= 8
    for s in (0, 2, 3, 5):
        for k in ('potential', 'gcount', 'tcount', 'tp', 'fn', 'fp', 'loc', 'mc', 'counts', 'simsum', 'idcount', 'matched', 'frag'):
            assert not np.asarray(dict(h, **c)[k][s]).any(), (s, k)
    for k in ('tp', 'fn', 'fp', 'loc', 'counts', 'simsum', 'gcount', 'idcount'):          # a misattributed frame shows
        assert not np.array_equal(dict(h, **c)[k][1], dict(h, **c)[k][4]), k
    assert all((c['counts'][s] > 0).all() for s in (1, 4))
    lo = int(a['seq_start'][4])                               # the frames on either side of the doubled empty sequence differ in size
    assert sizes(a)[lo - 1] != sizes(a)[lo] and (h['match'][[0, lo - 1, lo, 6], :5] >= 0).any(1).all()


def test_unprocessed_frames_carry_prev_in_both_solver_forms():
    a, h, c, _ = mr.case('unprocessed')
    n, m = a['ng'], a['nt']
    gaps = [f for f in range(len(n)) if n[f] == 0 or m[f] == 0]
    kinds = {(bool(n[f]), bool(m[f])) for f in gaps}
    assert kinds == {(True, False), (False, True), (False, False)}
    assert any(f + 1 in gaps for f in gaps)                                               # consecutive ones
    for s in (0, 1):
        lo, hi = a['seq_start'][s:s + 2]
        assert lo in gaps and hi - 1 in gaps                                              # at the start and at the end of a sequence
    assert int(n[:a['seq_start'][1]].max()) <= 8 and int(m[:a['seq_start'][1]].max()) <= 8
    assert (70, 66) in sizes(a)[a['seq_start'][1]:]
    # at least one CLEAR match differs from the match of the same frame without the bonus, right after a gap, in either form
    hit = sorted(set(mr.bonus_decided(a, c)) & set(mr.after_a_gap(a)))
    assert [f for f in hit if n[f] > 64] and [f for f in hit if n[f] <= 64 and m[f] <= 64], hit
    # the three wrong rules show
    wrong = clear_variant(a, clear_prev_on_gap=True)
    assert 'clear_match' in differs(wrong, c) and 'frag' in differs(wrong, c)
    for s in (0, 1):                                          # ... in the small-form sequence and in the large-form one
        lo, hi = a['seq_start'][s:s + 2]
        assert not np.array_equal(wrong['clear_match'][lo:hi], c['clear_match'][lo:hi]) and not np.array_equal(wrong['frag'][s], c['frag'][s])
    assert 'clear_match' in differs(clear_variant(a, bonus=0.0), c)
    old = clear_variant(a, count_empty_tracker=False)
    assert differs(old, c) == ['idcount'] and (old['idcount'] < c['idcount']).any()
    assert (ref.clear_metrics(old)['MT'], ref.clear_metrics(old)['ML']) != (ref.clear_metrics(c)['MT'], ref.clear_metrics(c)['ML'])


def test_ragged_ids_pad_to_the_largest_sequence():
    a, h, c, _ = mr.case('ragged_ids')
    n_gid, n_tid = h['potential'].shape[1:]
    used_g = [int(a['gid'][lo:hi].max()) + 1 for lo, hi in zip(a['seq_start'][:-1], a['seq_start'][1:])]
    used_t = [int(a['tid'][lo:hi].max()) + 1 for lo, hi in zip(a['seq_start'][:-1], a['seq_start'][1:])]
    assert used_g[0] == n_gid >= 80 and used_g[1:] == [3, 1] and used_t[0] == n_tid and max(used_t[1:]) < 16
    assert (n_gid * n_tid) % 256 != 0
    for s in (1, 2):                                          # the rows a sequence does not use
        assert not h['potential'][s, used_g[s]:].any() and not h['potential'][s, :, used_t[s]:].any()
        assert not h['gcount'][s, used_g[s]:].any() and not h['tcount'][s, used_t[s]:].any() and not h['mc'][s, :, used_g[s]:].any()
        assert not c['idcount'][s, used_g[s]:].any() and h['gcount'][s, :used_g[s]].all() and c['counts'][s, 0] > 0
    assert c['idcount'][0, 64:].all() and c['matched'][0, 64:].any() and c['frag'][0, 64:].max() > 1 and h['mc'][0, :, 64:].any()


def test_tall_and_wide_have_one_column_and_one_row():
    a, h, c, _ = mr.case('tall')
    assert a['sim'].shape[1:] == (200, 1) and (a['nt'] == 1).all() and int(a['ng'].min()) == 1
    assert max(mr.matched_slots(a, h['match'])[0]) >= 128 and max(mr.matched_slots(a, c['clear_match'])[0]) >= 128
    a, h, c, _ = mr.case('wide')
    assert a['sim'].shape[1:] == (1, 200) and (a['ng'] == 1).all() and int(a['nt'].max()) == 200 and int(a['nt'].min()) == 1
    assert max(mr.matched_slots(a, h['match'])[1]) >= 128 and max(mr.matched_slots(a, c['clear_match'])[1]) >= 128


# ------------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize('name', sorted(mr.EDGES))
def test_edges_stand_on_the_decisions_and_strict_comparisons_show(name):
    a, values = mr.edges(mr.EDGES[name])
    K = len(values)
    assert (K > 64) == (name == 'edges_nc4') and sizes(a) == [(K, K)]
    h = ref.hota(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], with_margin=False)
    assert h['match'][0].tolist() == [K - 1 - g for g in range(K)]                        # isolated pairs: every one matched
    tp, fn, fp, mc = hota_counts(a, h)
    assert np.array_equal(tp, h['tp']) and np.array_equal(mc, h['mc'])
    for i, k in enumerate(mr.EDGES[name]):                    # the pair AT alpha_k counts at k; so do the steps within EPS below it
        x = 0.05 + k * 0.05
        counted = [bool(h['mc'][0, k, 4 * i + j, K - 1 - (4 * i + j)]) for j in range(4)]
        assert values[4 * i] == x == ref.ALPHAS[k] and counted[:3] == [True, True, True]
        # EPS is two steps of [0.5, 1) and at least four of what lies below: there the third step below alpha still counts
        assert counted[3] == (x - values[4 * i + 3] <= ref.EPS) == (x <= 0.5)
        if k + 1 < ref.N_ALPHA:
            assert not h['mc'][0, k + 1, 4 * i:4 * i + 4].any()
    strict = hota_counts(a, h, strict=True)
    assert not np.array_equal(strict[0], h['tp']) and not np.array_equal(strict[3], h['mc'])
    assert (h['tp'][0] - strict[0][0])[list(mr.EDGES[name])].min() >= 1
    for thr in mr.EDGE_THRS:
        c = ref.clear(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], thr, with_margin=False)
        at = 4 * (len(mr.EDGES[name]) + mr.EDGE_THRS.index(thr))
        got = (c['clear_match'][0, at:at + 4] >= 0).tolist()
        assert values[at] == thr and got == [True, True, True, thr <= 0.5], (thr, got)
        assert c['counts'][0, 0] == sum(1 for v in values if not v < thr - ref.EPS) and differs(clear_variant(a, thr), c) == []
        assert 'clear_match' in differs(clear_variant(a, thr, eps=0.0), c)               # "< thr" drops the pairs just below thr
