"""CPU: the numpy yardstick of the tracking rule (tests/track_ref.py) against closed forms, the conditions of the generated
sequences (tests/track_cases.py) that make the device comparison of tests/test_gpu_track.py meaningful, and the parts of the
library and binding that need no GPU: exported symbols, the size of the parameter struct, the host-side refusals."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import track_ref as ref
from tests import track_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = [1.5, 1.75, 4.0, 2.0, 1.0, 20.0, 0.5]
NEW = ('rtm3d_track_default_params', 'rtm3d_tracks_state_bytes', 'rtm3d_tracks_workspace_bytes', 'rtm3d_tracks_update')


def records(boxes, topk=6, scores=None, classes=None):
    r = np.zeros((topk, 32), np.float32)
    for k, b in enumerate(boxes):
        r[k, 0] = 0 if classes is None else classes[k]
        r[k, 1] = 0.9 - 0.01 * k if scores is None else scores[k]
        r[k, 24:31] = b
        r[k, 31] = 2
    return r


def moved(x=0.0, z=0.0, ry=None):
    b = list(BOX)
    b[3] += x
    b[5] += z
    if ry is not None:
        b[6] = ry
    return b


DIST = ref.params(metric='dist', thresh=-5.0)


def test_first_update_gain_and_covariance():
    st = ref.Stream(4)
    ids, _ = ref.step(st, records([BOX]), 1.0, None, DIST)
    s = st.slots[0]
    assert ids[0] == 1 and s[0] == 1 and tuple(s[17:22]) == (10.0, 0.0, 1e4, 10.0, 10.0) and tuple(s[14:17]) == (0, 0, 0)
    ref.step(st, records([moved(x=1.0)]), 1.0, None, DIST)
    # predicted P = [[10 + 1e4, 1e4], [1e4, 1e4 + 0.01]], S = 10011: K = (10010, 1e4) / 10011
    Kp, Kv = 10010.0 / 10011.0, 1e4 / 10011.0
    want = [10010.0 - Kp * 10010.0, 1e4 - Kp * 1e4, 1e4 + 0.01 - Kv * 1e4, 10.0 - 10.0 / 11.0 * 10.0, 10.0 - 10.0 / 11.0 * 10.0]
    assert np.allclose(s[17:22], want, rtol=1e-12, atol=0)
    x0 = np.float64(np.float32(BOX[3]))
    y = np.float64(np.float32(BOX[3] + 1.0)) - x0
    assert abs(s[10] - (x0 + Kp * y)) < 1e-12 and abs(s[14] - Kv * y) < 1e-12
    assert s[2] == 2 and s[3] == 2 and s[4] == 0 and s[6] == 0


def test_noiseless_constant_velocity_converges():
    st = ref.Stream(4)
    v = np.array([0.5, 0.0, -0.25])
    err = []
    for f in range(12):
        b = list(BOX)
        b[3:6] = np.array(BOX[3:6]) + v * f
        ids, _ = ref.step(st, records([b]), 1.0, None, DIST)
        assert abs(ids[0]) == 1
        err.append(np.abs(st.slots[0, 14:17] - v).max())
    # the first estimate is Kv * v with Kv = 1e4 / 10011 (fp32 positions: 2e-6 of slack); every later update shrinks the error
    assert abs(err[1] - 0.5 * 11.0 / 10011.0) < 1e-5
    assert all(b <= a for a, b in zip(err[1:], err[2:])) and err[-1] < err[1] / 100


def test_heading_flip_leaves_ry_continuous():
    st = ref.Stream(4)
    for f in range(3):
        ref.step(st, records([moved(ry=1.2)]), 1.0, None, DIST)
    before = st.slots[0, 13]
    ids, margin = ref.step(st, records([moved(ry=1.2 + np.pi)]), 1.0, None, DIST)
    # the rule turns the PREDICTED ry by pi towards the detection, so the stored angle follows the detection's end of the box; what
    # stays continuous is the box itself: its axis (ry modulo pi) does not swing through the angles between the two ends
    after = st.slots[0, 13]
    assert ids[0] == 1 and abs(ref.wrap(2.0 * (after - before))) / 2.0 < 1e-6 and -np.pi <= after < np.pi
    assert abs(abs(ref.wrap(after - before)) - np.pi) < 1e-6
    back, _ = ref.step(st, records([moved(ry=1.2)]), 1.0, None, DIST)             # and back again: the same track, the first angle
    assert back[0] == 1 and abs(ref.wrap(st.slots[0, 13] - before)) < 1e-6
    assert abs(margin - np.pi / 2) < 1e-6                    # the heading difference was pi: pi / 2 from the decision
    # and near the seam: -3.1 and 3.1 are 0.083 apart
    st = ref.Stream(4)
    ref.step(st, records([moved(ry=3.1)]), 1.0, None, DIST)
    ref.step(st, records([moved(ry=-3.1)]), 1.0, None, DIST)
    assert abs(ref.wrap(st.slots[0, 13] - 3.1)) < 0.09


def test_ego_rotation_about_y_moves_ry_by_the_angle():
    a = 0.3
    c, s = np.cos(a), np.sin(a)
    ego = np.array([[c, 0, s, 0.5], [0, 1, 0, 0], [-s, 0, c, -1.0]]).reshape(12)
    for ry in (0.5, 3.0, -2.9):
        st = ref.Stream(2)
        ref.step(st, records([moved(ry=ry)]), 1.0, None, DIST)
        slot = st.slots[0].copy()
        ref.predict(slot, 1.0, ego)
        assert abs(ref.wrap(slot[13] - (np.float64(np.float32(ry)) + a))) < 1e-12
        x, z = np.float64(np.float32(BOX[3])), np.float64(np.float32(BOX[5]))
        assert np.allclose(slot[10:13], [c * x + s * z + 0.5, 1.0, -s * x + c * z - 1.0], rtol=0, atol=1e-12)
        # a static object seen from the moved camera is matched and stays static
        det = moved(ry=ry + a)
        det[3], det[5] = c * BOX[3] + s * BOX[5] + 0.5, -s * BOX[3] + c * BOX[5] - 1.0
        ids, _ = ref.step(st, records([det]), 1.0, ego, DIST)
        assert ids[0] == 1 and np.abs(st.slots[0, 14:17]).max() < 1e-5


def test_greedy_ties_resolve_to_the_lower_slot():
    st = ref.Stream(4)
    ref.step(st, records([moved(x=-1.0), moved(x=1.0)]), 1.0, None, DIST)
    ids, margin = ref.step(st, records([moved()]), 1.0, None, DIST)           # equidistant from both tracks
    assert ids[0] == 1 and margin == 0.0 and st.slots[0, 6] == 0 and st.slots[1, 6] == -1
    st = ref.Stream(4)
    ref.step(st, records([moved()]), 1.0, None, DIST)
    ids, margin = ref.step(st, records([moved(x=-1.0), moved(x=1.0)], scores=[0.5, 0.5]), 1.0, None, DIST)   # one track, two detections
    assert list(ids[:2]) == [1, 2] and margin == 0.0
    # the global order, not row by row: detection 0 is nearer to track 2 than to track 1, which then takes detection 1
    st = ref.Stream(4)
    ref.step(st, records([moved(x=-2.0), moved(x=2.0)]), 1.0, None, DIST)
    ids, _ = ref.step(st, records([moved(x=1.0), moved(x=-0.5)]), 1.0, None, DIST)
    assert list(ids[:2]) == [2, 1]


def test_table_full_drops_the_lowest_scores_and_counts_them():
    st = ref.Stream(2)
    ids, _ = ref.step(st, records([moved(x=10.0 * i) for i in range(4)]), 1.0, None, DIST)
    assert list(ids[:4]) == [1, 2, 0, 0] and tuple(st.header[:3]) == (2, 1, 2)
    ids, _ = ref.step(st, records([moved(x=10.0 * i) for i in range(4)]), 1.0, None, DIST)
    assert list(ids[:4]) == [1, 2, 0, 0] and tuple(st.header[:3]) == (2, 2, 4)


def test_gap_of_max_misses_keeps_the_id_and_one_more_loses_it():
    for gap, want in ((2, 1), (3, 2)):
        st = ref.Stream(4)
        P = ref.params(metric='dist', thresh=-5.0, max_misses=2)
        ref.step(st, records([BOX]), 1.0, None, P)
        for g in range(gap):
            ids, _ = ref.step(st, records([]), 1.0, None, P)
            assert not ids.any()
            assert (st.slots[0, 0] != 0) == (g + 1 <= 2) and (st.slots[0, 0] == 0 or (st.slots[0, 4] == g + 1 and st.slots[0, 3] == 0))
        ids, _ = ref.step(st, records([BOX]), 1.0, None, P)
        assert abs(ids[0]) == want


def test_confirmation_after_min_hits():
    P = ref.params(metric='dist', thresh=-5.0, min_hits=3)
    st = ref.Stream(4)
    signs = []
    for f in range(8):
        boxes = [BOX] + ([moved(x=20.0)] if f >= 4 else [])
        ids, _ = ref.step(st, records(boxes), 1.0, None, P)
        signs.append(list(ids[:2]))
    assert [s[0] for s in signs] == [1] * 8                              # frames 1 - 3: confirmed at once, then by its hits
    assert [s[1] for s in signs] == [0, 0, 0, 0, -2, -2, 2, 2]           # born in frame 5: tentative until its third hit
    # a miss takes the confirmation away again
    ref.step(st, records([BOX]), 1.0, None, P)
    ids, _ = ref.step(st, records([BOX, moved(x=20.0)]), 1.0, None, P)
    assert list(ids[:2]) == [1, -2]


def test_junk_slots_are_no_detections():
    r = records([BOX, moved(x=10.0), moved(x=20.0), moved(x=30.0)], scores=[0.9, 0.8, 0.2, 0.7])
    r[1, 31] = 1
    assert ref.detections(r, 0.3) == [0, 3]
    ids, _ = ref.step(ref.Stream(4), r, 1.0, None, ref.params(min_score=0.3))
    assert list(ids[:5]) == [1, 0, 0, 2, 0]


CASES = tc.cases()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_case_conditions(case):
    res = tc.reference(case)
    assert len(res) == 12 and min(float(r[2].min()) for r in res) >= tc.MARGIN
    B, T = case['frames'][0].shape[0], case['T']
    slots = [r[1][:, ref.HEADER:].reshape(B, T, ref.SLOT) for r in res]
    live = [int((s[..., 0] != 0).sum(1).max()) for s in slots]
    ndet = [max(len(ref.detections(f[b], case['params']['min_score'])) for b in range(B)) for f in case['frames']]
    flags = np.concatenate([f[..., 31].reshape(-1) for f in case['frames']])
    assert (flags == 1).any() and (flags == 0).any() and (flags == 2).any()
    assert case['topk'] == 7 or any((f[..., 31] == 2).any() and (f[f[..., 31] == 2][:, 1] < case['params']['min_score']).any() for f in case['frames'])
    if case['name'] == 'dense_3d':
        assert max(live) >= 70 and max(ndet) >= 70 and ndet[1] > live[0] and ndet[8] < live[7]
        id3 = res[0][0][0][case['frames'][0][0, :, 1] == np.float32(0.95 - 0.015)]
        # object 3 (a gap of two frames) keeps its id, object 9 (three) comes back with a new one: one id more than objects
        assert res[-1][1][0, 0] == 75 and abs(int(id3[0])) in np.abs(res[-1][0][0])
        assert any(float(r[2].min()) < 1.0 for r in res)                 # the flipped heading was decided somewhere
    if case['name'] == 'overflow_bev':
        assert res[-1][1][0, 2] > 0 and max(live) == 8 and res[-1][1][0, 0] > 8
    if case['name'] == 'three_streams_classes':
        assert B == 3 and ndet[5] == 5 and not res[5][0][1].any() and not res[0][0][2].any()
        assert any((r[0] < 0).any() for r in res) and any((r[0] > 0).any() for r in res)
    if case['name'] == 'crossing_dist_ego':
        assert case['egos'] is not None and min(float(r[2].min()) for r in res[1:]) < 0.1      # the crossing pair competed


# ------------------------------------------------------------------------------------------------ library and binding
def test_header_library_and_binding_agree():
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert re.search(r'#define RTM3D_ABI_VERSION 9\b', hdr) and _lib.ABI_VERSION == 9
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        m = re.search(r'\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert 'typedef struct rtm3d_track_params' in hdr
    assert '#define RTM3D_TRACK_HEADER_DOUBLES %d' % ref.HEADER in hdr and '#define RTM3D_TRACK_SLOT_DOUBLES %d' % ref.SLOT in hdr


def test_track_params_size_and_defaults_match_c(tmp_path):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no C compiler'
    src = ('#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%%zu %%zu %%zu", sizeof(rtm3d_track_params), offsetof(rtm3d_track_params, thresh), '
           'offsetof(rtm3d_track_params, r_dim));return 0;}' % REPO)
    exe = str(tmp_path / 'sizeof_track_params')
    subprocess.run([cc, '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    size, o_thresh, o_rdim = [int(v) for v in subprocess.check_output([exe]).split()]
    C = _lib.TrackParamsC
    assert (size, o_thresh, o_rdim) == (ctypes.sizeof(C), C.thresh.offset, C.r_dim.offset)
    from rtm3d_amd import track
    p = C()
    assert _lib.load().rtm3d_track_default_params(ctypes.byref(p)) == 0
    d = track.TrackParams().to_c()
    assert bytes(p) == bytes(d)
    want = dict(ref.DEFAULTS, metric=ref.METRICS[ref.DEFAULTS['metric']], class_aware=0)
    assert {k: getattr(p, k) for k, _ in C._fields_} == want
    assert track.HEADER == ref.HEADER and track.SLOT == ref.SLOT and track.METRICS == ref.METRICS


def test_sizes():
    lib = _lib.load()
    assert lib.rtm3d_tracks_state_bytes(3, 128) == 3 * (8 + 24 * 128) * 8
    assert lib.rtm3d_tracks_workspace_bytes(3, 100, 128) == 3 * 100 * 128 * 8
    assert lib.rtm3d_tracks_state_bytes(1, 0) == 0 and lib.rtm3d_tracks_state_bytes(1, 257) == 0 and lib.rtm3d_tracks_state_bytes(0, 8) == 0
    assert lib.rtm3d_tracks_workspace_bytes(1, 257, 8) == 0 and lib.rtm3d_tracks_workspace_bytes(1, 0, 8) == 0


def test_update_refusals_need_no_gpu():
    """Every argument is checked before anything is launched: the pointers below are never dereferenced."""
    lib = _lib.load()
    p = _lib.TrackParamsC()
    assert lib.rtm3d_track_default_params(ctypes.byref(p)) == 0
    fake = ctypes.c_void_p(0x1000)

    def call(B=1, topk=100, T=128, rec=fake, dt=1.0, params=p, state=fake, ids=fake, ws=fake):
        rc = lib.rtm3d_tracks_update(None, B, topk, T, rec, dt, None, None if params is None else ctypes.byref(params), state, ids, ws)
        return rc, lib.rtm3d_last_error().decode()

    for kw, word in ((dict(T=0), 'T 0'), (dict(T=257), 'T 257'), (dict(topk=257), 'topk 257'), (dict(topk=0), 'topk 0'), (dict(dt=0.0), 'dt'),
                     (dict(dt=-1.0), 'dt'), (dict(dt=float('nan')), 'dt'), (dict(dt=float('inf')), 'dt'), (dict(state=None), 'null'),
                     (dict(rec=None), 'null'), (dict(ids=None), 'null'), (dict(ws=None), 'null'), (dict(params=None), 'params'),
                     (dict(B=0), 'B 0')):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and msg.startswith('tracks_update'), (kw, msg)
    for field, bad, word in (('metric', 3, 'metric 3'), ('metric', -1, 'metric'), ('max_misses', -1, 'max_misses'), ('thresh', float('nan'), 'NaN'),
                             ('r_pos', 0.0, 'measurement'), ('q_vel', -1.0, 'process noise'), ('p0_vel', float('inf'), 'variances')):
        q = _lib.TrackParamsC.from_buffer_copy(p)
        setattr(q, field, bad)
        rc, msg = call(params=q)
        assert rc != 0 and word in msg, (field, msg)
    assert lib.rtm3d_track_default_params(None) != 0


def test_python_refusals_and_engine_signatures():
    import torch
    from rtm3d_amd import track, engine
    for fn in (engine.Engine.detect, engine.Engine.detect_frames):
        sig = inspect.signature(fn)
        assert sig.parameters['tracker'].default is None
    sig = inspect.signature(track.Tracker.__init__)
    assert sig.parameters['capacity'].default == 128 and sig.parameters['params'].default is None and sig.parameters['device'].default == 'cuda'
    sig = inspect.signature(track.Tracker.update)
    assert sig.parameters['dt'].default == 1.0 and sig.parameters['ego'].default is None
    with pytest.raises(ValueError, match='metric'):
        track.TrackParams(metric='giou')
    with pytest.raises(ValueError, match='unknown'):
        track.TrackParams(threshold=0.1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        track.Tracker(1, device='cpu')
    assert torch.float64 is not None
