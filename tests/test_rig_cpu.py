"""CPU: the numpy yardstick of the rig-fusion rule (tests/rig_ref.py) against closed forms, the conditions of the generated cases
(tests/rig_cases.py) that make the device comparison of tests/test_gpu_rig.py meaningful, and the parts of the library and
binding that need no GPU: exported symbols, the size of the parameter struct, the host-side refusals of both entry points, the
host-side check of the extrinsics."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import rig_ref as ref
from tests import rig_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rtm3d_rig_default_params', 'rtm3d_rig_workspace_bytes', 'rtm3d_rig_fuse', 'rtm3d_rig_scatter_ids')
BOX = np.array([1.5, 1.75, 4.0, 2.0, 1.0, 20.0, 0.5])


def records(C, topk, rows):
    """rows: [(camera, slot, score, cls, box7)]"""
    r = np.zeros((C, topk, 32), np.float32)
    for c, k, score, cls, box in rows:
        r[c, k, 0], r[c, k, 1], r[c, k, 31] = cls, score, 2
        r[c, k, 24:31] = box
    return r


def seen_from(box, E):
    p, ry = rc.to_camera(box[3:6], box[6], E)
    return np.concatenate([box[:3], p, [ry]])


def ident(C):
    return np.stack([rc.ext_matrix(0.0)] * C).reshape(C, 12)


def at(x, z=20.0, ry=0.5):
    b = BOX.copy()
    b[3], b[5], b[6] = x, z, ry
    return b


def test_one_box_seen_by_two_cameras_fuses_to_the_box():
    ext = np.stack([rc.ext_matrix(0.4, t=(1.0, 0.0, 0.5)), rc.ext_matrix(-1.1, t=(-0.7, 0.2, 0.0))])
    rec = records(2, 4, [(0, 0, 0.9, 0, seen_from(BOX, ext[0])), (1, 1, 0.6, 0, seen_from(BOX, ext[1]))])
    for merge in ('mean', 'best'):
        res = ref.fuse(rec, ext, 1, 2, ref.params(merge=merge))
        assert tuple(res['n'][0]) == (1, 0) and tuple(res['info'][0, 0]) == (0, 0, 2, 0b11)
        assert res['map'].tolist() == [[0, -1, -1, -1], [-1, 0, -1, -1]]
        assert np.abs(res['box'][0, 0] - BOX).max() < 1e-5                     # fp32 records: 2e-6 of slack in 20 m
        assert res['out'][0, 0, 0] == 0 and res['out'][0, 0, 1] == np.float32(0.9) and res['out'][0, 0, 31] == 2
        assert not res['out'][0, 0, 2:24].any() and not res['out'][0, 1:].any() and not res['info'][0, 1:].any()
        assert np.array_equal(res['out'][0, 0, 24:31], res['box'][0, 0].astype(np.float32))
    # the mean is the score-weighted one: move camera 1's view by 1 m in x, the fused x moves by 0.6 / 1.5 of it
    moved = BOX.copy()
    moved[3] += 1.0
    rec = records(2, 4, [(0, 0, 0.9, 0, seen_from(BOX, ext[0])), (1, 1, 0.6, 0, seen_from(moved, ext[1]))])
    res = ref.fuse(rec, ext, 1, 2, ref.params(merge='mean'))
    w0, w1 = np.float64(np.float32(0.9)), np.float64(np.float32(0.6))
    assert abs(res['box'][0, 0, 3] - (BOX[3] + w1 / (w0 + w1))) < 1e-5 and res['info'][0, 0, 2] == 2


def test_a_yaw_of_the_extrinsic_moves_ry_by_the_angle():
    for a in (0.3, -2.0, 3.0):
        E = rc.ext_matrix(a, t=(0.5, -0.1, 2.0)).reshape(12)
        for ry in (0.5, 3.0, -2.9):
            b = ref.transform(at(2.0, ry=ry), E)
            assert abs(ref.wrap(b[6] - (ry + a))) < 1e-12 and -np.pi <= b[6] < np.pi
            c, s = np.cos(a), np.sin(a)
            assert np.allclose(b[3:6], [c * 2.0 + s * 20.0 + 0.5, 1.0 - 0.1, -s * 2.0 + c * 20.0 + 2.0], rtol=0, atol=1e-12)
            assert tuple(b[:3]) == tuple(BOX[:3])
    # pitch and roll: the centre moves exactly, the heading keeps its projection into the x-z plane
    E = rc.ext_matrix(0.3, 0.1, -0.05, (0.0, 0.0, 0.0))
    b = ref.transform(at(2.0, ry=0.7), E.reshape(12))
    assert np.allclose(b[3:6], E[:, :3] @ np.array([2.0, 1.0, 20.0]), rtol=0, atol=1e-12)
    h = E[:, :3] @ np.array([np.cos(0.7), 0.0, -np.sin(0.7)])
    assert abs(ref.wrap(b[6] - np.arctan2(-h[2], h[0]))) < 1e-12


def test_same_camera_duplicates_stay_apart_under_cross_only():
    rec = records(2, 4, [(0, 0, 0.9, 0, at(2.0)), (0, 1, 0.8, 0, at(2.1))])
    res = ref.fuse(rec, ident(2), 1, 2, ref.params(cross_only=True))
    assert tuple(res['n'][0]) == (2, 0) and res['map'][0, :2].tolist() == [0, 1] and res['info'][0, :2, 2].tolist() == [1, 1]
    res = ref.fuse(rec, ident(2), 1, 2, ref.params(cross_only=False))
    assert tuple(res['n'][0]) == (1, 0) and res['map'][0, :2].tolist() == [0, 0] and tuple(res['info'][0, 0]) == (0, 0, 2, 0b01)
    # ... but two boxes of one camera meet in the cluster of another camera's representative
    rec = records(2, 4, [(1, 0, 0.95, 0, at(2.05)), (0, 0, 0.9, 0, at(2.0)), (0, 1, 0.8, 0, at(2.1))])
    res = ref.fuse(rec, ident(2), 1, 2, ref.params(cross_only=True))
    assert tuple(res['n'][0]) == (1, 0) and tuple(res['info'][0, 0]) == (1, 0, 3, 0b11) and res['map'][0, :2].tolist() == [0, 0]
    # class_aware keeps two classes at one place apart
    rec = records(2, 4, [(0, 0, 0.9, 0, at(2.0)), (1, 0, 0.8, 1, at(2.0))])
    assert tuple(ref.fuse(rec, ident(2), 1, 2, ref.params(class_aware=True))['n'][0]) == (2, 0)
    assert tuple(ref.fuse(rec, ident(2), 1, 2, ref.params(class_aware=False))['n'][0]) == (1, 0)


def test_members_never_attract():
    P = ref.params(metric='dist', thresh=-1.5)
    rec = records(3, 2, [(0, 0, 0.9, 0, at(0.0)), (1, 0, 0.8, 0, at(1.0)), (2, 0, 0.7, 0, at(2.0))])
    res = ref.fuse(rec, ident(3), 1, 3, P)
    assert tuple(res['n'][0]) == (2, 0) and res['map'][:, 0].tolist() == [0, 0, 1]
    assert tuple(res['info'][0, 0]) == (0, 0, 2, 0b011) and tuple(res['info'][0, 1]) == (2, 0, 1, 0b100)
    assert abs(res['margin'] - 0.5) < 1e-6
    # the earliest representative wins, not the nearest: C is 1.4 from A and 0.1 from the later representative D
    rec = records(4, 2, [(0, 0, 0.9, 0, at(0.0)), (1, 0, 0.85, 0, at(1.6)), (2, 0, 0.7, 0, at(1.4))])
    res = ref.fuse(rec, ident(4)[:3], 1, 3, P)
    assert res['map'][:, 0].tolist() == [0, 1, 0]


def test_overflow_drops_the_lowest_scores_and_counts_them():
    rows = [(c, k, 0.9 - 0.1 * c - 0.01 * k, 0, at(10.0 * (2 * c + k))) for c in range(2) for k in range(2)]
    res = ref.fuse(records(2, 3, rows), ident(2), 1, 2, ref.params(), cap=3)
    assert tuple(res['n'][0]) == (3, 1) and res['map'].tolist() == [[0, 1, -1], [2, -2, -1]]
    assert res['out'].shape == (1, 3, 32) and (res['out'][0, :, 31] == 2).all()
    assert list(res['out'][0, :, 1]) == sorted(res['out'][0, :, 1], reverse=True) and len(res['clusters'][0]) == 4


def test_equal_scores_go_to_the_lower_camera_then_the_lower_slot():
    rows = [(1, 0, 0.5, 0, at(0.0)), (0, 2, 0.5, 0, at(10.0)), (0, 1, 0.5, 0, at(20.0)), (1, 1, 0.7, 0, at(30.0))]
    rec = records(2, 3, rows)
    assert ref.candidates(rec, 0.0) == [(1, 1), (0, 1), (0, 2), (1, 0)]
    res = ref.fuse(rec, ident(2), 1, 2, ref.params())
    assert res['info'][0, :4, :2].tolist() == [[1, 1], [0, 1], [0, 2], [1, 0]]
    # twins with equal scores: camera 0 is the representative
    res = ref.fuse(records(2, 3, [(1, 0, 0.5, 0, at(0.0)), (0, 2, 0.5, 0, at(0.0))]), ident(2), 1, 2, ref.params())
    assert tuple(res['info'][0, 0]) == (0, 2, 2, 0b11)
    # -0 and +0 tie; a NaN score and a score below min_score are no candidates
    rec = records(2, 3, [(1, 0, 0.0, 0, at(0.0)), (0, 0, -0.0, 0, at(10.0)), (0, 1, np.nan, 0, at(20.0)), (0, 2, -0.5, 0, at(30.0))])
    assert ref.candidates(rec, 0.0) == [(0, 0), (1, 0)]
    assert ref.candidates(rec, -1.0) == [(0, 0), (1, 0), (0, 2)]


def test_heading_fold_of_twins_seen_from_opposite_ends():
    a, b = at(2.0, ry=1.2), at(2.0, ry=1.2 - np.pi + 0.02)
    far = ref.params(metric='dist', thresh=-10.0)              # the pair is 10 from its bar: the margin is the heading's
    res = ref.fuse(records(2, 2, [(0, 0, 0.8, 0, a), (1, 0, 0.8, 0, b)]), ident(2), 1, 2, far)
    assert res['info'][0, 0, 2] == 2 and abs(res['box'][0, 0, 6] - 1.21) < 1e-6
    assert abs(res['margin'] - (np.pi / 2 - 0.02)) < 1e-6
    res = ref.fuse(records(2, 2, [(0, 0, 0.8, 0, at(2.0, ry=3.1)), (1, 0, 0.8, 0, at(2.0, ry=-3.1))]), ident(2), 1, 2, ref.params())
    assert abs(abs(res['box'][0, 0, 6]) - np.pi) < 1e-6 and -np.pi <= res['box'][0, 0, 6] < np.pi


CASES = rc.cases()


def kept(rec, min_score):
    with np.errstate(invalid='ignore'):
        return (rec[..., 31] == 2) & (rec[..., 1].astype(np.float64) >= min_score)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_case_conditions(case):
    res = rc.reference(case)
    R, C, topk, cap, P = case['R'], case['C'], case['topk'], case['cap'], case['params']
    rec = case['rec']
    assert res['margin'] >= rc.MARGIN and rec.shape == (R * C, topk, 32) and case['ext'].shape == (R, C, 12)
    k = kept(rec, P['min_score'])
    assert ((res['map'] == -1) == ~k).all() and int(res['n'].sum()) == sum(len(c) for c in res['clusters'])
    name = case['name']
    if name == 'one_camera_passthrough':
        n = int(k.sum())
        assert (C, topk) == (1, 4) and n == 3 and tuple(res['n'][0]) == (n, 0) and (rec[0, :, 31] == 1).any()
        assert np.array_equal(res['out'][0, :n, 24:30], rec[0][k[0]][:, 24:30]) and np.array_equal(res['out'][0, :n, :2], rec[0][k[0]][:, :2])
        assert res['info'][0, :n, 1].tolist() == np.flatnonzero(k[0]).tolist() and (res['info'][0, :n, 2] == 1).all()
    if name == 'two_cameras_ties_and_flip':
        assert (C, topk) == (2, 8)
        twins = [c for c in res['clusters'][0] if len(c) == 2 and rec[c[0][0], c[0][1], 1] == rec[c[1][0], c[1][1], 1]]
        assert twins and all(c[0][0] == 0 for c in twins)                                    # equal scores: camera 0 represents
        sc = rec[..., 1][k]
        assert (np.unique(sc, return_counts=True)[1] >= 2).sum() >= 2                        # and a tie between unrelated boxes
        assert (rec[..., 31] == 0).any() and (rec[..., 31] == 1).any()
        ext = case['ext'][0]
        turned = [abs(float(ref.wrap(ref.transform(rec[c[0]][24:31].astype(np.float64), ext[c[0][0]])[6]
                                     - ref.transform(rec[c[1]][24:31].astype(np.float64), ext[c[1][0]])[6]))) for c in res['clusters'][0] if len(c) == 2]
        assert sum(t > 3.0 for t in turned) == 1 and sum(t < 0.2 for t in turned) >= 2         # one pair of twins seen from opposite ends
        assert any(len(c) == 2 for c in res['clusters'][0]) and any(len(c) == 1 for c in res['clusters'][0])
    if name == 'three_cameras_chain_dist':
        assert (C, topk) == (3, 7) and P['metric'] == 'dist' and not P['class_aware']
        cl = res['clusters'][0]
        info = res['info'][0]
        assert len(cl[0]) == 2 and cl[0][0][0] == 0 and cl[0][1][0] == 1                   # A with B
        assert len(cl[1]) == 1 and cl[1][0][0] == 2                                        # C alone: B, a member, does not attract it
        three = [c for c in cl if len(c) == 3]
        assert len(three) == 1 and [m[0] for m in three[0]] == [1, 0, 0]                   # two boxes of camera 0 under camera 1's
        assert any(not np.isfinite(res['box'][0, s]).all() and info[s, 2] == 1 for s in range(int(res['n'][0, 0])))
        assert np.isnan(rec[..., 1]).any() or (rec[..., 31] == 1).any()
        assert np.abs(case['ext'].reshape(3, 3, 4)[:, 1, 0]).min() > 1e-3                   # pitch / roll: R[1][0] != 0
    if name == 'six_cameras_two_rigs':
        assert (R, C, topk) == (2, 6, 100) and P['metric'] == 'iou3d' and P['class_aware'] and P['cross_only']
        per_cam = k.sum(1)
        assert per_cam.min() >= 12 and per_cam.max() <= 40 and np.isnan(rec[..., 1]).any()
        sizes = [len(c) for r in range(2) for c in res['clusters'][r]]
        assert max(sizes) >= 3 and sizes.count(2) >= 10 and sizes.count(1) >= 10
        assert res['margin'] < 1.5                              # some flipped view was folded
        assert not np.array_equal(res['out'][0], res['out'][1])
    if name == 'sixteen_cameras_overflow':
        assert (C, topk, cap) == (16, 128, 256) and tuple(res['n'][0]) == (256, len(res['clusters'][0]) - 256) and res['n'][0, 1] > 0
        assert (res['map'] == -2).any() and (res['map'] >= 0).any()
        assert any(len(c) >= 2 and len(set(m[0] for m in c)) < len(c) for c in res['clusters'][0])   # a link inside one camera
        assert int(k.sum()) > 256
    if name == 'three_rigs_own_extrinsics':
        assert (R, C, topk) == (3, 2, 8) and len({case['ext'][r].tobytes() for r in range(3)}) == 3
        assert tuple(res['n'][1]) == (0, 0) and not res['out'][1].any() and not k[2:4].any()          # a rig that sees nothing
        assert not k[5].any() and k[4].any() and (res['info'][2, :int(res['n'][2, 0]), 3] == 1).all()   # a camera that sees nothing
        assert (res['info'][0, :int(res['n'][0, 0]), 3] == 3).all() and res['n'][0, 0] == 4


def test_the_cases_cover_the_table():
    P = [c['params'] for c in CASES]
    assert {p['metric'] for p in P} == {'bev', 'iou3d', 'dist'} and {p['merge'] for p in P} == {'best', 'mean'}
    assert {p['class_aware'] for p in P} == {True, False} and {p['cross_only'] for p in P} == {True, False}
    assert {(c['C'], c['topk']) for c in CASES} >= {(1, 4), (2, 8), (3, 7), (6, 100), (16, 128)} and {c['R'] for c in CASES} == {1, 2, 3}
    rec = np.concatenate([c['rec'].reshape(-1, 32) for c in CASES])
    with np.errstate(invalid='ignore'):
        junk = [rec[:, 31] == 0, (rec[:, 31] == 1) & (rec[:, 24] > 0), (rec[:, 31] == 2) & (rec[:, 1] < rc.MIN_SCORE), (rec[:, 31] == 2) & np.isnan(rec[:, 1])]
    assert all(j.any() for j in junk) and all(c['params']['min_score'] == rc.MIN_SCORE for c in CASES)


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
    assert 'typedef struct rtm3d_rig_params' in hdr and '#define RTM3D_RIG_MERGE_BEST 0' in hdr and '#define RTM3D_RIG_MERGE_MEAN 1' in hdr
    assert _lib.load().rtm3d_abi_version() == 9


def test_rig_params_size_and_defaults_match_c(tmp_path):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no C compiler'
    src = ('#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%%zu %%zu %%zu %%zu", sizeof(rtm3d_rig_params), offsetof(rtm3d_rig_params, merge), '
           'offsetof(rtm3d_rig_params, thresh), offsetof(rtm3d_rig_params, min_score));return 0;}' % REPO)
    exe = str(tmp_path / 'sizeof_rig_params')
    subprocess.run([cc, '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    size, o_merge, o_thresh, o_min = [int(v) for v in subprocess.check_output([exe]).split()]
    C = _lib.RigParamsC
    assert (size, o_merge, o_thresh, o_min) == (ctypes.sizeof(C), C.merge.offset, C.thresh.offset, C.min_score.offset)
    from rtm3d_amd import rig
    p = C()
    assert _lib.load().rtm3d_rig_default_params(ctypes.byref(p)) == 0
    assert bytes(p) == bytes(rig.RigParams().to_c())
    want = dict(ref.DEFAULTS, metric=ref.METRICS[ref.DEFAULTS['metric']], merge=ref.MERGES[ref.DEFAULTS['merge']], class_aware=1, cross_only=1)
    assert {k: getattr(p, k) for k, _ in C._fields_} == want
    assert (p.metric, p.thresh, p.class_aware, p.cross_only, p.merge, p.min_score) == (0, 0.1, 1, 1, 1, 0.0)
    assert rig.METRICS == ref.METRICS and rig.MERGES == ref.MERGES
    assert _lib.load().rtm3d_rig_default_params(None) != 0


def test_workspace_bytes():
    lib = _lib.load()
    one = lib.rtm3d_rig_workspace_bytes(1, 6, 100)
    # at least: the transformed boxes and one bit per ordered pair
    assert one >= 600 * 7 * 8 + 600 * 600 // 8 and one % 8 == 0 and lib.rtm3d_rig_workspace_bytes(32, 6, 100) == 32 * one
    assert lib.rtm3d_rig_workspace_bytes(1, 16, 128) > 0 and lib.rtm3d_rig_workspace_bytes(1, 1, 1) > 0
    for R, C, topk in ((0, 6, 100), (-1, 6, 100), (1, 0, 100), (1, 17, 100), (1, 6, 0), (1, 6, 257), (1, 16, 129), (1, 9, 256)):
        assert lib.rtm3d_rig_workspace_bytes(R, C, topk) == 0, (R, C, topk)


def test_refusals_need_no_gpu():
    """Every argument is checked before anything is launched: the pointers below are never dereferenced."""
    lib = _lib.load()
    p = _lib.RigParamsC()
    assert lib.rtm3d_rig_default_params(ctypes.byref(p)) == 0
    fake = ctypes.c_void_p(0x1000)

    def fuse(R=1, C=6, topk=100, cap=128, rec=fake, ext=fake, params=p, out=fake, box=None, info=fake, map=fake, n=fake, ws=fake):
        rc_ = lib.rtm3d_rig_fuse(None, R, C, topk, cap, rec, ext, None if params is None else ctypes.byref(params), out, box, info, map, n, ws)
        return rc_, lib.rtm3d_last_error().decode()

    for kw, word in ((dict(R=0), 'R 0'), (dict(C=0), 'C 0'), (dict(C=17), 'C 17'), (dict(topk=0), 'topk 0'), (dict(topk=257), 'topk 257'),
                     (dict(C=16, topk=129), 'C * topk 2064'), (dict(cap=0), 'cap 0'), (dict(cap=257), 'cap 257'), (dict(params=None), 'params'),
                     (dict(rec=None), 'null'), (dict(ext=None), 'null'), (dict(out=None), 'null'), (dict(info=None), 'null'),
                     (dict(map=None), 'null'), (dict(n=None), 'null'), (dict(ws=None), 'null')):
        rc_, msg = fuse(**kw)
        assert rc_ != 0 and word in msg and msg.startswith('rig_fuse'), (kw, msg)
    for field, bad, word in (('metric', 3, 'metric 3'), ('metric', -1, 'metric'), ('merge', 2, 'merge 2'), ('merge', -1, 'merge'),
                             ('thresh', float('nan'), 'NaN'), ('min_score', float('nan'), 'NaN')):
        q = _lib.RigParamsC.from_buffer_copy(p)
        setattr(q, field, bad)
        rc_, msg = fuse(params=q)
        assert rc_ != 0 and word in msg, (field, msg)

    def scatter(R=1, C=6, topk=100, cap=128, map=fake, ids=fake, out=fake):
        rc_ = lib.rtm3d_rig_scatter_ids(None, R, C, topk, cap, map, ids, out)
        return rc_, lib.rtm3d_last_error().decode()

    for kw, word in ((dict(R=0), 'R 0'), (dict(C=17), 'C 17'), (dict(topk=0), 'topk 0'), (dict(C=16, topk=129), 'topk 129'), (dict(cap=0), 'cap 0'),
                     (dict(cap=257), 'cap 257'), (dict(map=None), 'null'), (dict(ids=None), 'null'), (dict(out=None), 'null')):
        rc_, msg = scatter(**kw)
        assert rc_ != 0 and word in msg and msg.startswith('rig_scatter_ids'), (kw, msg)


def test_rig_checks_the_extrinsics_on_the_host():
    from rtm3d_amd import rig
    good = np.stack([rig.mount(0.3, 0.1, -0.05, (1.0, 0.0, 2.0)), rig.mount(-2.0)])
    assert np.array_equal(rig.check_extrinsics(good, 1), good[None]) and rig.check_extrinsics(good, 3).shape == (3, 2, 3, 4)
    four = np.concatenate([good, np.tile([[[0.0, 0.0, 0.0, 1.0]]], (2, 1, 1))], axis=1)
    assert np.array_equal(rig.check_extrinsics(four, 1), good[None])
    assert np.allclose(rig.mount(0.3, 0.1, -0.05, (1, 2, 3)), rc.ext_matrix(0.3, 0.1, -0.05, (1, 2, 3)), rtol=0, atol=1e-15)
    assert np.allclose(rig.mount(0.5)[:, 2], [np.sin(0.5), 0.0, np.cos(0.5)]) and np.allclose(rig.mount(0, 0.5)[:, 2], [0, -np.sin(0.5), np.cos(0.5)])
    assert np.allclose(rig.mount(0, 0, 0.5)[:, 0], [np.cos(0.5), np.sin(0.5), 0])
    skew = good.copy()
    skew[1, 0, 0] += 1e-4
    with pytest.raises(ValueError, match='camera 1.*orthonormal'):
        rig.Rig(skew)
    mirror = good.copy()
    mirror[0, :, 0] *= -1.0
    with pytest.raises(ValueError, match='camera 0.*reflection'):
        rig.Rig(mirror)
    nan = good.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match='camera 1.*finite'):
        rig.Rig(nan)
    per_rig = np.stack([good, skew])
    with pytest.raises(ValueError, match='camera 1 of rig 1'):
        rig.Rig(per_rig, R=2)
    with pytest.raises(ValueError, match='shape'):
        rig.Rig(good[0])
    with pytest.raises(ValueError, match='shape'):
        rig.Rig(per_rig, R=3)
    with pytest.raises(ValueError, match='cameras'):
        rig.Rig(np.tile(good[:1], (17, 1, 1)))
    with pytest.raises(ValueError, match='cap'):
        rig.Rig(good, cap=257)
    with pytest.raises(RuntimeError, match='no CPU path'):
        rig.Rig(good, device='cpu')
    with pytest.raises(ValueError, match='metric'):
        rig.RigParams(metric='3d')
    with pytest.raises(ValueError, match='merge'):
        rig.RigParams(merge='median')
    with pytest.raises(ValueError, match='unknown'):
        rig.RigParams(threshold=0.1)


def test_engine_method_and_older_signatures():
    from rtm3d_amd import engine, rig
    sig = inspect.signature(engine.Engine.detect_frames_rig)
    assert list(sig.parameters) == ['self', 'images', 'K_camera', 'rig', 'kitti', 'nms3d', 'tracker', 'out']
    assert [sig.parameters[k].default for k in ('kitti', 'nms3d', 'tracker', 'out')] == [False, None, None, None]
    assert list(inspect.signature(engine.Engine.detect).parameters) == ['self', 'x', 'K_per_image', 'out', 'tracker', 'nms3d']
    assert list(inspect.signature(engine.Engine.detect_frames).parameters) == ['self', 'images', 'K_camera', 'kitti', 'out', 'draw', 'tracker', 'nms3d']
    assert list(inspect.signature(engine.Engine.detect_frames_src).parameters)[:5] == ['self', 'sources', 'K_camera', 'order', 'packed']
    sig = inspect.signature(rig.Rig.__init__)
    assert list(sig.parameters) == ['self', 'extrinsics', 'R', 'cap', 'params', 'device']
    assert (sig.parameters['R'].default, sig.parameters['cap'].default, sig.parameters['params'].default, sig.parameters['device'].default) == (1, None, None, 'cuda')
