"""CPU: the yardstick of the box-overlap tests (tests/box_overlap_ref.py) against closed forms, the conditions the shared test
inputs must meet (tests/box_overlap_cases.py), and what the new surface promises without a device: the refusals of the two
C entry points, the refusal of CPU tensors, the `nms3d` keyword of Detect3DPipeline / Engine."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from rtm3d_amd import _lib, box_overlap, engine
from rtm3d_amd.pipeline import Detect3DPipeline
from tests import box_overlap_ref as ref
from tests import box_overlap_cases as cases


def _interval(lo_a, hi_a, lo_b, hi_b):
    return max(0.0, min(hi_a, hi_b) - max(lo_a, lo_b))


def test_yardstick_equals_interval_products_on_axis_aligned_boxes():
    rng = np.random.Generator(np.random.PCG64(3))
    yaws = (0.0, np.pi / 2, -np.pi / 2, np.pi)
    worst, hits = 0.0, 0
    for _ in range(300):
        a = np.concatenate([rng.uniform(0.3, 6.0, 3), rng.uniform(-3.0, 3.0, 3), [yaws[rng.integers(4)]]])
        b = np.concatenate([rng.uniform(0.3, 6.0, 3), rng.uniform(-3.0, 3.0, 3), [yaws[rng.integers(4)]]])

        def extent(box):                         # (x extent, z extent): l along x at ry = 0 / pi, along z at +- pi / 2
            turned = abs(abs(box[6]) - np.pi / 2) < 1e-9
            return (box[1], box[2]) if turned else (box[2], box[1])
        (ax, az), (bx, bz) = extent(a), extent(b)
        inter = _interval(a[3] - ax / 2, a[3] + ax / 2, b[3] - bx / 2, b[3] + bx / 2) * \
            _interval(a[5] - az / 2, a[5] + az / 2, b[5] - bz / 2, b[5] + bz / 2)
        ov = _interval(a[4] - a[0] / 2, a[4] + a[0] / 2, b[4] - b[0] / 2, b[4] + b[0] / 2)
        sa, sb = a[1] * a[2], b[1] * b[2]
        want = {'iou': (inter / (sa + sb - inter), inter * ov / (sa * a[0] + sb * b[0] - inter * ov)),
                'a': (inter / sa, inter * ov / (sa * a[0])), 'b': (inter / sb, inter * ov / (sb * b[0]))}
        hits += inter > 0
        for crit in ref.CRITERIA:
            got = ref.overlap(a, b, crit)
            worst = max(worst, abs(got[0] - want[crit][0]), abs(got[1] - want[crit][1]))
    assert hits >= 100, hits
    assert worst <= 1e-12, worst


def test_yardstick_on_the_degenerate_cases_and_invalid_boxes():
    for name, a, b, bev, vol in cases.degenerate_cases():
        got = ref.overlap(a, b)
        assert abs(got[0] - bev) <= 1e-12 and abs(got[1] - vol) <= 1e-12, (name, got, bev, vol)
        back = ref.overlap(b, a)
        assert abs(back[0] - bev) <= 1e-12 and abs(back[1] - vol) <= 1e-12, (name, back)
    ok, bad = cases.invalid_boxes()
    for b in bad:
        for crit in ref.CRITERIA:
            assert ref.overlap(ok, b, crit) == (0.0, 0.0) and ref.overlap(b, ok, crit) == (0.0, 0.0) and ref.overlap(b, b, crit) == (0.0, 0.0)


def test_yardstick_greedy_nms_on_a_chain():
    """Three boxes in a row, each overlapping the next above the threshold and the one after below it: the middle one goes,
    the third stays (suppression is by SURVIVORS only); at an IoU equal to the threshold nothing goes (strictly greater)."""
    rec = np.zeros((5, 32), np.float32)
    for k, x in enumerate((0.0, 1.0, 2.0)):
        rec[k + 1, 24:31] = (1.5, 2.0, 4.0, x, 1.0, 10.0, 0.0)
        rec[k + 1, 31] = 2
    rec[4, 24:31], rec[4, 31] = rec[1, 24:31], 1                      # a flag-1 copy of the first box: no candidate
    bev, vol = ref.record_ious(rec)
    assert abs(bev[1, 2] - 3.0 / 5.0) <= 1e-12 and abs(bev[1, 3] - 2.0 / 6.0) <= 1e-12 and bev[4].max() == 0
    assert ref.nms_flags(rec, 0.5, bev).tolist() == [0, 2, 1, 2, 1]
    assert ref.nms_flags(rec, float(bev[1, 2]), bev).tolist() == [0, 2, 2, 2, 1]
    rec[2, 0] = rec[3, 0] = 1                                         # the second and third share a class the first has not
    assert ref.nms_flags(rec, 0.5, bev, class_aware=True).tolist() == [0, 2, 2, 1, 1]


def test_shared_inputs_meet_their_conditions():
    A, Bx, na, nb = cases.random_pairs()
    assert A.shape == (3, 17, 7) and na.tolist() == [17, 0, 5] and nb.tolist() == [17, 4, 0]
    assert np.abs(A[..., 3:6]).max() <= 40 and np.abs(Bx[..., 3:6]).max() <= 40
    assert A[..., :3].min() >= 0.3 and A[..., :3].max() <= 12 and np.abs(Bx[..., 6]).max() <= 4 * np.pi
    assert min(ref.min_edge_angle(a, b) for m in range(3) for a in A[m] for b in Bx[m]) >= cases.MIN_EDGE_ANGLE
    bev, _ = ref.overlaps(A[:1], Bx[:1])
    assert (bev > 0.01).sum() >= 10, (bev > 0).sum()                  # the set does exercise the clipping
    for topk in cases.NMS_SHAPES:
        rec = cases.nms_records(topk)
        assert rec.shape == (2, topk, 32)
        flags = rec[..., 31]
        assert all((flags == f).any() for f in (0, 1, 2))
        assert ((flags[1] == 2).sum() == 0) == (topk < 64)
        went = 0
        for b in range(2):
            ious = dict(zip(('bev', '3d'), ref.record_ious(rec[b])))
            for metric, thr in cases.NMS_THRESH.items():
                m = ious[metric][np.triu_indices(topk, 1)]
                assert np.abs(m[m > 0] - thr).min(initial=1.0) > cases.IOU_GAP, (topk, b, metric)
                agnostic = ref.nms_flags(rec[b], thr, ious[metric])
                aware = ref.nms_flags(rec[b], thr, ious[metric], class_aware=True)
                went += (agnostic != flags[b]).sum()
                if (flags[b] == 2).any():
                    i, j = topk // 3, topk // 3 + 2                   # the two classes at one place
                    assert (agnostic[i], agnostic[j], aware[i], aware[j]) == (2, 1, 2, 2)
        assert went >= 2, (topk, went)


# ------------------------------------------------------------------------------------------------ the surface, no device
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _err(lib):
    return lib.rtm3d_last_error().decode()


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below is refused on the host
    ov, nms = lib.rtm3d_box_overlaps, lib.rtm3d_records_nms3d
    for B, ca, cb in ((0, 1, 1), (1, 0, 1), (1, 1, -2)):
        assert ov(None, B, ca, cb, p, p, p, p, 0, p, p) != 0 and 'bad sizes' in _err(lib)
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert ov(None, 1, 2, 2, *args, 0, p, p) != 0 and 'null pointer' in _err(lib)
    assert ov(None, 1, 2, 2, p, p, p, p, 0, None, None) != 0 and 'both outputs' in _err(lib)
    for crit in (-1, 3):
        assert ov(None, 1, 2, 2, p, p, p, p, crit, p, p) != 0 and 'unknown criterion %d' % crit in _err(lib)
    assert nms(None, 2, 300, p, 0.5, 0, 0, None) != 0 and 'topk 300' in _err(lib) and '256' in _err(lib)
    assert nms(None, 0, 100, p, 0.5, 0, 0, None) != 0 and 'bad sizes' in _err(lib)
    assert nms(None, 2, 100, None, 0.5, 0, 0, None) != 0 and 'null pointer' in _err(lib)
    assert nms(None, 2, 100, p, 0.5, 2, 0, None) != 0 and 'unknown metric 2' in _err(lib)
    assert nms(None, 2, 100, p, float('nan'), 0, 0, None) != 0 and 'NaN' in _err(lib)
    assert lib.rtm3d_abi_version() == 9


def test_cpu_tensors_are_refused():
    a = torch.zeros(2, 3, 7, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        box_overlap.overlaps(a, a)
    with pytest.raises(RuntimeError, match='no CPU path'):
        box_overlap.nms3d_records(torch.zeros(2, 100, 32), 0.5)
    with pytest.raises(ValueError, match='criterion'):
        box_overlap.overlaps(a, a, criterion='union')
    with pytest.raises(ValueError, match='metric'):
        box_overlap.nms3d_records(torch.zeros(2, 100, 32), 0.5, metric='2d')


def test_nms3d_keyword_of_pipeline_and_engine():
    for fn in (Detect3DPipeline.__init__, engine.Engine.detect, engine.Engine.detect_frames):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == 'nms3d' and params['nms3d'].default is None, fn
    opts = box_overlap.nms3d_options
    assert opts(None) is None
    assert opts(0.5) == {'iou_thresh': 0.5}
    assert opts({'iou_thresh': 0.25, 'metric': '3d', 'class_aware': True}) == {'iou_thresh': 0.25, 'metric': '3d', 'class_aware': True}
    for bad in ({'metric': 'bev'}, {'iou_thresh': 0.5, 'metric': 'area'}, {'iou_thresh': 0.5, 'topk': 3}):
        with pytest.raises(ValueError, match='nms3d'):
            opts(bad)
