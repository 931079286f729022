"""GPU: the record tail - rtm3d_pack_records, rtm3d_project_boxes (csrc/decode3d.hip), rtm3d_frames_adjust_k,
rtm3d_records_to_camera (csrc/frames.hip) and the shared csrc/box_project.h - against the fp64 yardstick of
tests/record_tail_ref.py over the cases of tests/record_tail_regimes.py.  tests/test_record_tail_regimes.py asserts on the CPU
that every case is in the regime it is named for and that the yardstick agrees with the project's host forms and with the
vectors of the reference run.

Bars: records (rtm3d_pack_records, and [2:24] after rtm3d_records_to_camera) and K_net bit-equal - the header defines the
operation order, and every Ry of the tables is clear of an fp32 rounding midpoint; projections, rectangles and row entries [1],
[2:6], [12] within 1e-9 |want| + 1e-7, the bar of test_project_boxes_device_vs_reference_vectors (the device's sin / cos / atan2
are not the host's), with the finite / infinite / NaN pattern equal; every other row entry bit-equal; rows of not-kept slots all
zero.  Each test prints its largest disagreement.

Measured on an MI355X (the figures the tests print; copied to profiles/record_tail.txt): rtm3d_project_boxes at most 2.27e-13 from the
yardstick (9.9e-7 of the bar), the toleranced row entries at most 1.71e-13 (the pool case, 9.9e-7 of the bar; 1.14e-13 over the 260
rows of b65k8); everything under a bit-equal bar is bit-equal.  With the kernels as they were before this suite eight tests fail:
the kept_rule case and the NMS-order test (a slot with flag 1 got a row), the refusal at frame 67 (frames 0..63 had been rewritten),
and five project_boxes cases (the rectangle was reduced from +-1e300 sentinels, which hid infinite and NaN corners)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, box_overlap, kitti_eval, preprocess        # noqa: E402
from rtm3d_amd import distributed as rdist                             # noqa: E402
from rtm3d_amd import kitti_results as kr                              # noqa: E402
from rtm3d_amd.model_utils import Boxes3D, FUN_ACCEPT                  # noqa: E402
from tests import box_overlap_ref                                      # noqa: E402
from tests import record_tail_ref as ref                               # noqa: E402
from tests import record_tail_regimes as rg                            # noqa: E402
from tests.util import record_measurement                              # noqa: E402

RTOL, ATOL = 1e-9, 1e-7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def to_dev(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)                        # a copy: the cases are read-only


def geom_array(geoms):
    return (_lib.FrameGeom * len(geoms))(*[_lib.FrameGeom(*g) for g in geoms])


def solver_outputs(dev, x, fun, status):
    bx = Boxes3D(len(x), dev)
    bx.x.copy_(to_dev(dev, x)); bx.fun.copy_(to_dev(dev, fun)); bx.status.copy_(to_dev(dev, status))
    return bx


def pattern(a):
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 2, np.where(np.isinf(a), np.sign(a) * 3, 0)).astype(np.int8)


def within_bar(got, want, what):
    """Pattern equal, finite values within RTOL |want| + ATOL; returns (largest absolute difference, largest in units of the bar)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(pattern(got), pattern(want)), (what, np.argwhere(pattern(got) != pattern(want))[:6].tolist())
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0, 0.0
    d = np.abs(got[fin] - want[fin])
    units = d / (RTOL * np.abs(want[fin]) + ATOL)
    assert units.max() <= 1.0, (what, float(d.max()), float(units.max()))
    return float(d.max()), float(units.max())


def stream(dev):
    return _lib.stream_ptr(dev)


# ------------------------------------------------------------------------------------------------ 1. pack_records
def device_pack(dev, c, solved):
    t = {k: to_dev(dev, c[k]) for k in ('n', 'cls', 'score', 'mproj', 'verts', 'bbox', 'x', 'fun', 'status')}
    rec = torch.full((c['B'], c['topk'], 32), -7.0, dtype=torch.float32, device=dev)
    s = [t[k].data_ptr() if solved else None for k in ('x', 'fun', 'status')]
    _lib.check(_lib.load().rtm3d_pack_records(stream(dev), c['B'], c['topk'], t['n'].data_ptr(), t['cls'].data_ptr(), t['score'].data_ptr(),
                                              t['mproj'].data_ptr(), t['verts'].data_ptr(), t['bbox'].data_ptr(), *s, float(c['fun_accept']),
                                              rec.data_ptr()), 'pack_records')
    torch.cuda.synchronize()
    return rec.cpu().numpy(), t


@pytest.mark.parametrize('name', rg.PACK_ALL)
def test_pack_records_equals_the_yardstick_bit_for_bit(dev, name):
    c = rg.pack_case(name)
    kept = 0
    for solved in (True, False):
        s = (c['x'], c['fun'], c['status']) if solved else (None, None, None)
        want = ref.pack_records(c['n'], c['cls'], c['score'], c['mproj'], c['verts'], c['bbox'], c['topk'], *s, fun_accept=c['fun_accept'])
        got, t = device_pack(dev, c, solved)
        diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(diff) == 0, (name, solved, len(diff), diff[:8].tolist())
        kept += int((want[..., 31] == 2).sum())
        if c['fun_accept'] == FUN_ACCEPT:                                 # and through the Python wrapper
            bx = solver_outputs(dev, c['x'], c['fun'], c['status']) if solved else None
            via = rdist.pack_records(t['n'], t['cls'], t['score'], t['mproj'], t['verts'], t['bbox'], c['topk'], bx)
            assert bits(via.cpu().numpy()) == bits(want)
    print('pack_records %s: %d slots, %d kept, bit-equal with and without the solver outputs' % (name, c['B'] * c['topk'], kept))


# ------------------------------------------------------------------------------------------------ 2. project_boxes
@pytest.mark.parametrize('name', rg.PROJECT_NAMES)
def test_project_boxes_equals_the_yardstick(dev, name):
    c = rg.project_case(name)
    want_proj, want_rect = ref.project_boxes(c['x'], c['status'], c['K'], c['topk'])
    bx = solver_outputs(dev, c['x'], np.zeros(c['N']), c['status'])
    proj, rect = kr.project_boxes_device(bx, to_dev(dev, c['K']), topk=c['topk'])
    proj, rect = proj.cpu().numpy(), rect.cpu().numpy()
    dead = c['status'] < 0
    assert not proj[dead].any() and not rect[dead].any()
    worst = max(within_bar(proj, want_proj, name + ' proj'), within_bar(rect, want_rect, name + ' rect'))
    print('project_boxes %s: N %d, largest disagreement %.3g (%.3g of the bar %g |want| + %g)' % (name, c['N'], worst[0], worst[1], RTOL, ATOL))
    record_measurement('record_tail', 'project_boxes ' + name, {'abs': worst[0], 'of_bar': worst[1]})


# ------------------------------------------------------------------------------------------------ 3. frames_adjust_K
@pytest.mark.parametrize('B', rg.ADJUST_B)
def test_frames_adjust_K_equals_the_yardstick_bit_for_bit(dev, B):
    c = rg.adjust_case(B)
    want = np.array([ref.k_net(c['K'][b], g) for b, g in enumerate(c['geoms'])])
    got = preprocess.adjust_K_device(to_dev(dev, c['K']), geom_array(c['geoms'])).cpu().numpy()
    assert got.shape == (B, 9) and bits(got) == bits(want), np.argwhere(got != want)[:8].tolist()


# ------------------------------------------------------------------------------------------------ 4. records_to_camera
def device_camera(dev, c, rec=None):
    """(records, rows, records of the run without rows) of rtm3d_records_to_camera on the case's canvas records."""
    rec = c['rec'] if rec is None else rec
    geom = geom_array(c['geoms'])
    bx = solver_outputs(dev, c['x'], c['fun'], c['status'])
    assert c['fun_accept'] == FUN_ACCEPT
    got, rows = preprocess.records_to_camera(to_dev(dev, rec), geom, K_camera=to_dev(dev, c['K']), boxes=bx, kitti=True)
    plain = preprocess.records_to_camera(to_dev(dev, rec), geom)
    torch.cuda.synchronize()
    return got.cpu().numpy(), rows.cpu().numpy(), plain.cpu().numpy()


def check_camera(c, rec, got, rows, what):
    """The bars of the module docstring for one run; returns the largest disagreement of the toleranced row entries."""
    want = ref.to_camera(rec, c['geoms'])
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(diff) == 0, (what, len(diff), diff[:8].tolist())           # [2:24] of live slots moved, everything else stayed
    want_rows = ref.kitti_rows(rec, c['x'], c['fun'], c['status'], c['K'], c['geoms'], c['fun_accept'])
    keptm = want_rows[..., 14] == 2
    assert np.array_equal(rows[..., 14] == 2, keptm), (what, np.argwhere((rows[..., 14] == 2) != keptm)[:8].tolist())
    assert not rows[~keptm].any()
    exact = [0, 6, 7, 8, 9, 10, 11, 13, 14, 15]
    assert bits(rows[keptm][:, exact]) == bits(want_rows[keptm][:, exact]), what
    return within_bar(rows[keptm][:, [1, 2, 3, 4, 5, 12]], want_rows[keptm][:, [1, 2, 3, 4, 5, 12]], what)


@pytest.mark.parametrize('name', rg.CAMERA_NAMES)
def test_records_to_camera_equals_the_yardstick(dev, name):
    c = rg.camera_case(name)
    got, rows, plain = device_camera(dev, c)
    assert bits(got) == bits(plain)                                       # with and without d_kitti: the same records
    worst = check_camera(c, c['rec'], got, rows, name)
    if name == 'kept_rule':
        assert np.array_equal(rows[..., 14] == 2, c['want_row'])
        empty = c['rec'][..., 31] == 0
        assert bits(got[empty]) == bits(c['rec'][empty])                  # garbage in a flag-0 slot is not touched
    if name == 'alpha':
        n = len(c['want_alpha'])
        assert rows[0, n:, 1].tolist() == [-math.pi, -math.pi] and rows[0, n:, 12].tolist() == [math.pi, -math.pi]
    print('records_to_camera %s: %d x %d slots, %d rows, largest disagreement of alpha / rectangle / ry %.3g (%.3g of the bar %g |want| + %g)'
          % (name, c['B'], c['topk'], int((rows[..., 14] == 2).sum()), worst[0], worst[1], RTOL, ATOL))
    record_measurement('record_tail', 'records_to_camera ' + name, {'abs': worst[0], 'of_bar': worst[1]})


# ------------------------------------------------------------------------------------------------ 5. NMS before or after the rows
def test_nms_before_or_after_the_rows_gives_the_same_records_and_rows(dev):
    """rtm3d_records_nms3d may run before or after rtm3d_records_to_camera: a slot it suppressed (flag 2 -> 1, solver outputs
    untouched) has no KITTI row either way."""
    c = rg.nms_order_case()
    geom = geom_array(c['geoms'])
    bx = solver_outputs(dev, c['x'], c['fun'], c['status'])
    K = to_dev(dev, c['K'])
    a = box_overlap.nms3d_records(to_dev(dev, c['rec']), rg.NMS_THRESH)
    a, rows_a = preprocess.records_to_camera(a, geom, K_camera=K, boxes=bx, kitti=True)
    b, rows_b = preprocess.records_to_camera(to_dev(dev, c['rec']), geom, K_camera=K, boxes=bx, kitti=True)
    box_overlap.nms3d_records(b, rg.NMS_THRESH, kitti_rows=rows_b)
    torch.cuda.synchronize()
    a, rows_a, b, rows_b = (t.cpu().numpy() for t in (a, rows_a, b, rows_b))
    after = c['rec'].copy()
    for m in range(c['B']):
        after[m, :, 31] = box_overlap_ref.nms_flags(c['rec'][m], rg.NMS_THRESH, box_overlap_ref.record_ious(c['rec'][m])[0])
    assert int(((c['rec'][..., 31] == 2) & (after[..., 31] == 1)).sum()) >= 1
    assert bits(a[..., 31]) == bits(after[..., 31]) == bits(b[..., 31])
    assert np.array_equal(rows_a[..., 14] == 2, after[..., 31] == 2), 'a slot suppressed before the rows were made has a row'
    assert bits(a) == bits(b) and bits(rows_a) == bits(rows_b)
    check_camera(c, after, a, rows_a, 'nms, then rows')
    la, lb = kitti_eval.from_rows(rows_a), kitti_eval.from_rows(rows_b)
    assert la.n.tolist() == lb.n.tolist() == (after[..., 31] == 2).sum(1).tolist()
    for f in kitti_eval.Labels.FIELDS:
        assert bits(getattr(la, f)) == bits(getattr(lb, f)), f


# ------------------------------------------------------------------------------------------------ 6. refusals
def guarded(dev, n, dtype, seed):
    """A device buffer of n + 2 x 64 elements with random content (the outer 64 on either side are guards), its host copy."""
    g = np.random.Generator(np.random.PCG64(seed))
    host = g.uniform(1, 100, n + 128).astype(dtype)
    return torch.from_numpy(host.copy()).to(dev), host


def test_entries_refuse_bad_arguments(dev):
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    p = buf.data_ptr()
    geom = geom_array(rg.geoms_for(2))
    st = stream(dev)

    def refused(rc, text):
        assert rc != 0 and text in lib.rtm3d_last_error().decode(), lib.rtm3d_last_error().decode()
    refused(lib.rtm3d_records_to_camera(st, 0, 2, geom, p, None, None, None, None, 0.1, None), 'records_to_camera: bad arguments')
    refused(lib.rtm3d_records_to_camera(st, -1, 2, geom, p, None, None, None, None, 0.1, None), 'records_to_camera: bad arguments')
    refused(lib.rtm3d_records_to_camera(st, 2, 0, geom, p, None, None, None, None, 0.1, None), 'records_to_camera: bad arguments')
    refused(lib.rtm3d_records_to_camera(st, 2, 2, geom, None, None, None, None, None, 0.1, None), 'records_to_camera: bad arguments')
    refused(lib.rtm3d_records_to_camera(st, 2, 2, None, p, None, None, None, None, 0.1, None), 'records_to_camera: bad arguments')
    for missing in range(4):
        four = [None if k == missing else p for k in range(4)]
        refused(lib.rtm3d_records_to_camera(st, 2, 2, geom, p, *four, 0.1, p), 'the KITTI rows need')
    refused(lib.rtm3d_frames_adjust_k(st, 0, geom, p, p), 'frames_adjust_K: bad arguments')
    refused(lib.rtm3d_frames_adjust_k(st, 2, None, p, p), 'frames_adjust_K: bad arguments')
    refused(lib.rtm3d_frames_adjust_k(st, 2, geom, None, p), 'frames_adjust_K: bad arguments')
    refused(lib.rtm3d_frames_adjust_k(st, 2, geom, p, None), 'frames_adjust_K: bad arguments')
    refused(lib.rtm3d_pack_records(st, 0, 2, p, p, p, p, p, p, None, None, None, 0.1, p), 'pack_records: bad sizes')
    refused(lib.rtm3d_pack_records(st, 2, 0, p, p, p, p, p, p, None, None, None, 0.1, p), 'pack_records: bad sizes')
    refused(lib.rtm3d_pack_records(st, 2, 2, p, p, p, p, p, p, p, None, p, 0.1, p), 'pack_records: null pointer')
    refused(lib.rtm3d_pack_records(st, 2, 2, p, p, p, p, p, p, None, None, None, 0.1, None), 'pack_records: null pointer')
    refused(lib.rtm3d_project_boxes(st, 0, 0, p, p, p, p, p), 'project_boxes: bad sizes')
    refused(lib.rtm3d_project_boxes(st, 2, -1, p, p, p, p, p), 'project_boxes: bad sizes')
    refused(lib.rtm3d_project_boxes(st, 2, 0, p, p, None, p, p), 'project_boxes: null pointer')
    torch.cuda.synchronize()
    assert not buf.any()                                                   # nothing was launched on the way


@pytest.mark.parametrize('bad', [3, 67])
def test_a_bad_geometry_is_refused_before_any_frame_is_converted(dev, bad):
    """70 frames are two launch chunks (64 + 6).  A geometry with rh = 0 at frame 3 or at frame 67 is refused by name, and not
    one byte of the records, the rows or K_net has changed - the frames of the chunk before the bad one included."""
    lib = _lib.load()
    B, topk = 70, 2
    geoms = rg.geoms_for(B)
    g = geoms[bad]
    geoms[bad] = (g[0], g[1], 0, g[3], g[4], g[5])
    geom = geom_array(geoms)
    r = rg.rng(600 + bad)
    x = rg.random_boxes(r, B * topk)
    bx = solver_outputs(dev, x, np.full(B * topk, 0.01), np.zeros(B * topk, np.int32))
    rec, rec0 = guarded(dev, B * topk * 32, np.float32, 1)
    rec[64:-64].view(B, topk, 32)[..., 31] = 2.0
    rec0[64:-64].reshape(B, topk, 32)[..., 31] = 2.0
    rows, rows0 = guarded(dev, B * topk * 16, np.float64, 2)
    K, _ = guarded(dev, B * 9, np.float64, 3)
    K_net, K_net0 = guarded(dev, B * 9, np.float64, 4)
    st = stream(dev)

    def inner(t):
        return t.data_ptr() + 64 * t.element_size()
    for with_rows in (True, False):
        four = [inner(K), bx.x.data_ptr(), bx.fun.data_ptr(), bx.status.data_ptr()] if with_rows else [None] * 4
        assert lib.rtm3d_records_to_camera(st, B, topk, geom, inner(rec), *four, 0.1, inner(rows) if with_rows else None) != 0
        msg = lib.rtm3d_last_error().decode()
        assert msg.startswith('records_to_camera: frame %d has an empty size' % bad), msg
        torch.cuda.synchronize()
        assert bits(rec.cpu().numpy()) == bits(rec0), 'records were rewritten before the refusal'
        assert bits(rows.cpu().numpy()) == bits(rows0), 'rows were written before the refusal'
    assert lib.rtm3d_frames_adjust_k(st, B, geom, inner(K), inner(K_net)) != 0
    msg = lib.rtm3d_last_error().decode()
    assert msg.startswith('frames_adjust_K: frame %d has an empty size' % bad), msg
    torch.cuda.synchronize()
    assert bits(K_net.cpu().numpy()) == bits(K_net0), 'K_net was written before the refusal'
    # the wrappers raise with the same message
    with pytest.raises(RuntimeError, match='frame %d has an empty size' % bad):
        preprocess.records_to_camera(rec[64:-64].view(B, topk, 32), geom)
    with pytest.raises(RuntimeError, match='frame %d has an empty size' % bad):
        preprocess.adjust_K_device(K[64:-64].view(B, 9), geom)
    torch.cuda.synchronize()
    assert bits(rec.cpu().numpy()) == bits(rec0)
    # and the same batch with the geometry mended goes through
    geoms[bad] = g
    assert lib.rtm3d_records_to_camera(st, B, topk, geom_array(geoms), inner(rec), None, None, None, None, 0.1, None) == 0
    torch.cuda.synchronize()
    after = rec.cpu().numpy()
    assert bits(after[:64]) == bits(rec0[:64]) and bits(after[-64:]) == bits(rec0[-64:])            # the guards
    assert bits(after[64:-64].reshape(B, topk, 32)) == bits(ref.to_camera(rec0[64:-64].reshape(B, topk, 32), geoms))


def test_python_wrappers_refuse_wrong_tensors(dev):
    c = rg.camera_case('b1k3')
    geom = geom_array(c['geoms'])
    rec = to_dev(dev, c['rec'])
    bx = solver_outputs(dev, c['x'], c['fun'], c['status'])
    K = to_dev(dev, c['K'])
    for wrong in (rec.cpu(), rec.double(), rec[0], rec[:, :, :31], torch.cat([rec, rec]), rec.transpose(1, 2).contiguous().transpose(1, 2)):
        with pytest.raises(ValueError):
            preprocess.records_to_camera(wrong, geom)
    with pytest.raises(ValueError):
        preprocess.records_to_camera(rec, geom, kitti=True)
    with pytest.raises(ValueError):
        preprocess.records_to_camera(rec, geom, K_camera=K, kitti=True)
    with pytest.raises(ValueError):
        preprocess.records_to_camera(rec, geom, K_camera=K, boxes=solver_outputs(dev, c['x'][:2], c['fun'][:2], c['status'][:2]), kitti=True)
    for wrong in (K.cpu(), K.float(), torch.cat([K, K])):
        with pytest.raises(ValueError):
            preprocess.adjust_K_device(wrong, geom)
    with pytest.raises(ValueError):
        preprocess.adjust_K_device(K, geom, out=torch.empty(2, 9, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        kr.project_boxes_device(bx, K, topk=2)
    with pytest.raises(ValueError):
        rdist.pack_records(torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev), None, None, None, None, 3)
    torch.cuda.synchronize()
    assert bits(rec.cpu().numpy()) == bits(c['rec'])                       # no refusal touched the records
