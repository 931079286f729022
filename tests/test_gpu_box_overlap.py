"""GPU: rtm3d_box_overlaps and rtm3d_records_nms3d (csrc/box_overlap.hip) against the fp64 numpy yardstick of
tests/box_overlap_ref.py (itself checked against closed forms in tests/test_box_overlap_cpu.py), and the `nms3d` keyword of
Detect3DPipeline / Engine.detect.

Measured on the MI355X (random ragged set, all three criteria, BEV and 3D): largest disagreement with the yardstick 6.7e-15,
largest asymmetry iou(a, b) - iou(b, a) 1.1e-16; bars 1e-9 and 1e-12."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                     # noqa: E402
from rtm3d_amd import _lib, weights, engine, box_overlap  # noqa: E402
from rtm3d_amd.pipeline import Detect3DPipeline      # noqa: E402
from tests import box_overlap_ref as ref             # noqa: E402
from tests import box_overlap_cases as cases         # noqa: E402
from tests.util import load_golden                   # noqa: E402

ABS_TOL = 1e-9          # both sides fp64; a clipped vertex divides by the sine of the angle between two edges (>= 1e-3 rad)
EXACT_TOL = 1e-12       # closed forms, symmetry


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------ 1. overlap matrices
@pytest.fixture(scope='module')
def ragged():
    A, Bx, na, nb = cases.random_pairs()
    return A, Bx, na, nb, {c: ref.overlaps(A, Bx, na, nb, c) for c in ref.CRITERIA}


def test_overlaps_equal_the_yardstick_on_a_ragged_set(dev, ragged):
    A, Bx, na, nb, want = ragged
    assert min(ref.min_edge_angle(a, b) for m in range(3) for a in A[m] for b in Bx[m]) >= cases.MIN_EDGE_ANGLE
    tA, tB = torch.from_numpy(A).to(dev), torch.from_numpy(Bx).to(dev)
    tna, tnb = torch.from_numpy(na).to(dev), torch.from_numpy(nb).to(dev)
    worst = 0.0
    for crit in ref.CRITERIA:
        bev, vol = box_overlap.overlaps(tA, tB, tna, tnb, criterion=crit)
        bev, vol = bev.cpu().numpy(), vol.cpu().numpy()
        assert bev.shape == (3, 17, 17) and np.isfinite(bev).all() and np.isfinite(vol).all()
        for got, exp in ((bev, want[crit][0]), (vol, want[crit][1])):
            worst = max(worst, float(np.abs(got - exp).max()))
            for m in range(3):                                   # beyond the counts: exactly 0
                assert not got[m, na[m]:].any() and not got[m, :, nb[m]:].any()
        assert (bev[0] > 0).sum() >= 10 and (vol[0] > 0).sum() >= 3
    print('box overlaps: largest disagreement with the yardstick %.3g (bar %g)' % (worst, ABS_TOL))
    assert worst <= ABS_TOL, worst
    # symmetry, and the (N, 7) form with every entry counted
    ab = box_overlap.overlaps(tA[0], tB[0])
    ba = box_overlap.overlaps(tB[0], tA[0])
    assert ab[0].shape == (17, 17)
    asym = max(float((ab[k] - ba[k].T).abs().max()) for k in (0, 1))
    print('box overlaps: largest asymmetry %.3g (bar %g)' % (asym, EXACT_TOL))
    assert asym <= EXACT_TOL, asym
    assert np.abs(ab[0].cpu().numpy() - want['iou'][0][0]).max() <= ABS_TOL
    # 'a' and 'b' are each other's transpose
    over_a = box_overlap.overlaps(tA[:1], tB[:1], criterion='a')
    over_b = box_overlap.overlaps(tB[:1], tA[:1], criterion='b')
    assert max(float((over_a[k] - over_b[k].transpose(1, 2)).abs().max()) for k in (0, 1)) <= EXACT_TOL


def test_overlaps_of_degenerate_and_invalid_boxes(dev):
    cs = cases.degenerate_cases()
    a = torch.from_numpy(np.stack([c[1] for c in cs])).to(dev).unsqueeze(1)          # one pair per "image"
    b = torch.from_numpy(np.stack([c[2] for c in cs])).to(dev).unsqueeze(1)
    for x, y in ((a, b), (b, a)):
        bev, vol = box_overlap.overlaps(x, y)
        bev, vol = bev.cpu().numpy().reshape(-1), vol.cpu().numpy().reshape(-1)
        for k, (name, _, _, e_bev, e_vol) in enumerate(cs):
            assert abs(bev[k] - e_bev) <= EXACT_TOL and abs(vol[k] - e_vol) <= EXACT_TOL, (name, bev[k], vol[k])
    ok, bad = cases.invalid_boxes()
    boxes = torch.from_numpy(np.concatenate([ok[None], bad, ok[None]])).to(dev)
    for crit in ref.CRITERIA:
        bev, vol = (t.cpu().numpy() for t in box_overlap.overlaps(boxes, boxes, criterion=crit))
        assert np.isfinite(bev).all() and np.isfinite(vol).all()
        n = len(bad)
        for m in (bev, vol):
            assert not m[1:1 + n].any() and not m[:, 1:1 + n].any()
            assert np.abs(m[[0, 0, -1, -1], [0, -1, 0, -1]] - 1.0).max() <= EXACT_TOL
    with pytest.raises(RuntimeError, match='both outputs'):
        _lib.check(_lib.load().rtm3d_box_overlaps(None, 1, 1, 1, boxes.data_ptr(), boxes.data_ptr(), boxes.data_ptr(), boxes.data_ptr(),
                                                  0, None, None), 'box_overlaps')


# ------------------------------------------------------------------------------------------------ 2. NMS on records
@pytest.fixture(scope='module')
def nms_inputs():
    out = {}
    for topk in cases.NMS_SHAPES:
        rec = cases.nms_records(topk)
        ious = [dict(zip(('bev', '3d'), ref.record_ious(rec[b]))) for b in range(rec.shape[0])]
        out[topk] = (rec, ious)
    return out


@pytest.mark.parametrize('topk', cases.NMS_SHAPES)
def test_nms3d_records_equal_the_yardstick(dev, nms_inputs, topk):
    rec, ious = nms_inputs[topk]
    B = rec.shape[0]
    rows0 = np.random.Generator(np.random.PCG64(topk)).standard_normal((B, topk, 16))
    total = 0
    for metric, thr in cases.NMS_THRESH.items():
        for b in range(B):
            m = ious[b][metric][np.triu_indices(topk, 1)]
            assert np.abs(m[m > 0] - thr).min(initial=1.0) > cases.IOU_GAP          # no decision hinges on round-off
        for aware in (False, True):
            want = np.stack([ref.nms_flags(rec[b], thr, ious[b][metric], class_aware=aware) for b in range(B)])
            t, rows = torch.from_numpy(rec).to(dev), torch.from_numpy(rows0).to(dev)
            ret = box_overlap.nms3d_records(t, thr, metric=metric, class_aware=aware, kitti_rows=rows)
            assert ret is t
            got, got_rows = t.cpu().numpy(), rows.cpu().numpy()
            assert np.array_equal(got[..., 31], want), (topk, metric, aware, np.argwhere(got[..., 31] != want)[:5])
            went = (rec[..., 31] == 2) & (want == 1)
            total += int(went.sum())
            expect = rec.copy()
            expect[..., 31] = want
            assert got.tobytes() == expect.tobytes()                                # every other byte is unchanged
            expect_rows = rows0.copy()
            expect_rows[went] = 0.0
            assert got_rows.tobytes() == expect_rows.tobytes()
            box_overlap.nms3d_records(t, thr, metric=metric, class_aware=aware, kitti_rows=rows)     # a second call changes nothing
            assert t.cpu().numpy().tobytes() == expect.tobytes() and rows.cpu().numpy().tobytes() == expect_rows.tobytes()
            # without the rows, and as one flat list of images
            t2 = torch.from_numpy(rec).to(dev).reshape(B * topk, 32).reshape(B, 1, topk, 32)
            assert np.array_equal(box_overlap.nms3d_records(t2, thr, metric=metric, class_aware=aware).cpu().numpy()[:, 0, :, 31], want)
    assert total >= 4, total


def test_nms3d_refuses_more_than_256_slots(dev):
    t = torch.zeros(2, 300, 32, device=dev)
    t[..., 31] = 2
    with pytest.raises(RuntimeError, match='topk 300 is more than the 256'):
        box_overlap.nms3d_records(t, 0.5)
    torch.cuda.synchronize()
    assert bool((t[..., 31] == 2).all())


# ------------------------------------------------------------------------------------------------ 3. pipeline and engine
def twin(dev, tmp_path, monkeypatch):
    """The model of e2e_dla34_small.npz with its heat-map plane of class 0 copied onto class 1 and one reference dimension for
    both: every peak of the one plane fires on the other, and the solver gives both the same 3D box.  The regression weights
    are random, so the solver's residual keeps none of these boxes at the product's bar (0 of 45 live slots measured): the bar
    is raised for this model (pack_records reads model_utils.FUN_ACCEPT, save_engine writes engine.FUN_ACCEPT into the file),
    which turns every solved slot into a kept one (45 measured) and the twins whose solved box is a valid one (2 pairs measured)
    into 3D duplicates."""
    from rtm3d_amd import model_utils
    monkeypatch.setattr(model_utils, 'FUN_ACCEPT', 1e6)
    monkeypatch.setattr(engine, 'FUN_ACCEPT', 1e6)
    g = load_golden('e2e_dla34_small.npz')
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    cfg = rtm3d_amd.kitti_config(bb)
    sd = weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']), heat_gain=float(g['heat_gain']))
    for key in sd:
        if key.endswith('main_kf_head.weight') or key.endswith('main_kf_head.bias'):
            sd[key][1] = sd[key][0]
    m = rtm3d_amd.create_model(cfg).to('cuda:0').eval()
    m.load_state_dict(sd)
    dim_ref = [list(r) for r in cfg.DETECTOR.dim_ref]
    dim_ref[1] = list(dim_ref[0])
    path = str(tmp_path / 'twin.rtm3d')
    m.save_engine(path, B, H, W, dim_ref=dim_ref)
    x = weights.synth_images(B, H, W, seed=int(g['img_seed'])).to(dev)
    K = torch.as_tensor(np.tile(g['K'], (B, 1)), dtype=torch.float64, device=dev)
    return m, path, dim_ref, x, K, B


def test_pipeline_and_engine_nms3d_keyword(dev, tmp_path, monkeypatch):
    m, path, dim_ref, x, K, B = twin(dev, tmp_path, monkeypatch)
    plain = Detect3DPipeline(m, B, dev, dim_ref=dim_ref, gather=False)
    base = plain.results(plain.submit(x, K), copy=True)
    off = Detect3DPipeline(m, B, dev, dim_ref=dim_ref, gather=False, nms3d=None)
    assert torch.equal(off.results(off.submit(x, K), copy=True), base)
    want = box_overlap.nms3d_records(base.clone(), 0.5)
    torch.cuda.synchronize()
    kept, left = int((base[..., 31] == 2).sum()), int((want[..., 31] == 2).sum())
    twins = sum(int(a[31] == 2 and b[31] == 2 and a[0] != b[0] and np.array_equal(a[24:31], b[24:31]) and np.isfinite(a[24:31]).all() and (a[24:27] > 0).all())
                for img in base.cpu().numpy() for k, a in enumerate(img) for b in img[k + 1:])
    print('twin planes: %d live slots, %d kept 3D boxes, %d identical valid boxes of two classes, %d kept after nms3d'
          % (int((base[..., 31] >= 1).sum()), kept, twins, left))
    assert twins >= 2 and left <= kept - twins, (kept, twins, left)
    on = Detect3DPipeline(m, B, dev, dim_ref=dim_ref, gather=False, nms3d=0.5)
    for _ in range(on.depth + 1):                                    # every slot, and one of them twice
        assert torch.equal(on.results(on.submit(x, K), copy=True), want)
    aware = Detect3DPipeline(m, B, dev, dim_ref=dim_ref, gather=False, nms3d={'iou_thresh': 0.5, 'metric': '3d', 'class_aware': True})
    assert torch.equal(aware.results(aware.submit(x, K), copy=True), box_overlap.nms3d_records(base.clone(), 0.5, metric='3d', class_aware=True))
    for p in (plain, off, on, aware):
        p.drain()
    eng = engine.Engine(path, dev)
    assert torch.equal(eng.detect(x, K), base) and torch.equal(eng.detect(x, K, nms3d=None), base)
    assert torch.equal(eng.detect(x, K, nms3d=0.5), want)
    eng.close()
