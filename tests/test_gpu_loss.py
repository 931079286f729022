"""GPU: the validation loss on the device (csrc/loss.hip through rtm3d_amd.loss) against the numpy restatement
tests/loss_ref.py and the reference-run fixture tests/golden/loss_cases.npz.

Bars (include/rtm3d_hip.h, "validation loss"): the per-object table bit-equal (fp64, the same operation order, no contraction
on either side); m_hm equal after rounding to fp32, at most 1 fp32 ulp where the two exps differ, centre cells exactly 1.0f /
0.9999f; counts exactly equal; the five losses within 1e-5 relative of the restatement - element terms differ by a few fp32
ulp of expf, logf and the division, about 1e-6, and all terms of a sum have one sign, so the sum's relative error is bounded
by the terms' - and within max(4 x the reference's own fp32-vs-fp64 distance, 1e-5 relative) of the reference's fp64 run."""
import numpy as np
import pytest
import torch

from rtm3d_amd import loss as L
from tests import loss_cases as lc, loss_ref as ref
from tests.util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def device_logits(logits, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in logits]


def run(case, dev, logits=None, cfg=None):
    """-> (items (5,) fp32, counts (5,) int32) of RTM3DLoss on the device."""
    cfg = cfg if cfg is not None else {'MODEL': {'FOCAL_LOSS_ALPHA': case['alpha'], 'FOCAL_LOSS_BEDA': case['beta']}}
    fn = L.RTM3DLoss(cfg)
    loss, items = fn(device_logits(lc.logits(case) if logits is None else logits, dev), lc.batch(case))
    torch.cuda.synchronize()
    assert loss.shape == () and items.shape == (5,) and items.dtype == torch.float32
    items, counts = items.cpu().numpy(), fn.counts.cpu().numpy()
    assert float(loss) == items[4] or (np.isnan(float(loss)) and np.isnan(items[4]))
    return items, counts


def rel_err(items, want):
    assert (np.isnan(items) == np.isnan(want)).all(), (items, want)
    ok = ~np.isnan(want)
    return (np.abs(items[ok].astype(np.float64) - want[ok].astype(np.float64)) / np.abs(want[ok].astype(np.float64))).max(initial=0.0)


@pytest.mark.parametrize('name', lc.ALL_CASES)
def test_targets_and_loss_match_the_restatement(dev, name):
    """Every fixture case (B = 1, 2, 5; the 24 x 40 and the odd 13 x 37 map; alpha = 1.5, beta = 3; no object at all; an empty
    image next to a full one; overlapping Gaussians) and every regime case (clipped squares and corner centres, noise, cls -1,
    vertices outside / negative / behind the camera / a supplied mask_3d, R = 0, R > W, m_proj outside, 150 objects in one
    image).  Measured on an MI355X: table bit-equal, m_hm 0 ulp on every case, counts equal, losses within 1.4e-7 relative of
    the restatement (bar 1e-5) and within 1.0e-7 relative of the reference's fp64 run (bar 1e-5 relative)."""
    c, b, tab, hm, items, counts = lc.restated(name)
    t = L.build_targets(lc.batch(c), c['H'], c['W'], device=dev)
    torch.cuda.synchronize()
    got = t['table'].cpu().numpy()
    assert got.shape == tab.shape and np.array_equal(got.view(np.int64), tab.view(np.int64)), np.argwhere(got.view(np.int64) != tab.view(np.int64))[:5]
    worst = lc.check_heatmap(t['m_hm'].cpu().numpy(), hm, tab)
    N = len(tab)
    assert t['m_proj'].dtype == torch.int64 and np.array_equal(t['m_proj'].cpu().numpy(), tab[:, 8:10].astype(np.int64))
    assert np.array_equal(t['v_proj'].cpu().numpy(), tab[:, 32:48].reshape(N, 8, 2).astype(np.int64))
    assert np.array_equal(t['v_mask'].cpu().numpy(), tab[:, 80:88] != 0) and np.array_equal(t['mask_3d'].cpu().numpy(), tab[:, 4] != 0)
    assert np.array_equal(t['v_off'].cpu().numpy(), tab[:, 48:64].reshape(N, 8, 2)) and np.array_equal(t['m_off'].cpu().numpy(), tab[:, 10:12])
    assert np.array_equal(t['v_coor_off'].cpu().numpy(), tab[:, 64:80].reshape(N, 8, 2))
    d_items, d_counts = run(c, dev)
    assert np.array_equal(d_counts, counts), (d_counts, counts)
    e = rel_err(d_items, items)
    print(name, 'm_hm ulp', worst, 'loss rel err vs restatement %.3g' % e, d_items, d_counts)
    assert e <= 1e-5
    if name in lc.FIXTURE_CASES:
        ef = lc.check_items_against_fixture(d_items, load_golden('loss_cases.npz'), name)
        print(name, 'loss rel err vs the reference fp64 run %.3g' % ef)


def test_person_sitting_doubles_into_two_classes(dev):
    """from_kitti: one Person_sitting row paints 0.9999 into the Pedestrian AND the Cyclist map and is no positive; the Van a
    noise Car; DontCare nothing."""
    rows = [[('Person_sitting', 0, 0, 0.1, 60., 20., 84., 40., 1.2, 0.6, 0.8, 1., 1.5, 12., 0.2), ('DontCare', -1, -1, -10, 5., 5., 20., 20., -1, -1, -1, -1000, -1000, -1000, -10),
             ('Van', 0, 0, 0., 100., 10., 124., 30., 2., 1.9, 5., 3., 1.6, 20., 0.1), ('Car', 0, 0, 0.1, 20., 24., 44., 44., 1.5, 1.6, 3.9, -2., 1.6, 20., -1.0)]]
    b = L.LabelBatch.from_kitti(rows, lc.camera(13, 37).reshape(1, 9))
    t = L.build_targets(b, 13, 37, device=dev)
    hm = t['m_hm'].cpu().numpy()
    assert t['class'].tolist() == [1, 2, -1, 0, 0] and t['noise_mask'].tolist() == [True, True, False, True, False]
    assert hm[0, 1, 7, 18] == np.float32(0.9999) and hm[0, 2, 7, 18] == np.float32(0.9999) and hm[0, 0, 5, 28] == np.float32(0.9999)
    assert hm[0, 0, 8, 8] == 1.0 and (hm == 1.0).sum() == 1 and hm[0, :, 3, 3].max() == 0
    tab = ref.object_table(b.rows, b.K, 1, 13, 37)
    assert np.array_equal(t['table'].cpu().numpy().view(np.int64), tab.view(np.int64))


def test_extreme_and_nonfinite_logits(dev):
    """Logits of +-30 and +-inf saturate at the clamp and stay finite; one NaN makes the main term and the total NaN.  Nothing
    faults: the outputs of every run are read back."""
    c, b, tab, hm, items, counts = lc.restated('fx_b5_odd')
    base = lc.logits(c)
    for fill in (30.0, -30.0, np.inf, -np.inf):
        lg = [a.copy() for a in base]
        lg[0][:, :, ::2, ::3] = fill
        lg[0][0, 0, 0, 0] = -fill
        lg[2][:, :, ::2, :] = fill
        lg[3][:, 1] = -fill
        want, wc = ref.loss(tab, b.img_start, c['B'], c['C'], c['H'], c['W'], lg, c['alpha'], c['beta'])
        got, gc = run(c, dev, lg)
        if np.isfinite(fill):
            assert np.isfinite(got).all()
        assert np.isfinite(got[[0, 2, 3]]).all() and np.array_equal(gc, wc) and rel_err(got[[0, 2, 3]], want[[0, 2, 3]]) <= 1e-5, (fill, got, want)
    lg = [a.copy() for a in base]
    lg[0][3, 1, 5, 7] = np.nan
    got, gc = run(c, dev, lg)
    assert np.isnan(got[0]) and np.isnan(got[4]) and np.isfinite(got[1:4]).all() and np.array_equal(gc, counts)
    np.testing.assert_array_equal(got[1:4], run(c, dev)[0][1:4])
    lg = [a.copy() for a in base]
    lg[1][:] = np.nan
    got, _ = run(c, dev, lg)
    assert np.isnan(got[1]) and np.isnan(got[4]) and np.isfinite(got[[0, 2, 3]]).all()


def test_unaligned_logits_take_the_scalar_path(dev):
    """W % 4 == 0 but a heat map that starts 4 bytes into an allocation: the 16-byte loads do not apply; same result."""
    c, b, tab, hm, items, counts = lc.restated('fx_b2_empty')
    lg = device_logits(lc.logits(c), dev)
    flat = torch.empty(lg[0].numel() + 1, dtype=torch.float32, device=dev)
    off = flat[1:].view(lg[0].shape)
    off.copy_(lg[0])
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    fn = L.RTM3DLoss()
    a = fn(lg, lc.batch(c))[1].cpu().numpy()
    bb = fn([off] + lg[1:], lc.batch(c))[1].cpu().numpy()
    assert rel_err(bb, items) <= 1e-5 and rel_err(a, items) <= 1e-5
    assert rel_err(bb, a) <= 1e-6                        # (another summation order within a lane: not bit-equal by rule)


def test_same_call_twice_is_bit_identical(dev):
    for name in ('fx_b1', 'many'):
        c = lc.make(name)
        fn, lg, bt = L.RTM3DLoss(), device_logits(lc.logits(c), dev), lc.batch(c)
        a = fn(lg, bt)[1].clone()
        ca = fn.counts.clone()
        for _ in range(3):
            b2 = fn(lg, bt)[1]
            assert a.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes() and torch.equal(ca, fn.counts)
        assert L.RTM3DLoss()(lg, lc.batch(c))[1].cpu().numpy().tobytes() == a.cpu().numpy().tobytes()


def test_weights_scale_the_items(dev):
    c, b, tab, hm, items, counts = lc.restated('fx_b1')
    cfg = {'TRAINING': {'W_MKF': 2.0, 'W_VFM': 0.25, 'W_M_OFF': 3.0, 'W_V_OFF': 0.0}}
    got, _ = run(c, dev, cfg=cfg)
    want, _ = ref.loss(tab, b.img_start, c['B'], c['C'], c['H'], c['W'], lc.logits(c), weights=(2.0, 0.25, 3.0, 0.0))
    assert rel_err(got[:3], want[:3]) <= 1e-5 and got[3] == 0 and rel_err(got[4:], want[4:]) <= 1e-5


def test_validation_loss_accumulates_without_synchronising(dev):
    """ValidationLoss.add over three batches of different B equals the restated batch-size weighted mean (test_epoch,
    train.py:65-81); add performs no host synchronisation (torch's sync debug mode raises on one; the library's own calls are
    launches only) - also for a batch that was not staged: its upload is from pinned memory and asynchronous -, result() is the
    one place that waits."""
    names = ('fx_b1', 'fx_b5_odd', 'fx_b2_empty')
    vl = L.ValidationLoss()
    assert np.isnan(vl.result())
    prepared = []
    for n in names:
        c = lc.make(n)
        bt = lc.batch(c)
        if n != names[-1]:                              # the last batch stays on the host: add uploads it and builds its table
            bt.to(dev).table(c['H'], c['W'])
        prepared.append((device_logits(lc.logits(c), dev), bt))
    vl.add(*prepared[0])                                # (allocates the accumulator)
    vl.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for lg, bt in prepared:
            vl.add(lg, bt)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    got = vl.result()
    tot = [(float(lc.restated(n)[4][4]), lc.restated(n)[0]['B']) for n in names]
    want = sum(t * b for t, b in tot) / sum(b for _, b in tot)
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert vl.result() == got
    vl.reset()
    vl.add(*prepared[1])
    assert abs(vl.result() - tot[1][0]) <= 1e-5 * abs(tot[1][0])
    # a batch whose loss is NaN makes the mean NaN, as the reference's loop stops on it
    c = lc.make('fx_none')
    vl.add(device_logits(lc.logits(c), dev), lc.batch(c))
    assert np.isnan(vl.result())


def test_refusals_on_the_device_side(dev):
    c = lc.make('fx_b1')
    lg, bt = device_logits(lc.logits(c), dev), lc.batch(c)
    fn = L.RTM3DLoss()
    with pytest.raises(ValueError, match='ver_coor'):
        fn([lg[0], lg[1][:, :8].contiguous(), lg[2], lg[3]], bt)
    with pytest.raises(ValueError, match='contiguous fp32'):
        fn([lg[0].double(), lg[1], lg[2], lg[3]], bt)
    with pytest.raises(RuntimeError, match='CUDA'):
        fn([a.cpu() for a in lg], bt)
    with pytest.raises(ValueError, match='images'):
        fn([torch.cat([a, a]) for a in lg], bt)
    from rtm3d_amd import _lib
    lib = _lib.load()
    assert lib.rtm3d_loss_eval(None, 1, 3, 8, 8, None, None, None, None, None, None, 0, None, None, None, None, None) != 0
    assert b'null' in lib.rtm3d_last_error()
    assert lib.rtm3d_loss_objects(None, -1, 1, None, None, 4.0, 8, 8, None) != 0 and lib.rtm3d_loss_workspace_bytes(0, 3, 8, 8) == 0
    assert lib.rtm3d_loss_heatmap(None, 1, 70000, 8, 8, None, None, 0, None) != 0


def test_model_logits_into_the_loss_end_to_end(dev):
    """A small DLA-34 forward (model(x)[1], as train.py:71 takes it) into RTM3DLoss and into test_epoch, against the
    restatement on the same logits."""
    import rtm3d_amd
    from rtm3d_amd import weights
    cfg = rtm3d_amd.kitti_config('DLA-34')
    model = rtm3d_amd.create_model(cfg).to(dev).eval()
    model.load_state_dict(weights.synth_state_dict('DLA-34', 1, 'trained', heat_bias=-3.0))
    B, Hin, Win = 2, 128, 256
    H, W = Hin // 4, Win // 4
    x = weights.synth_images(B, Hin, Win).to(dev)
    rng = np.random.default_rng(3)
    objs = sum([lc._scene(rng, b, 4, H, W) for b in range(B)], [])
    c = lc._case(B, H, W, objs)
    bt = lc.batch(c)
    pred = model(x)[1]
    loss, items = L.RTM3DLoss(cfg)(pred, bt)
    torch.cuda.synchronize()
    tab = ref.object_table(bt.rows, bt.K, B, H, W)
    want, wc = ref.loss(tab, bt.img_start, B, 3, H, W, [p.cpu().numpy() for p in pred])
    got = items.cpu().numpy()
    assert np.isfinite(got).all() and wc[0] > 0 and rel_err(got, want) <= 1e-5, (got, want)
    mean = L.test_epoch(model, [(x, bt), (x, lc.batch(c))], cfg)
    assert mean is not None and abs(mean - float(got[4])) <= 1e-6 * abs(float(got[4]))
