"""GPU: rtm3d_frames_augment (csrc/augment.hip) BYTE FOR BYTE against the numpy restatement tests/augment_ref.py over the case
tables of tests/augment_cases.py - every branch of the pixel rule over small shapes, the three output modes, the identity against
preprocess_batch, every address modulo 4, every chunk boundary, determinism, the noise statistics, a refused call, and the facade
end to end into RTM3DLoss.  Packed destinations carry 64 guard bytes of 0xA5 on both sides."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                            # noqa: E402
from rtm3d_amd import _lib, augment, preprocess, weights    # noqa: E402
from rtm3d_amd.loss import RTM3DLoss                        # noqa: E402
from tests import augment_cases as ac                       # noqa: E402
from tests import augment_ref as ref                        # noqa: E402

GUARD, GUARD_BYTE = 64, 0xA5
SENTINEL16 = 0x7E55                                         # a NaN pattern no table holds
SUMS_JUNK = 0x5A5A5A5A5A5A
NOISE_SEED = 0x9E3779B97F4A7C15                             # confirmed on the CPU: mean 0.084, variance 51.29 over 12288 values


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def luts(dev):
    """(device fp32 table, device fp16 table, host fp32 [3][256], host fp16 [3][256] as uint16 bits)"""
    d32, d16 = preprocess.device_luts(ac.MEAN, ac.STD, dev)
    h32 = preprocess.normalize_lut(ac.MEAN, ac.STD)
    return d32, d16, h32, np.ascontiguousarray(h32.astype(np.float16)).view(np.uint16)


TABLE = ref.noise_table()
_REF = {}


def reference(key, jobs, H, W):
    """The reference canvases of a job list, computed once per key and shared (read-only) by the tests that need them."""
    if key not in _REF:
        out = [ac.reference_canvas(src, d, H, W, TABLE) for src, d in jobs]
        for c in out:
            c.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def c_frames(jobs):
    arr = (_lib.AugmentFrameC * len(jobs))()
    for f, (_, d) in zip(arr, jobs):
        for k in ('h', 'w', 'x0', 'y0', 'rw', 'rh', 'alpha_q', 'beta_q', 'sigma_q', 'ax', 'bx', 'ay', 'by'):
            setattr(f, k, int(d[k]))
        f.seed_lo, f.seed_hi = int(d['seed']) & 0xFFFFFFFF, int(d['seed']) >> 32
        f.fill[0], f.fill[1], f.fill[2] = d['fill']
    return arr


def at_offset(arr, dev, offset):
    """A numpy uint8 array on the device, `offset` bytes into an allocation of its own."""
    flat = np.ascontiguousarray(arr).reshape(-1)
    buf = torch.empty(offset + flat.size, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[offset:].copy_(torch.from_numpy(flat))
    return buf[offset:].view(arr.shape)


def launch(dev, luts, jobs, H, W, mode, out_ptr, border=0, src_offset=0, sums=None, srcs=None):
    """One rtm3d_frames_augment call (chunks of 32 inside); jobs that hold the same source array share one device copy."""
    lib = _lib.load()
    if srcs is None:
        shared = {}
        for src, _ in jobs:
            if id(src) not in shared:
                shared[id(src)] = at_offset(src, dev, src_offset)
        srcs = [shared[id(src)] for src, _ in jobs]
    table = augment.device_noise_table(dev)
    sums = sums if sums is not None else torch.empty(len(jobs), 3, dtype=torch.int64, device=dev)
    rc = lib.rtm3d_frames_augment(_lib.stream_ptr(dev), len(jobs), _lib.ptr_array(srcs), c_frames(jobs), ctypes.c_void_p(out_ptr), mode, H, W,
                                  border, table.data_ptr(), luts[0].data_ptr(), luts[1].data_ptr(), sums.data_ptr())
    return rc, sums, srcs


def run_packed(dev, luts, jobs, H, W, src_offset=0, dst_offset=0):
    """Mode 2 into a guarded buffer -> (B, H, W, 3) uint8 numpy."""
    n = len(jobs) * H * W * 3
    buf = torch.full((dst_offset + GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    at = dst_offset + GUARD
    rc, sums, _ = launch(dev, luts, jobs, H, W, 2, buf.data_ptr() + at, src_offset=src_offset)
    assert rc == 0, _lib.load().rtm3d_last_error().decode()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:at] == GUARD_BYTE).all() and (host[at + n:] == GUARD_BYTE).all(), 'a guard byte was written'
    return host[at:at + n].reshape(len(jobs), H, W, 3), sums.cpu().numpy()


def compare(got, want, jobs, what):
    for i, (g, w_) in enumerate(zip(got, want)):
        if not np.array_equal(g, w_):
            d = jobs[i][1]
            bad = np.argwhere((g != w_).any(axis=-1))
            raise AssertionError('%s: frame %d (%s) differs at %d pixels, first (y, x) = %s: got %s want %s'
                                 % (what, i, {k: d[k] for k in ('h', 'w', 'x0', 'y0', 'rw', 'rh', 'alpha_q', 'beta_q', 'sigma_q', 'flip', 'scale')},
                                    len(bad), bad[0].tolist(), g[tuple(bad[0])].tolist(), w_[tuple(bad[0])].tolist()))


# ---------------------------------------------------------------------------------------------------- 1. every branch
@pytest.mark.parametrize('canvas', ac.CANVASES)
def test_every_branch_over_small_shapes(dev, luts, canvas):
    """Every source size x every rectangle width x every parameter set on one canvas size, in ONE call (hundreds of frames: every
    chunk is full), the rectangles at drawn places."""
    H, W = canvas
    jobs = ac.shape_jobs(H, W, seed=100 + ac.CANVASES.index(canvas))
    want = reference(('shapes', canvas), jobs, H, W)
    got, sums = run_packed(dev, luts, jobs, H, W)
    compare(got, want, jobs, 'canvas %s' % (canvas,))
    for i, ((_, d), w_) in enumerate(zip(jobs, want)):                      # the channel sums the border colour came from
        rect = w_[d['y0']:d['y0'] + d['rh'], d['x0']:d['x0'] + d['rw']].reshape(-1, 3).astype(np.int64)
        assert np.array_equal(sums[i], rect.sum(axis=0)), i
    # the table reaches what it is about: OUT pixels in the fill colour, both clips, partial runs at both ends
    names = [ac.PARAM_NAMES[i % len(ac.PARAM_NAMES)] for i in range(len(jobs))]
    out_seen = any(n == 'zoom_out_fill' and d['rw'] >= 8 and (w_[d['y0']:d['y0'] + d['rh'], d['x0']:d['x0'] + d['rw']] == (7, 200, 255)).all(axis=-1).any()
                   for n, (_, d), w_ in zip(names, jobs, want))
    assert out_seen and {d['x0'] % 4 for _, d in jobs} == {0, 1, 2, 3} and {(d['x0'] + d['rw']) % 4 for _, d in jobs} == {0, 1, 2, 3}
    assert any(d['x0'] == 0 for _, d in jobs) and any(d['x0'] + d['rw'] == W for _, d in jobs) and any(d['rh'] == H for _, d in jobs)


# ---------------------------------------------------------------------------------------------------- 2. modes
def test_modes_are_the_tables_applied_to_the_packed_bytes(dev, luts):
    """Modes 0 and 1 against the normalisation tables applied to the reference's bytes (which mode 2 equals, test 1): every
    pixel written (the buffers start as NaN / a sentinel), mode 1 for every phase of the border, whose ring stays untouched."""
    H, W = 33, 65
    jobs = ac.shape_jobs(H, W, seed=101)[::5]
    want = reference(('shapes', (H, W)), ac.shape_jobs(H, W, seed=101), H, W)[::5]
    B = len(jobs)
    out = torch.full((B, 3, H, W), float('nan'), dtype=torch.float32, device=dev)
    rc, _, _ = launch(dev, luts, jobs, H, W, 0, out.data_ptr())
    assert rc == 0
    got = out.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b].view(np.uint32), ref.normalise32(want[b], luts[2]).view(np.uint32), err_msg='fp32 frame %d' % b)
    # fp32 at a base that is 4- but not 16-byte aligned: the scalar stores
    flat = torch.full((B * 3 * H * W + 1,), float('nan'), dtype=torch.float32, device=dev)
    rc, _, _ = launch(dev, luts, jobs, H, W, 0, flat.data_ptr() + 4)
    assert rc == 0 and torch.equal(flat[1:].view(B, 3, H, W).cpu().view(torch.int32), torch.from_numpy(got).view(torch.int32))
    for P in (0, 1, 2, 3, 4):
        t = torch.full((B, H + 2 * P, W + 2 * P, 4), SENTINEL16, dtype=torch.int16, device=dev)
        rc, _, _ = launch(dev, luts, jobs, H, W, 1, t.data_ptr(), border=P)
        assert rc == 0
        g16 = t.cpu().numpy().view(np.uint16)
        ring = np.ones(g16.shape[1:3], bool)
        ring[P:P + H, P:P + W] = False
        assert (g16[:, ring] == SENTINEL16).all(), 'border %d: the ring was written' % P
        for b in range(B):
            np.testing.assert_array_equal(g16[b, P:P + H, P:P + W], ref.normalise16(want[b], luts[3]), err_msg='nhwc4 border %d frame %d' % (P, b))


def test_mode_1_through_a_models_input_tensor(dev, luts):
    """augment.frames(model=m) at the smallest canvas a plan takes (32 x 64): the plan's own input tensor, read back, holds the
    reference's fp16 canvases, and forward_logits(None, preloaded=...) runs on it."""
    from tests.conv_harness import D2H, _hip_memcpy
    bb = 'RESNET-18'
    m = rtm3d_amd.create_model(rtm3d_amd.kitti_config(bb)).to(dev).eval()
    m.load_state_dict(weights.synth_state_dict(bb, 1, 'trained', heat_bias=-3.5))
    H, W, B = 32, 64, 3
    rng = np.random.Generator(np.random.PCG64(31))
    srcs = [ac.frame_bytes(h, w, rng) for h, w in ((20, 60), (32, 64), (25, 53))]
    P = augment.AugmentParams.identity(B)
    P.alpha[:], P.beta[:], P.sigma[:], P.seed[:] = (1.1, 0.9, 1.0), (0.05, 0.0, -0.1), (3.2, 7.0, 0.0), (11, 2 ** 40 + 5, 3)
    P.scale[:], P.flip[:] = (1.1, 1.0, 1.2), (True, False, True)
    for b, s in enumerate(srcs):
        rh, rw = augment.resized_size(s.shape[0], s.shape[1], 64)
        P.offset[b] = augment.affine_offset_of(rw, rh, P.scale[b])
    ret, pads, rhw = augment.frames([torch.from_numpy(s).to(dev) for s in srcs], P, (H, W), ac.MEAN, ac.STD, resize_to=64, model=m)
    assert ret is None
    base, border = m.input_tensor(B, H, W)
    torch.cuda.synchronize()
    got = np.empty((B, H + 2 * border, W + 2 * border, 4), np.uint16)
    _hip_memcpy(_lib.load(), got.ctypes.data, base, got.nbytes, D2H)
    desc, _ = augment.descriptors([s.shape[:2] for s in srcs], P, (H, W), 64)
    aq, bq, sq = augment.quantise(P)
    for b, s in enumerate(srcs):
        f = desc[b]
        assert (f.rh, f.rw) == rhw[b] and (f.x0, f.y0) == pads[b]
        want = ref.canvas(s, H, W, f.x0, f.y0, f.rw, f.rh, (f.ax, f.bx, f.ay, f.by), alpha_q=int(aq[b]), beta_q=int(bq[b]), sigma_q=int(sq[b]),
                          seed=int(P.seed[b]), table=TABLE)
        np.testing.assert_array_equal(got[b, border:border + H, border:border + W], ref.normalise16(want, luts[3]), err_msg='frame %d' % b)
    logits = m.forward_logits(None, preloaded=(B, H, W))
    torch.cuda.synchronize()
    assert len(logits) == 4 and all(bool(torch.isfinite(t).all()) for t in logits)


# ---------------------------------------------------------------------------------------------------- 3. identity
def test_identity_is_preprocess_batch(dev):
    """Identity parameters, no Resize: mode 0 equals preprocess_batch on the same frames bit for bit, mean-coloured border included."""
    rng = np.random.Generator(np.random.PCG64(32))
    H, W = 48, 64
    frames = [torch.from_numpy(ac.frame_bytes(h, w, rng)).to(dev) for h, w in ((48, 64), (37, 53), (5, 4), (1, 1), (2, 2), (48, 1), (1, 64))]
    want, pads_p, rhw_p = preprocess.preprocess_batch(frames, (H, W), ac.MEAN, ac.STD)
    got, pads, rhw = augment.frames(frames, augment.AugmentParams.identity(len(frames)), (H, W), ac.MEAN, ac.STD)
    torch.cuda.synchronize()
    assert pads == pads_p and rhw == rhw_p and got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 4. addresses
def test_address_sweep(dev, luts):
    """Source and destination bases at byte offsets 0..3: the same bytes come out wherever they lie (an odd H * W puts the later
    frames of a batch at every address modulo 4 as well)."""
    H, W = 33, 65
    jobs = ac.shape_jobs(H, W, seed=101)[3::7]
    want = reference(('shapes', (H, W)), ac.shape_jobs(H, W, seed=101), H, W)[3::7]
    for so in range(4):
        for do in range(4):
            got, _ = run_packed(dev, luts, jobs, H, W, src_offset=so, dst_offset=do)
            compare(got, want, jobs, 'source + %d, destination + %d' % (so, do))


# ---------------------------------------------------------------------------------------------------- 5. chunks
@pytest.mark.parametrize('B', [1, 31, 32, 33, 65])
def test_chunk_boundaries(dev, luts, B):
    """Frames of unequal sizes and rectangles across every chunk boundary (32 frames per launch), every parameter set in turn."""
    H, W = 32, 32
    pool = ac.shape_jobs(H, W, seed=100)
    jobs = [pool[(7 * i) % len(pool)] for i in range(65)][:B]
    want = reference(('shapes', (H, W)), pool, H, W)
    want = [want[(7 * i) % len(pool)] for i in range(B)]
    got, _ = run_packed(dev, luts, jobs, H, W)
    compare(got, want, jobs, 'B = %d' % B)


# ---------------------------------------------------------------------------------------------------- 6. determinism
def test_determinism_and_batch_position(dev, luts):
    H, W = 48, 64
    rng = np.random.Generator(np.random.PCG64(33))
    src = ac.frame_bytes(37, 53, rng)
    other = ac.frame_bytes(5, 4, rng)
    d = ac.descriptor(37, 53, 3, 2, 57, 44, 'all_on', seed=77)
    filler = ac.descriptor(5, 4, 1, 1, 9, 7, 'noise', seed=5)
    a, _ = run_packed(dev, luts, [(src, d)], H, W)
    b, _ = run_packed(dev, luts, [(src, d)], H, W)
    assert np.array_equal(a, b)                                                   # the same seed: the same bytes
    c, _ = run_packed(dev, luts, [(src, dict(d, seed=78))], H, W)
    assert not np.array_equal(a, c)                                               # another seed: other bytes
    many, _ = run_packed(dev, luts, [(other, filler)] * 40 + [(src, d)] + [(other, filler)] * 3, H, W)
    assert np.array_equal(many[40], a[0])                                         # a frame's bytes do not hang on its place in the batch
    compare(a, [ac.reference_canvas(src, d, H, W, TABLE)], [(src, d)], 'all_on')


# ---------------------------------------------------------------------------------------------------- 7. noise statistics
def test_noise_statistics(dev, luts):
    """A flat source of 128, 64 x 64, identity map, sigma_q = 453 (sigma^2 = 50): the device's bytes are the reference's, and the
    reference's 12288 noise values have |mean| < 0.3 and a variance within 5 % of 50 (both more than 4 standard errors:
    sigma / sqrt(12288) = 0.064, and the variance of a variance estimate of 12288 normal values is 2 sigma^4 / n: 0.64)."""
    H = W = 64
    src = np.full((H, W, 3), 128, np.uint8)
    ax, bx, ay, by = ref.geometry(H, W, H, W)
    d = dict(h=H, w=W, x0=0, y0=0, rw=W, rh=H, alpha_q=65536, beta_q=0, sigma_q=453, seed=NOISE_SEED, fill=(0, 0, 0), ax=ax, bx=bx, ay=ay, by=by,
             flip=0, scale=1.0)
    n = ref.noise_values(H, W, 453, NOISE_SEED, TABLE)
    print('noise: mean %.4f variance %.4f min %d max %d' % (n.mean(), n.var(), n.min(), n.max()))
    assert n.size == 12288 and abs(n.mean()) < 0.3 and abs(n.var() - 50) < 0.05 * 50
    got, _ = run_packed(dev, luts, [(src, d)], H, W)
    assert np.array_equal(got[0].astype(np.int64) - 128, n)
    compare(got, [ac.reference_canvas(src, d, H, W, TABLE)], [(src, d)], 'noise')


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_a_refused_call_has_launched_nothing(dev, luts):
    """A batch whose LAST frame is refused (beyond the first chunk): destination, guards and channel sums are as they were."""
    H, W = 32, 32
    pool = ac.shape_jobs(H, W, seed=100)
    for bad in (dict(sigma_q=65536), dict(x0=30, rw=8), dict(ax=1 << 40)):
        jobs = pool[:39] + [(pool[39][0], dict(pool[39][1], **bad))]
        n = len(jobs) * H * W * 3
        buf = torch.full((GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        sums = torch.full((len(jobs), 3), SUMS_JUNK, dtype=torch.int64, device=dev)
        rc, _, _ = launch(dev, luts, jobs, H, W, 2, buf.data_ptr() + GUARD, sums=sums)
        torch.cuda.synchronize()
        assert rc != 0 and 'frame 39' in _lib.load().rtm3d_last_error().decode(), bad
        assert bool((buf == GUARD_BYTE).all()) and bool((sums == SUMS_JUNK).all()), bad
    # a packed destination that overlaps a source
    src = torch.full((5 * 4 * 3 + H * W * 3,), 7, dtype=torch.uint8, device=dev)
    d = ac.descriptor(5, 4, 0, 0, 9, 7, 'identity', seed=0)
    rc, _, _ = launch(dev, luts, [(None, d)], H, W, 2, src.data_ptr() + 59, srcs=[src[:60].view(5, 4, 3)])
    torch.cuda.synchronize()
    assert rc != 0 and 'overlaps' in _lib.load().rtm3d_last_error().decode() and bool((src == 7).all())
    with pytest.raises(RuntimeError, match='frame 0'):
        P = augment.AugmentParams.identity(1)
        P.sigma[0] = 1023.99                                                       # sigma_q 65535: fine
        P.scale[0] = 1e-7                                                          # |ax| beyond 2^40
        augment.frames([src[:60].view(5, 4, 3)], P, (H, W), ac.MEAN, ac.STD)


# ---------------------------------------------------------------------------------------------------- 9. end to end
def test_train_augmentation_feeds_the_loss(dev):
    """TrainAugmentation on 4 small frames with two labels each -> RTM3DLoss on random logits: a finite loss, a gradient that is
    not zero; and on the device's own packed canvas the painted marker lies where the moved label says (the CPU test's bound)."""
    h, w, size = 60, 200, (64, 224)
    centres = [(120, 25), (60, 30), (150, 35), (90, 20)]
    frames, rows = [], []
    for cx, cy in centres:
        f = np.full((h, w, 3), 100, np.uint8)
        f[cy - 1:cy + 2, cx - 1:cx + 2] = 250
        frames.append(torch.from_numpy(f).to(dev))
        rows.append([['Car', 0.0, 0.0, 0.1, cx - 10.0, cy - 8.0, cx + 10.0, cy + 8.0, 1.5, 1.6, 3.9, (cx - 100) / 35.0, 1.5, 20.0, 0.4],
                     ['Pedestrian', 0.0, 0.0, -0.2, 20.0, 10.0, 34.0, 50.0, 1.7, 0.6, 0.8, -2.3, 1.6, 20.0, -1.0]])
    K = [np.array([700., 0, 100, 0, 700, 30, 0, 0, 1])] * 4
    aug = augment.TrainAugmentation(size, ac.MEAN, ac.STD, rng=np.random.Generator(np.random.PCG64(9)), resize_to=0)
    inp, batch, params = aug(frames, rows, K)
    assert inp.shape == (4, 3, 64, 224) and inp.dtype == torch.float32 and bool(torch.isfinite(inp).all())
    assert batch.B == 4 and batch.N == 8 and (batch.rows[0::2, 1] == 0).all()
    assert params.flip.any() and not params.flip.all() and (params.scale != 1).any()          # this draw mirrors and zooms some frames
    g = torch.Generator(device='cpu').manual_seed(3)
    logits = [torch.randn(4, c, 16, 56, generator=g).to(dev).requires_grad_(True) for c in (3, 16, 2, 2)]
    loss, items = RTM3DLoss(None)(logits, batch)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(t.grad).all()) for t in logits)
    assert all(float(t.grad.abs().sum()) > 0 for t in logits)
    # the geometry of the same draw without its photometric half, as packed bytes
    geo = augment.AugmentParams(np.ones(4), np.zeros(4), np.zeros(4), params.seed, params.scale, params.offset, params.flip, params.fill)
    canv, pads, rhw = augment.frames(frames, geo, size, ac.MEAN, ac.STD, mode='uint8')
    canv = canv.cpu().numpy()
    for b in range(4):
        (x0, y0), (rh, rw) = pads[b], rhw[b]
        wgt = canv[b, y0:y0 + rh, x0:x0 + rw, 0].astype(np.float64) - 100
        assert wgt.min() >= 0 and wgt.sum() > 0
        ys, xs = np.mgrid[y0:y0 + rh, x0:x0 + rw]
        px, py = (wgt * xs).sum() / wgt.sum(), (wgt * ys).sum() / wgt.sum()
        r = batch.rows[2 * b]
        print('frame %d: centroid (%.3f, %.3f), label centre (%.3f, %.3f)' % (b, px, py, (r[3] + r[5]) / 2, (r[4] + r[6]) / 2))
        assert abs(px - (r[3] + r[5]) / 2) <= 1.5 and abs(py - (r[4] + r[6]) / 2) <= 1.5
