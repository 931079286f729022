"""CPU: the training augmentation without a device (include/rtm3d_hip.h, "training augmentation") - Philox against the published
known answers, the noise table, the labels against the reference's own chain (tests/golden/augment_cases.npz, made by
tests/golden/make_golden_augment.py), the geometry and the plan against the numpy restatement (tests/augment_ref.py) and the
regime table (tests/augment_cases.py), every refusal of rtm3d_frames_augment_check, and that header, binding and library agree."""
import ctypes
import os
import re
import shutil
import statistics
import subprocess

import numpy as np
import pytest

from rtm3d_amd import _lib, augment
from rtm3d_amd.loss import transform_obj_label
from tests import augment_cases as ac
from tests import augment_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['rtm3d_augment_noise_table', 'rtm3d_augment_geometry', 'rtm3d_frames_augment_plan', 'rtm3d_frames_augment_check', 'rtm3d_frames_augment']


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'augment_cases.npz'), allow_pickle=False)


# ------------------------------------------------------------------------------------------------ Philox, the noise table
@pytest.mark.parametrize('ctr, key, want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(ctr, key, want):
    assert ' '.join('%08x' % int(v) for v in ref.philox4x32_10(ctr, key)) == want
    # ... and as one element of an array of counters
    c0 = np.array([5, ctr[0], 9], np.uint64)
    got = ref.philox4x32_10((c0, ctr[1], ctr[2], ctr[3]), key)
    assert ' '.join('%08x' % int(v[1]) for v in got) == want


def test_noise_table(lib):
    T = augment.noise_table()
    nd = statistics.NormalDist()
    want = np.array([round(1024 * nd.inv_cdf((k + 0.5) / 4096)) for k in range(4096)], np.int64)
    assert T.dtype == np.int16 and np.array_equal(T, want) and np.array_equal(T, ref.noise_table())
    assert np.array_equal(T, -T[::-1]) and int(T.max()) == 3756 and int(T.min()) == -3756
    # no entry near a rounding tie: the table does not hang on the last bits of the inverse
    frac = np.array([1024 * nd.inv_cdf((k + 0.5) / 4096) for k in range(4096)])
    assert np.abs(np.abs(frac - np.floor(frac)) - 0.5).min() > 2.8e-5
    for sigma_q, var in ((202, 10.0), (453, 50.0)):
        n = (T.astype(np.int64) * sigma_q + 32768) >> 16
        print('sigma_q %d: mean %g variance %g' % (sigma_q, n.mean(), n.var()))
        assert n.mean() == 0 and abs(n.var() - var) < 0.01 * var
    assert lib.rtm3d_augment_noise_table(None) != 0


# ------------------------------------------------------------------------------------------------ labels
def fixture_case(g, c):
    p = 'c%02d_' % c
    names = [str(s) for s in g['names']]
    h, w, resize_to, H, W, rh, rw = (int(v) for v in g[p + 'frame'])
    rows = g[p + 'rows']
    fired, scale, ox, oy, flip = g[p + 'draw']
    krows = [[names[int(r[0])]] + [float(v) for v in r[1:]] for r in rows]
    P = augment.AugmentParams.identity(1)
    P.scale[0], P.offset[0], P.flip[0] = scale, (ox, oy), bool(flip)
    return dict(p=p, hw=(h, w), resize_to=resize_to, size=(H, W), rhw=(rh, rw), rows=rows, krows=krows, params=P, fired=int(fired), flip=int(flip))


def test_labels_equal_the_references_chain(golden):
    g = golden
    objs = [str(s) for s in g['objs']]
    rel = [str(s).split('|') for s in g['relate']]
    assert objs == ['Car', 'Pedestrian', 'Cyclist'] and rel == [['Van', 'Truck'], ['Person_sitting'], ['Person_sitting']]
    seen = dict(combos=set(), narrow=0, centre=0, doubled=0, noise=0, ry=set(), resize=set())
    for c in range(int(g['n_cases'])):
        k = fixture_case(g, c)
        p = k['p']
        assert np.array_equal(augment.affine_offset_of(k['rhw'][1], k['rhw'][0], k['params'].scale[0]), k['params'].offset[0]) or not k['fired']
        lb = augment.labels([k['krows']], [g['K0']], [k['hw']], k['params'], k['size'], k['resize_to'])
        cls, noise, rep = transform_obj_label([r[0] for r in k['krows']], objs, rel)
        idx = np.repeat(np.arange(len(k['rows'])), rep)
        bb = k['rows'][idx, 4:8]
        narrow = ((bb[:, 2] - bb[:, 0]) <= 2) | ((bb[:, 3] - bb[:, 1]) <= 2)
        keep = (cls != -1) & ~narrow                       # what RemoveBadBBox leaves: the rows the reference still holds
        assert lb.N == len(idx) and np.array_equal(lb.rows[~keep, 1], np.full((~keep).sum(), -1.0))        # nothing is compacted
        R = lb.rows[keep]
        assert np.array_equal(R[:, 3:7], g[p + 'bbox']), c
        assert np.array_equal(lb.K[0], g[p + 'K'][0]) and (g[p + 'K'] == g[p + 'K'][0]).all(), c
        assert np.array_equal(R[:, 13], g[p + 'Ry']) and np.array_equal(R[:, 10:13], g[p + 'location']), c
        assert np.array_equal(R[:, 1] != -1, g[p + 'mask'] != 0), c
        alive = g[p + 'mask'] != 0
        assert np.array_equal(R[alive, 1], g[p + 'class'][alive]) and np.array_equal(R[:, 2], g[p + 'noise_mask']), c
        assert np.array_equal(R[:, 7:10], g[p + 'dimension']) and (lb.rows[:, 16] == -1).all(), c           # mask_3d stays derived
        seen['combos'].add((k['fired'], k['flip']))
        seen['narrow'] += int((narrow & (cls != -1)).sum()); seen['centre'] += int((~alive).sum())
        seen['doubled'] += int((np.array(rep) == 2).sum()); seen['noise'] += int(noise.sum())
        seen['ry'] |= set(np.sign(k['rows'][:, 14]).tolist()); seen['resize'].add(k['rhw'] != k['hw'])
    assert seen['combos'] == {(0, 0), (0, 1), (1, 0), (1, 1)} and seen['ry'] == {-1.0, 0.0, 1.0} and seen['resize'] == {True, False}
    assert seen['narrow'] >= 12 and seen['centre'] >= 8 and seen['doubled'] >= 24 and seen['noise'] >= 48, seen


def test_labels_identity_is_from_kitti(golden):
    """Identity parameters and no Resize: the rows of LabelBatch.from_kitti with the letterbox pad, except the boxes RemoveBadBBox
    and the centre mask take."""
    from rtm3d_amd.loss import LabelBatch
    k = fixture_case(golden, 1)                                       # 370 x 1280 on 384 x 1280, no Resize
    assert k['rhw'] == k['hw']
    lb = augment.labels([k['krows'], k['krows'][:2]], [golden['K0']] * 2, [k['hw']] * 2, augment.AugmentParams.identity(2), k['size'])
    fk = LabelBatch.from_kitti([k['krows'], k['krows'][:2]], [golden['K0']] * 2, pad=(0.0, 7.0))
    assert lb.N == fk.N and np.array_equal(lb.img_start, fk.img_start) and np.allclose(lb.K, fk.K, rtol=1e-15, atol=0)
    same = lb.rows[:, 1] == fk.rows[:, 1]
    assert same.sum() >= 4 and (lb.rows[~same, 1] == -1).all()
    assert np.allclose(lb.rows[:, 3:7], fk.rows[:, 3:7], rtol=1e-15, atol=1e-12) and np.array_equal(lb.rows[:, 7:16], fk.rows[:, 7:16])
    m3 = [np.arange(len(k['krows'])) % 2, [1, 0]]
    lb3 = augment.labels([k['krows'], k['krows'][:2]], [golden['K0']] * 2, [k['hw']] * 2, augment.AugmentParams.identity(2), k['size'], mask_3d=m3)
    assert set(lb3.rows[:, 16].tolist()) == {0.0, 1.0}


def test_draw_follows_the_references_defaults():
    rng = np.random.Generator(np.random.PCG64(5))
    P = augment.AugmentParams.draw(4000, (375, 1242), 1280, rng)
    photo, noisy, zoom = (P.alpha != 1) | (P.beta != 0), P.sigma > 0, P.scale != 1
    for m in (photo, noisy, zoom, P.flip):
        assert abs(m.mean() - 0.5) < 0.04                                               # p = 0.5 each: 4000 draws, 5 standard errors
    assert (np.abs(P.alpha[photo] - 1) <= 0.2).all() and (np.abs(P.beta[photo]) <= 0.2).all()
    assert (P.sigma[noisy] ** 2 >= 10 - 1e-9).all() and (P.sigma[noisy] ** 2 <= 50 + 1e-9).all()
    assert (P.scale[zoom] >= 1).all() and (P.scale[zoom] <= 1.2).all() and (P.offset[~zoom] == 0).all()
    rh, rw = 386, 1280
    for b in np.flatnonzero(zoom)[:50]:
        wh = np.array([rw, rh], np.float32)
        assert np.array_equal(P.offset[b], ((wh - wh * np.float32(P.scale[b])) / np.float32(2)).astype(np.float64))
    assert len(set(P.seed.tolist())) == 4000
    I = augment.AugmentParams.identity(3)
    assert [tuple(int(v[0]) for v in augment.quantise(I))] == [(65536, 0, 0)] and (I.scale == 1).all() and not I.flip.any()


# ------------------------------------------------------------------------------------------------ geometry
def c_geometry(lib, h, w, rh, rw, pad_w, pad_h, scale, ox, oy, flip):
    g = _lib.FrameGeom(h, w, rh, rw, pad_w, pad_h)
    f = _lib.AugmentFrameC()
    f.alpha_q, f.sigma_q = 12345, 77                                   # fields the function must leave alone
    rc = lib.rtm3d_augment_geometry(ctypes.byref(g), scale, ox, oy, flip, ctypes.byref(f))
    return rc, f


def test_geometry_equals_the_restatement(lib):
    rng = np.random.Generator(np.random.PCG64(6))
    sizes = [(375, 1242, 386, 1280), (370, 1280, 370, 1280), (376, 1241, 193, 639), (1, 1, 1, 1), (2, 2, 7, 9), (37, 53, 33, 64), (16384, 16384, 1, 1),
             (1, 1, 16384, 16384)]
    for h, w, rh, rw in sizes:
        for _ in range(12):
            scale = float(rng.choice([1.0, rng.uniform(1, 1.2), rng.uniform(0.3, 3)]))
            ox, oy = (0.0, 0.0) if rng.random() < 0.3 else (float(rng.uniform(-0.3, 0.3) * rw), float(rng.uniform(-0.3, 0.3) * rh))
            flip = int(rng.integers(0, 2))
            rc, f = c_geometry(lib, h, w, rh, rw, 3, 5, scale, ox, oy, flip)
            assert rc == 0 and (f.ax, f.bx, f.ay, f.by) == ref.geometry(h, w, rh, rw, scale, ox, oy, flip), (h, w, rh, rw, scale, ox, oy, flip)
            assert (f.h, f.w, f.x0, f.y0, f.rw, f.rh, f.alpha_q, f.sigma_q) == (h, w, 3, 5, rw, rh, 12345, 77)
    # the identity with equal sizes: sx == 32 * x for every x
    rc, f = c_geometry(lib, 16384, 16384, 16384, 16384, 0, 0, 1.0, 0.0, 0.0, 0)
    assert rc == 0 and (f.ax, f.bx, f.ay, f.by) == (32 * 65536, 32768, 32 * 65536, 32768)
    x = np.arange(16384, dtype=np.int64)
    assert np.array_equal((x * f.ax + f.bx) >> 16, 32 * x)
    # the mirror of the identity: sx == 32 * (w - 1 - x)
    rc, f = c_geometry(lib, 5, 1242, 5, 1242, 0, 0, 1.0, 0.0, 0.0, 1)
    x = np.arange(1242, dtype=np.int64)
    assert rc == 0 and np.array_equal((x * f.ax + f.bx) >> 16, 32 * (1241 - x))
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf')), dict(ox=float('nan')), dict(oy=float('inf')),
               dict(rw=0), dict(h=0), dict(scale=1e-300)):
        a = dict(h=4, w=4, rh=4, rw=4, pad_w=0, pad_h=0, scale=1.0, ox=0.0, oy=0.0, flip=0)
        a.update(kw)
        rc, _ = c_geometry(lib, **a)
        assert rc != 0 and lib.rtm3d_last_error().decode().startswith('augment_geometry'), kw
    assert lib.rtm3d_augment_geometry(None, 1.0, 0.0, 0.0, 0, None) != 0


# ------------------------------------------------------------------------------------------------ pixels follow labels
@pytest.mark.parametrize('resize_to, size', [(None, (64, 224)), (160, (64, 160)), (256, (96, 256))])
@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('zoom', [0, 1])
def test_pixels_follow_labels_on_the_restatement(lib, resize_to, size, flip, zoom):
    """A 3 x 3 block painted at a label's bbox centre in a flat source: after the augmentation the block's centroid on the canvas
    lies within 1.5 px of the transformed bbox centre (the reference's mirror moves boxes by w' - x and pixels by w' - 1 - x, and
    its Resize scales boxes about the corner and pixels about their centres: the bound is not 1)."""
    h, w = 60, 200
    cx, cy = 120, 25
    src = np.full((h, w, 3), 100, np.uint8)
    src[cy - 1:cy + 2, cx - 1:cx + 2] = 250
    row = ['Car', 0.0, 0.0, 0.1, cx - 10.0, cy - 8.0, cx + 10.0, cy + 8.0, 1.5, 1.6, 3.9, 1.0, 1.5, 20.0, 0.4]
    P = augment.AugmentParams.identity(1)
    rh, rw = augment.resized_size(h, w, resize_to) if resize_to else (h, w)
    if zoom:
        P.scale[0] = 1.15
        P.offset[0] = augment.affine_offset_of(rw, rh, 1.15)
    P.flip[0] = bool(flip)
    desc, geom = augment.descriptors([(h, w)], P, size, resize_to)
    f = desc[0]
    assert (f.rh, f.rw) == (rh, rw)
    lb = augment.labels([[row]], [np.array([700., 0, 100, 0, 700, 30, 0, 0, 1])], [(h, w)], P, size, resize_to)
    assert lb.rows[0, 1] == 0
    canvas = ref.canvas(src, size[0], size[1], f.x0, f.y0, f.rw, f.rh, (f.ax, f.bx, f.ay, f.by))
    wgt = canvas[f.y0:f.y0 + f.rh, f.x0:f.x0 + f.rw, 0].astype(np.float64) - 100
    assert wgt.min() >= 0 and wgt.sum() > 0
    ys, xs = np.mgrid[f.y0:f.y0 + f.rh, f.x0:f.x0 + f.rw]
    px, py = (wgt * xs).sum() / wgt.sum(), (wgt * ys).sum() / wgt.sum()
    bx, by = (lb.rows[0, 3] + lb.rows[0, 5]) / 2, (lb.rows[0, 4] + lb.rows[0, 6]) / 2
    print('centroid (%.3f, %.3f) label centre (%.3f, %.3f)' % (px, py, bx, by))
    assert abs(px - bx) <= 1.5 and abs(py - by) <= 1.5


# ------------------------------------------------------------------------------------------------ refusals
def good_frame(**kw):
    f = _lib.AugmentFrameC(h=5, w=4, x0=2, y0=1, rw=9, rh=7, alpha_q=65536, beta_q=0, sigma_q=0, ax=32 * 65536, bx=32768, ay=32 * 65536, by=32768)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_every_refusal_fires_and_names_the_frame(lib):
    """Through rtm3d_frames_augment_check AND through the launcher, which refuses before its first memset or launch: nothing here
    touches a device, the pointers are never dereferenced."""
    fake = 0x10000
    B, bad_at = 3, 1

    def call(frames=None, src=None, out=fake, mode=0, H=32, W=32, border=0, table=fake, lut=fake, lut16=fake, sums=fake, n=None):
        frames = frames if frames is not None else [good_frame() for _ in range(B)]
        arr = (_lib.AugmentFrameC * len(frames))(*frames)
        src = src if src is not None else [0x20000 + 0x1000 * i for i in range(len(frames))]
        ptrs = (ctypes.c_void_p * len(src))(*src)
        n = len(frames) if n is None else n
        rc1 = lib.rtm3d_frames_augment_check(n, ptrs, arr, out, mode, H, W, border, table, lut, lut16, sums)
        m1 = lib.rtm3d_last_error().decode()
        if rc1:                                                          # (an accepted call would launch: not here)
            rc2 = lib.rtm3d_frames_augment(None, n, ptrs, arr, out, mode, H, W, border, table, lut, lut16, sums)
            assert rc2 != 0 and lib.rtm3d_last_error().decode() == m1
        return rc1, m1

    assert call()[0] == 0 and call(mode=1, border=3)[0] == 0 and call(mode=2, lut=None, lut16=None)[0] == 0
    assert call(frames=[good_frame(alpha_q=1 << 24, beta_q=(1 << 31) - (1 << 24), sigma_q=65535, ax=(1 << 40) - 1, ay=-(1 << 40) + 1)] * 2)[0] == 0

    def one_bad(**kw):
        return [good_frame(**(kw if i == bad_at else {})) for i in range(B)]

    per_frame = [
        (dict(h=0), 'a side must lie in 1..16384'), (dict(w=16385), 'a side must lie in 1..16384'), (dict(h=-3), 'a side'),
        (dict(x0=24), 'leaves the 32 x 32 canvas'), (dict(y0=26), 'leaves'), (dict(x0=-1), 'leaves'), (dict(rw=0), 'leaves'), (dict(rh=33, y0=0), 'leaves'),
        (dict(sigma_q=-1), 'sigma_q -1'), (dict(sigma_q=65536), 'sigma_q 65536'),
        (dict(alpha_q=(1 << 24) + 1), 'alpha_q'), (dict(alpha_q=-(1 << 24) - 1), 'alpha_q'),
        (dict(beta_q=(1 << 31) - (1 << 24) + 1), 'beta_q'), (dict(beta_q=-(1 << 31) + (1 << 24) - 1), 'beta_q'),
        (dict(ax=1 << 40), '2^40'), (dict(ax=-(1 << 40)), '2^40'), (dict(ay=1 << 40), '2^40'), (dict(ay=-(1 << 62)), '2^40'),
        (dict(bx=1 << 56), '2^56'), (dict(by=-(1 << 56)), '2^56'), (dict(reserved=1), 'reserved'),
    ]
    for kw, word in per_frame:
        rc, msg = call(frames=one_bad(**kw))
        assert rc != 0 and msg.startswith('frames_augment: frame %d' % bad_at) and word in msg, (kw, msg)
    rc, msg = call(src=[0x20000, 0, 0x22000])
    assert rc != 0 and 'frame 1: the source is a NULL pointer' in msg
    # a packed destination over a source: frame 2's 5 x 4 x 3 bytes begin inside the 3 * 32 * 32 * 3 destination bytes
    rc, msg = call(mode=2, out=0x30000, src=[0x20000, 0x21000, 0x30000 + 3 * 32 * 32 * 3 - 1])
    assert rc != 0 and 'frame 2: the destination overlaps this source' in msg
    assert call(mode=2, out=0x30000, src=[0x20000, 0x21000, 0x30000 + 3 * 32 * 32 * 3])[0] == 0        # ... and just behind them
    assert call(mode=2, out=0x30000, src=[0x20000, 0x21000, 0x30000 - 60])[0] == 0                     # ... and just in front
    assert call(mode=2, out=0x30000, src=[0x20000, 0x21000, 0x30000 - 59])[0] != 0
    assert call(mode=0, out=0x30000, src=[0x20000, 0x21000, 0x30000])[0] == 0                          # (the check is mode 2's: fp32 cannot alias bytes)
    whole = [(dict(out=None), 'destination is a NULL'), (dict(table=None), 'noise table is a NULL'), (dict(sums=None), 'channel sums are a NULL'),
             (dict(lut=None), 'fp32 normalisation table is a NULL'), (dict(mode=1, lut16=None), 'fp16 normalisation table is a NULL'),
             (dict(mode=3), 'out_mode 3'), (dict(mode=-1), 'out_mode -1'), (dict(n=0), 'B = 0'), (dict(H=0), 'canvas'), (dict(W=16385), 'canvas'),
             (dict(mode=1, border=-1), 'out_border -1'), (dict(out=fake + 2), 'multiple of 4'), (dict(mode=1, out=fake + 4), 'multiple of 8'),
             (dict(table=fake + 1), 'odd'), (dict(sums=fake + 4), 'multiple of 8')]
    for kw, word in whole:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith('frames_augment') and word in msg, (kw, msg)
    assert call(mode=2, out=fake + 3, lut=None, lut16=None)[0] == 0 and call(mode=1, lut=None)[0] == 0 and call(mode=0, lut16=None)[0] == 0
    assert lib.rtm3d_frames_augment_check(1, None, None, fake, 0, 32, 32, 0, fake, fake, fake, fake) != 0
    # the facade refuses what it can see before the library does
    P = augment.AugmentParams.identity(1)
    P.alpha[0] = 300.0
    with pytest.raises(ValueError):
        augment.descriptors([(5, 4)], P, (32, 32))
    with pytest.raises(ValueError):
        augment.descriptors([(50, 4)], augment.AugmentParams.identity(1), (32, 32))                     # does not fit
    with pytest.raises(ValueError):
        augment.AugmentParams(1, 0, 0, 0, 0.0, (0, 0), 0, (0, 0, 0))


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize('name', list(ac.REGIMES))
def test_plan_regimes(lib, name):
    mode, H, W, border, rects = ac.REGIMES[name]
    arr = (_lib.AugmentFrameC * len(rects))(*[good_frame(x0=x0, y0=y0, rw=rw, rh=rh) for x0, y0, rw, rh in rects])
    got = augment.plan(arr, (H, W), mode, border)
    want = ac.expected_plan(name)
    assert [{k: getattr(p, k) for k, _ in _lib.AugmentPlan._fields_} for p in got] == want
    for p in got:                                                       # every interior run has a thread, every grid row a frame
        assert p.grid_x * p.threads >= p.runs > (p.grid_x - 1) * p.threads and p.grid_y == p.count <= ac.CHUNK


def test_plan_table_and_refusals(lib):
    plans = {n: ac.expected_plan(n) for n in ac.REGIMES}
    assert {p['shift'] for ps in plans.values() for p in ps} == {0, 1, 2, 3}
    assert [len(plans[n]) for n in ('chunk_31', 'chunk_32', 'chunk_33', 'chunk_65_last_full')] == [1, 1, 2, 3]
    assert plans['one_full_canvas'][0]['border_grid_x'] == 0 and plans['chunk_65_last_full'][2]['border_grid_x'] == 0
    assert plans['nhwc4_border_3'][0]['border_grid_x'] > 0 and plans['many_border_blocks'][0]['border_grid_x'] == ac.BORDER_GRID
    assert plans['kitti'][0]['runs'] == 375 * 312 and plans['single_pixel'][0]['runs'] == 1
    out = (_lib.AugmentPlan * 1)()
    arr = (_lib.AugmentFrameC * 2)(good_frame(), good_frame(x0=30))
    assert lib.rtm3d_frames_augment_plan(2, arr, 0, 32, 32, 0, out) != 0 and 'frames_augment_plan: frame 1' in lib.rtm3d_last_error().decode()
    assert lib.rtm3d_frames_augment_plan(1, arr, 0, 32, 32, 0, None) != 0 and lib.rtm3d_frames_augment_plan(0, arr, 0, 32, 32, 0, out) != 0
    assert lib.rtm3d_frames_augment_plan(1, arr, 5, 32, 32, 0, out) != 0 and lib.rtm3d_frames_augment_plan(1, None, 0, 32, 32, 0, out) != 0


# ------------------------------------------------------------------------------------------------ library and binding
def test_header_library_and_binding_agree():
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert re.search(r'#define RTM3D_ABI_VERSION 9\b', hdr) and _lib.ABI_VERSION == 9
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert 'typedef struct rtm3d_augment_frame' in hdr and 'typedef struct rtm3d_augment_plan' in hdr and 'training augmentation' in hdr
    assert _lib.load().rtm3d_abi_version() == 9
    mk = open(os.path.join(REPO, 'rtm3d_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\baugment\.hip\b', mk, re.M)
    # one copy of Philox, used by the kernel and by nothing else
    csrc = os.path.join(REPO, 'rtm3d_amd', 'csrc')
    users = sorted(f for f in os.listdir(csrc) if f.endswith(('.hip', '.h', '.cpp')) and 'philox' in open(os.path.join(csrc, f)).read().lower())
    assert users == ['augment.hip', 'philox.h'], users


def test_structs_have_the_c_layout(tmp_path):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no C compiler'
    fields = ['h', 'rh', 'alpha_q', 'sigma_q', 'seed_hi', 'fill', 'reserved', 'ax', 'by']
    pfields = [k for k, _ in _lib.AugmentPlan._fields_]
    src = ('#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu", sizeof(rtm3d_augment_frame), '
           'sizeof(rtm3d_augment_plan));\n' % REPO
           + ''.join('printf(" %%zu", offsetof(rtm3d_augment_frame, %s));\n' % f for f in fields)
           + ''.join('printf(" %%zu", offsetof(rtm3d_augment_plan, %s));\n' % f for f in pfields) + 'return 0;}')
    exe = str(tmp_path / 'sizeof_augment')
    subprocess.run([cc, '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    F, P = _lib.AugmentFrameC, _lib.AugmentPlan
    assert got == [ctypes.sizeof(F), ctypes.sizeof(P)] + [getattr(F, f).offset for f in fields] + [getattr(P, f).offset for f in pfields]
    assert ctypes.sizeof(F) == 80 and 32 * (8 + ctypes.sizeof(F)) + 128 <= 4096          # a chunk's descriptors fit the kernel arguments
