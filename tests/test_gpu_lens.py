"""GPU: rtm3d_frames_remap and rtm3d_lens_map_build (csrc/lens.hip) against the numpy restatement tests/lens_ref.py over the
case table of tests/lens_cases.py - the remap BYTE FOR BYTE with 64 guard bytes around every destination, the Brown / rational
builder entry for entry, the fisheye builder entry for entry away from rounding boundaries; the refusals through the
launchers; Engine.detect_frames_lens against Engine.detect_frames / detect_frames_src; the C example."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                            # noqa: E402
from rtm3d_amd import _lib, weights, engine, lens, pixfmt   # noqa: E402
from tests import lens_cases as cases                       # noqa: E402
from tests import lens_ref as ref                           # noqa: E402
from tests import pixfmt_ref                                # noqa: E402
from tests.util import load_golden                          # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_BYTE = 64, 0xA5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------------------------------- helpers
def at_offset(arr, dev, offset):
    """A numpy uint8 array on the device, `offset` bytes into an allocation of its own (torch allocations are 512-byte
    aligned, so the offset is the address modulo 4)."""
    flat = np.ascontiguousarray(arr).reshape(-1)
    buf = torch.empty(offset + flat.size, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[offset:].copy_(torch.from_numpy(flat))
    return buf[offset:].view(arr.shape)


class Guarded(object):
    """Destinations with GUARD bytes of 0xA5 before and after each, `offset` bytes into their allocations."""

    def __init__(self, sizes, dev, offset=0):
        self.bufs, self.out = [], []
        for ho, wo in sizes:
            n = ho * wo * 3
            buf = torch.full((offset + GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
            self.bufs.append((buf, offset + GUARD, n))
            self.out.append(buf[offset + GUARD:offset + GUARD + n].view(ho, wo, 3))

    def guards_intact(self):
        return all(bool((b[:at] == GUARD_BYTE).all()) and bool((b[at + n:] == GUARD_BYTE).all()) for b, at, n in self.bufs)

    def untouched(self):
        return all(bool((b == GUARD_BYTE).all()) for b, _, _ in self.bufs)


def run_and_compare(jobs, dev, fill=(0, 0, 0), src_offset=0, dst_offset=0):
    """jobs = [(frame (h, w, 3) uint8, map (ho, wo, 2) int32)] in ONE rtm3d_frames_remap call (chunks of 32 inside); jobs that
    hold the same map array share one device map.  Every frame against the reference."""
    shared = {}
    for _, m in jobs:
        if id(m) not in shared:
            shared[id(m)] = lens.LensMap.from_array(m, device=dev)
    g = Guarded([m.shape[:2] for _, m in jobs], dev, dst_offset)
    got = lens.remap([at_offset(f, dev, src_offset) for f, _ in jobs], [shared[id(m)] for _, m in jobs], fill, out=g.out)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, g.out))
    for i, (f, m) in enumerate(jobs):
        want = ref.remap(f, m, fill)
        assert torch.equal(got[i].cpu(), torch.from_numpy(want)), (i, f.shape, m.shape, fill, src_offset, dst_offset)
    assert g.guards_intact()
    return got


# ---------------------------------------------------------------------------------------------------- 1. maps x sizes
@pytest.mark.parametrize('kind', cases.MAP_KINDS)
def test_map_kinds_over_every_size(dev, kind):
    """Every destination size of the table against every source size; each map serves a frame of random bytes, one of zeros and
    one of 255s.  Zero fill, and a fill of three different bytes."""
    rng = np.random.Generator(np.random.PCG64(10 + cases.MAP_KINDS.index(kind)))
    jobs, states = [], set()
    for h, w in cases.SRC_SIZES:
        frames = cases.frames_for(h, w, rng)
        for ho, wo in cases.DST_SIZES:
            m = cases.make_map(kind, h, w, ho, wo, rng)
            jobs += [(f, m) for f in frames]
            if (h, w) == (5, 4) and (ho, wo) == (48, 64):
                states = cases.axis_states(m, h, w)
                if kind == 'fractions':
                    assert len({(int(a) & 31, int(b) & 31) for a, b in m.reshape(-1, 2)}) == 1024        # every (ax, ay) pair
    if kind == 'random':       # every border combination: each axis has (first, second) sample inside = 00 01 10 11
        assert states == {(a, b) for a in range(4) for b in range(4)}, states
        every = set().union(*[set(np.unique(ref.sample_pattern(m, *f.shape[:2])).tolist()) for f, m in jobs])
        assert every == {0, 1, 2, 3, 4, 5, 8, 10, 12, 15}, every                 # ... which are the ten patterns four samples can show
    if kind == 'special':
        assert states >= {(0, 0), (1, 1), (2, 2)}, states                 # the special values alone give these
    run_and_compare(jobs, dev)
    run_and_compare(jobs[:3 * len(cases.DST_SIZES)], dev, fill=(7, 200, 255))


# ---------------------------------------------------------------------------------------------------- 2. addresses
def test_address_sweep(dev):
    """Source and destination bases at byte offsets 0..3 into their allocations: the same bytes come out wherever they lie.
    (3 x 8 and 3 x 7: rows of two whole runs, which keep the base's alignment, and rows that end in a partial run - every
    branch of the run store, csrc/rgb_runs.h, at every address modulo 4.)"""
    rng = np.random.Generator(np.random.PCG64(20))
    jobs = []
    for (h, w), dsts in (((37, 53), [(48, 64), (33, 65), (3, 5), (1, 7)]), ((5, 4), [(2, 9), (3, 4), (1, 1), (3, 8), (3, 7)])):
        f = cases.frames_for(h, w, rng)[0]
        jobs += [(f, cases.make_map(kind, h, w, ho, wo, rng)) for ho, wo in dsts for kind in ('random', 'fractions')]
    first = None
    for so in range(4):
        for do in range(4):
            got = [t.cpu() for t in run_and_compare(jobs, dev, (1, 2, 3), so, do)]
            first = first or got
            assert all(torch.equal(a, b) for a, b in zip(first, got))


def test_map_at_a_dword_address_and_odd_widths(dev):
    """A map is 4-byte aligned, no more: the same map 4, 8 and 12 bytes into its allocation, for even and odd widths (the rows
    of an odd width alternate between 16- and 8-byte aligned runs)."""
    rng = np.random.Generator(np.random.PCG64(21))
    h, w = 37, 53
    f = cases.frames_for(h, w, rng)[0]
    src = torch.from_numpy(f).to(dev)
    for ho, wo in ((48, 64), (33, 65), (7, 6), (2, 9)):
        m = cases.make_map('random', h, w, ho, wo, rng)
        want = torch.from_numpy(ref.remap(f, m, (4, 5, 6)))
        for skip in (0, 1, 2, 3):
            buf = torch.zeros(skip + m.size, dtype=torch.int32, device=dev)
            buf[skip:].copy_(torch.from_numpy(m.reshape(-1)))
            lm = lens.LensMap(buf[skip:].view(ho, wo, 2))
            assert lm.tensor.data_ptr() % 16 == 4 * skip
            g = Guarded([(ho, wo)], dev)
            lens.remap([src], [lm], (4, 5, 6), out=g.out)
            torch.cuda.synchronize()
            assert torch.equal(g.out[0].cpu(), want) and g.guards_intact(), (ho, wo, skip)


# ---------------------------------------------------------------------------------------------------- 3. batches
def test_batch_of_33_mixed_frames(dev):
    """33 frames make two launches; sources, destinations and map kinds are mixed within the call, two frames share one map;
    every frame as on its own."""
    rng = np.random.Generator(np.random.PCG64(30))
    jobs = []
    for i in range(cases.CHUNK + 1):
        h, w = cases.SRC_SIZES[i % len(cases.SRC_SIZES)]
        ho, wo = cases.DST_SIZES[(i * 5 + 2) % len(cases.DST_SIZES)]
        jobs.append((cases.frames_for(h, w, rng)[0], cases.make_map(cases.MAP_KINDS[(i * 3) % 4], h, w, ho, wo, rng)))
    jobs[31] = (cases.frames_for(*jobs[4][0].shape[:2], rng)[0], jobs[4][1])          # frames 4 and 31 share a map, as do 32 and 0:
    jobs[32] = (cases.frames_for(*jobs[0][0].shape[:2], rng)[0], jobs[0][1])          # across the chunks too
    assert len({m.shape for _, m in jobs}) > 8 and jobs[31][1] is jobs[4][1]
    many = [t.cpu() for t in run_and_compare(jobs, dev, (3, 2, 1))]
    for i in (0, 4, 31, 32):
        assert torch.equal(run_and_compare([jobs[i]], dev, (3, 2, 1))[0].cpu(), many[i])


# ---------------------------------------------------------------------------------------------------- 4. the builder
def build_on_device(case, dev):
    _, kind, K, dist, Kr, R, (ho, wo) = case
    model = lens.LensModel(kind, K, dist, cases.LENS_SIZE)
    # build_maps takes the rotation in OpenCV's sense: the transpose of the header's R
    lm = lens.build_maps([model], K_rect=Kr, R=np.asarray(R, np.float64).reshape(3, 3).T, out_size=(ho, wo), device=dev)[0]
    torch.cuda.synchronize()
    assert lm.size == (ho, wo) and lm.K_rect.tolist() == [float(v) for v in Kr]
    return lm.tensor.cpu().numpy()


@pytest.mark.parametrize('case', cases.BROWN_CASES, ids=[c[0] for c in cases.BROWN_CASES])
def test_builder_brown_and_rational_exact(dev, case):
    got, want = build_on_device(case, dev), cases.reference_map(case)
    outside = want[..., 0] == ref.OUTSIDE
    print('%s: %d of %d entries outside' % (case[0], outside.sum(), outside.size))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if case[0] == 'tilted':
        assert 0.05 < outside.mean() < 0.95
    else:
        assert not outside.any()


@pytest.mark.parametrize('case', cases.FISHEYE_CASES, ids=[c[0] for c in cases.FISHEYE_CASES])
def test_builder_fisheye(dev, case):
    """atan and sqrt are the device library's: equal wherever the reference's U*32 + 0.5 (V*32 + 0.5) is farther than 1e-6 from an
    integer, within 1 elsewhere (tests/test_lens_cpu.py caps those entries at 0.1 % of the case)."""
    _, kind, K, dist, Kr, R, (ho, wo) = case
    got, want = build_on_device(case, dev).astype(np.int64), cases.reference_map(case).astype(np.int64)
    near = ref.near_half(kind, K, dist, Kr, R, ho, wo)
    diff = np.abs(got - want)
    print('%s: %d entries differ, %d near a boundary, max difference %d' % (case[0], (diff > 0).sum(), near.sum(), diff.max()))
    assert near.mean() <= 0.001
    assert (diff[~near] == 0).all(), np.argwhere((diff > 0) & ~near)[:5]
    assert (diff[near] <= 1).all()


def test_builder_batches_and_shared_launch(dev):
    """Nine maps of mixed kinds and sizes in one call (two launches of at most 8): each as built on its own."""
    all_cases = (cases.BROWN_CASES + cases.FISHEYE_CASES[:1]) * 2
    all_cases = all_cases[:9]
    models = [lens.LensModel(c[1], c[2], c[3], cases.LENS_SIZE) for c in all_cases]
    maps = lens.build_maps(models, K_rect=[c[4] for c in all_cases], R=[np.asarray(c[5], np.float64).reshape(3, 3).T for c in all_cases],
                           out_size=[c[6] for c in all_cases], device=dev)
    torch.cuda.synchronize()
    for c, m in zip(all_cases, maps):
        assert np.array_equal(m.tensor.cpu().numpy(), build_on_device(c, dev)), c[0]
    # the defaults: the lens's own K and size, no rotation
    c = cases.BROWN_CASES[2]
    m = lens.build_maps([lens.LensModel(c[1], c[2], c[3], cases.LENS_SIZE)], device=dev)[0]
    assert m.size == cases.LENS_SIZE and np.array_equal(m.tensor.cpu().numpy(), ref.build_map(c[1], c[2], c[3], c[2], cases.EYE, *cases.LENS_SIZE))


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_destination_untouched(dev):
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(40))
    shapes = [((6, 10), (4, 4)), ((5, 7), (8, 3)), ((3, 3), (3, 3))]
    frames = [torch.from_numpy(cases.frames_for(h, w, rng)[0]).to(dev) for (h, w), _ in shapes]
    np_maps = [cases.make_map('random', h, w, ho, wo, rng) for (h, w), (ho, wo) in shapes]
    maps = [lens.LensMap.from_array(m, device=dev) for m in np_maps]
    g = Guarded([d for _, d in shapes], dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    fill = (ctypes.c_uint8 * 3)(0, 0, 0)

    def args():
        return [(ctypes.c_void_p * 3)(*[f.data_ptr() for f in frames]), (ctypes.c_int * 6)(*[v for (h, w), _ in shapes for v in (h, w)]),
                lens.c_maps(maps), (ctypes.c_void_p * 3)(*[o.data_ptr() for o in g.out]), fill]

    def refused(a, word):
        assert lib.rtm3d_frames_remap(stream, 3, *a) != 0, word
        assert word in lib.rtm3d_last_error().decode(), (lib.rtm3d_last_error().decode(), word)
        torch.cuda.synchronize()
        assert g.untouched(), word

    # the LAST frame is the bad one: nothing of the good ones in front of it may have been launched
    a = args(); a[0][2] = None
    refused(a, 'frame 2: the source is a NULL')
    a = args(); a[3][2] = None
    refused(a, 'frame 2: the destination is a NULL')
    a = args(); a[2][2].d_map = None
    refused(a, 'frame 2: the map is a NULL')
    a = args(); a[2][2].d_map = a[2][2].d_map + 2
    refused(a, 'frame 2: the map\'s address is no multiple of 4')
    a = args(); a[2][2].reserved = 3
    refused(a, 'frame 2: reserved = 3')
    a = args(); a[2][2].wo = 16385
    refused(a, 'frame 2: a map of 3 x 16385')
    a = args(); a[1][5] = 0
    refused(a, 'frame 2 is 3 x 0')
    a = args(); a[0][2] = a[3][2] + 5
    refused(a, 'frame 2: the destination overlaps its source')
    a = args(); a[4] = None
    refused(a, 'null pointer')
    # Python: destinations of the wrong shape, frames that are no frames, a fill that is no byte triple, counts that differ
    with pytest.raises(ValueError, match='destination'):
        lens.remap(frames, maps, out=[o[:, :-1] for o in g.out])
    with pytest.raises(ValueError, match='uint8'):
        lens.remap([f.float() for f in frames], maps, out=g.out)
    with pytest.raises(ValueError, match='three bytes'):
        lens.remap(frames, maps, (0, 0), out=g.out)
    with pytest.raises(ValueError, match='2 maps for 3 frames'):
        lens.remap(frames, maps[:2], out=g.out)
    with pytest.raises(ValueError, match='int32'):
        lens.LensMap(maps[0].tensor.long())
    with pytest.raises(ValueError, match='int32 values'):
        lens.LensMap.from_array(np_maps[0].astype(np.float32), device=dev)
    assert g.untouched()
    # the builder: a refused call leaves its maps untouched
    t = torch.full((2, 4, 5, 2), 77, dtype=torch.int32, device=dev)
    m, r = (_lib.LensModelC * 2)(), (_lib.LensRectC * 2)()
    for i in range(2):
        m[i] = lens.LensModel.brown(cases.K_LENS, [0.1], (4, 5)).c_struct()
        r[i] = _lib.LensRectC(4, 5, (ctypes.c_double * 9)(*cases.K_LENS), (ctypes.c_double * 9)(*cases.EYE))
    m[1].kind = 5
    ptrs = (ctypes.c_void_p * 2)(t[0].data_ptr(), t[1].data_ptr())
    assert lib.rtm3d_lens_map_build(stream, 2, m, r, ptrs) != 0 and 'map 1: unknown lens kind 5' in lib.rtm3d_last_error().decode()
    torch.cuda.synchronize()
    assert bool((t == 77).all())
    with pytest.raises(RuntimeError, match='fisheye lens has four'):
        bad = lens.LensModel.fisheye(cases.K_LENS, [0.1], (4, 5)); bad.dist[5] = 1.0
        lens.build_maps([bad], device=dev)
    # and the same remap, unbroken, does write
    lens.remap(frames, maps, out=g.out)
    torch.cuda.synchronize()
    assert g.guards_intact() and all(torch.equal(o.cpu(), torch.from_numpy(ref.remap(f.cpu().numpy(), m))) for o, f, m in zip(g.out, frames, np_maps))


# ---------------------------------------------------------------------------------------------------- 6. the engine
def identity_map(h, w, dev, K=None):
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return lens.LensMap.from_array(np.stack([32 * u, 32 * v], -1), K_rect=K, device=dev)


@pytest.fixture(scope='module')
def small(dev, tmp_path_factory):
    """The small synthetic engine of tests/test_gpu_pixfmt.py (128 x 256 canvas, batch 2), its ragged frames as RGB arrays and as
    NV12 surfaces at a pitch of 256.  (The acceptance bar of the 3D solver is raised as there: the fixture's weights are
    random, and the KITTI rows are to hold something.)"""
    from rtm3d_amd import model_utils
    from tests.test_gpu_frames import uint8_frames
    from tests.test_gpu_pixfmt import rgb_to_nv12
    g = load_golden('e2e_dla34_small.npz')
    bb = str(g['backbone'])
    B, H, W = [int(v) for v in g['shape']]
    cfg = rtm3d_amd.kitti_config(bb)
    m = rtm3d_amd.create_model(cfg).to('cuda:0').eval()
    m.load_state_dict(weights.synth_state_dict(bb, int(g['seed']), str(g['style']), heat_bias=float(g['heat_bias']),
                                               heat_gain=float(g['heat_gain'])))
    path = str(tmp_path_factory.mktemp('lens') / 'small.rtm3d')
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(model_utils, 'FUN_ACCEPT', 1e6)
        mp.setattr(engine, 'FUN_ACCEPT', 1e6)
        m.save_engine(path, B, H, W)
    full = uint8_frames(weights.synth_images(B, H, W, seed=int(g['img_seed'])), cfg.DATASET.MEAN, cfg.DATASET.STD)
    frames = [full[0], np.ascontiguousarray(full[1][9:110, 20:243])]              # the canvas itself, and 101 x 223 (odd both ways)
    K = np.tile(g['K'], (B, 1)) * np.array([[1.0], [1.03]])
    K[:, 6:] = (0, 0, 1)
    nv12 = []
    for f in frames:
        h, w = f.shape[:2]
        y, c = rgb_to_nv12(f)
        surf = np.full((h + c.shape[0], 256), 0x5A, np.uint8)
        surf[:h, :w] = y
        surf[h:, :c.shape[1]] = c
        nv12.append({'format': 'nv12', 'h': h, 'w': w, 'planes': [surf.reshape(-1), surf.reshape(-1)[h * 256:]], 'pitches': [256, 256],
                     'matrix': 'bt601', 'range': 'limited', 'file': y.tobytes() + c.tobytes()})
    eng = engine.Engine(path, dev)
    eng.set_frame_params(cfg.DATASET.MEAN, cfg.DATASET.STD, None)
    yield {'engine': eng, 'path': path, 'frames': frames, 'nv12': nv12, 'K': K, 'mean': cfg.DATASET.MEAN, 'std': cfg.DATASET.STD, 'B': B}
    eng.close()


def upload_nv12(s, dev):
    planes = [torch.from_numpy(p.copy()).to(dev) for p in s['planes']]
    return pixfmt.FrameSource(planes, 'nv12', size=(s['h'], s['w']), pitches=s['pitches'], matrix=s['matrix'], range=s['range'])


def test_engine_identity_map_equals_detect_frames(dev, small):
    eng, K = small['engine'], small['K']
    imgs = [torch.from_numpy(f).to(dev) for f in small['frames']]
    want_rec, want_rows = eng.detect_frames(imgs, K, kitti=True)
    want_rec, want_rows = want_rec.clone(), want_rows.clone()
    assert int((want_rec[..., 31] >= 1).sum()) > 0 and int((want_rows[..., 14] == 2).sum()) > 0
    maps = [identity_map(*f.shape[:2], dev, K=k) for f, k in zip(small['frames'], K)]
    for _ in range(2):                                                       # the second call replays the captured graph
        rec, rows, rect = eng.detect_frames_lens(imgs, maps, kitti=True)
        torch.cuda.synchronize()
        assert torch.equal(rec, want_rec) and torch.equal(rows, want_rows)
        assert all(torch.equal(r, i) for r, i in zip(rect, imgs)) and rect is eng.last_rect
    # K_rect= overrides the maps' own; the caller's buffers are used when given
    mine = [torch.empty_like(i) for i in imgs]
    rec, rect = eng.detect_frames_lens(imgs, [identity_map(*f.shape[:2], dev) for f in small['frames']], K_rect=K, rect=mine)
    assert torch.equal(rec, want_rec) and rect[0] is mine[0] and all(torch.equal(r, i) for r, i in zip(mine, imgs))
    with pytest.raises(ValueError, match='needs K_rect'):
        eng.detect_frames_lens(imgs, [identity_map(*f.shape[:2], dev) for f in small['frames']])
    with pytest.raises(ValueError, match='batches of 2'):
        eng.detect_frames_lens(imgs[:1], maps[:1])
    # a map the remap refuses, and a rectified frame the canvas cannot hold: by name, before anything is launched
    mine[0].fill_(7)
    cm = lens.c_maps(maps)
    cm[1].reserved = 1
    pptr = (ctypes.c_void_p * 2)(*[i.data_ptr() for i in imgs])
    rptr = (ctypes.c_void_p * 2)(*[p.data_ptr() for p in mine])
    hw = (ctypes.c_int * 4)(*[v for i in imgs for v in i.shape[:2]])
    args = (ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), None, pptr, hw, 0, cm, rptr, (ctypes.c_uint8 * 3)(0, 0, 0),
            ctypes.c_void_p(torch.as_tensor(K, device=dev).data_ptr()), ctypes.c_void_p(rec.data_ptr()), None,
            ctypes.c_void_p(eng.frames_workspace.data_ptr()))
    assert eng.lib.rtm3d_engine_detect_frames_lens(eng.ctx, *args) != 0 and 'frame 1: reserved = 1' in eng.lib.rtm3d_last_error().decode()
    with pytest.raises(RuntimeError, match=r'frame 1 \(129x8'):
        eng.detect_frames_lens(imgs, [maps[0], identity_map(129, 8, dev, K=K[1])], rect=[mine[0], torch.empty(129, 8, 3, dtype=torch.uint8, device=dev)])
    torch.cuda.synchronize()
    assert bool((mine[0] == 7).all())


def test_engine_nv12_sources_identity_map_equals_detect_frames_src(dev, small):
    eng, K = small['engine'], small['K']
    srcs = [upload_nv12(s, dev) for s in small['nv12']]
    want_rec, want_rows = eng.detect_frames_src(srcs, K, kitti=True)
    want_rec, want_rows, want_packed = want_rec.clone(), want_rows.clone(), [p.clone() for p in eng.last_packed]
    assert int((want_rec[..., 31] >= 1).sum()) > 0 and int((want_rows[..., 14] == 2).sum()) > 0
    maps = [identity_map(s['h'], s['w'], dev, K=k) for s, k in zip(small['nv12'], K)]
    rec, rows, rect = eng.detect_frames_lens(srcs, maps, kitti=True)
    torch.cuda.synchronize()
    assert torch.equal(rec, want_rec) and torch.equal(rows, want_rows)
    assert all(torch.equal(r, p) for r, p in zip(rect, want_packed)) and all(torch.equal(q, p) for q, p in zip(eng.last_packed, want_packed))
    assert all(torch.equal(p.cpu(), torch.from_numpy(pixfmt_ref.convert(s))) for p, s in zip(want_packed, small['nv12']))
    # the BGR order reaches the conversion
    _, rect = eng.detect_frames_lens(srcs, maps, order='bgr')
    assert all(torch.equal(r, p.flip(-1)) for r, p in zip(rect, want_packed))


def test_engine_brown_map(dev, small):
    """A real map: the rectified frames are the remap of the converted frames, the records those of detect_frames on them."""
    eng, K = small['engine'], small['K']
    srcs = [upload_nv12(s, dev) for s in small['nv12']]
    models = [lens.LensModel.brown(k, [-0.18, 0.04, 1e-3, -2e-3, -0.006], (s['h'], s['w'])) for s, k in zip(small['nv12'], K)]
    Kr = K.copy()
    Kr[1, [0, 4]] *= 0.9                                                     # frame 1: a shorter rectified focal length
    maps = lens.build_maps(models, K_rect=list(Kr), out_size=[(small['nv12'][0]['h'], small['nv12'][0]['w']), (96, 200)], device=dev)
    for m, mod, k in zip(maps, models, Kr):
        assert np.array_equal(m.tensor.cpu().numpy(), ref.build_map('brown', mod.K, mod.dist, k, cases.EYE, *m.size))
        assert int((m.tensor[..., 0] == ref.OUTSIDE).sum()) == 0
    rec, rows, rect = eng.detect_frames_lens(srcs, maps, kitti=True, fill=(5, 6, 7))
    rec, rows = rec.clone(), rows.clone()
    torch.cuda.synchronize()
    conv = pixfmt.convert(srcs)
    want_rect = lens.remap(conv, maps, (5, 6, 7))
    assert all(torch.equal(a, b) for a, b in zip(rect, want_rect)) and [tuple(r.shape) for r in rect] == [m.size + (3,) for m in maps]
    assert all(torch.equal(r.cpu(), torch.from_numpy(ref.remap(c.cpu().numpy(), m.tensor.cpu().numpy(), (5, 6, 7))))
               for r, c, m in zip(rect, conv, maps))
    assert not torch.equal(rect[0], conv[0])                                 # the lens does bend the frame
    want_rec, want_rows = eng.detect_frames(want_rect, Kr, kitti=True)
    print('Brown map: %d live slots, %d kept' % (int((want_rec[..., 31] >= 1).sum()), int((want_rows[..., 14] == 2).sum())))
    assert torch.equal(rec, want_rec) and torch.equal(rows, want_rows) and int((want_rec[..., 31] >= 1).sum()) > 0


def test_c_example_prints_the_rows_of_the_python_path(dev, small, tmp_path):
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_detect_lens')
    if not os.path.exists(exe):
        subprocess.run(['make', '-C', os.path.join(REPO, 'rtm3d_amd', 'csrc'), 'example'], check=True)
    eng, K, B = small['engine'], small['K'], small['B']
    s = small['nv12'][0]
    fx, fy, cx, cy = 0.97 * K[0, 0], 0.97 * K[0, 4], K[0, 2] + 1.5, K[0, 5] - 0.75
    dist = [-0.18, 0.04, 1e-3, -2e-3, -0.006]
    model = lens.LensModel.brown([fx, 0, cx, 0, fy, cy, 0, 0, 1], dist, (s['h'], s['w']))
    lm = lens.build_maps([model], K_rect=K[0], device=dev)[0]                # the example: one map from frame 0's K, shared
    src = upload_nv12(s, dev)
    rec, rows, rect = eng.detect_frames_lens([src] * B, [lm] * B, K_rect=K, kitti=True)
    rec, rows, total = rec.cpu().numpy(), rows.cpu().numpy(), int(rect[0].long().sum())
    frame, params = str(tmp_path / 'frame.nv12'), str(tmp_path / 'params.bin')
    with open(frame, 'wb') as f:
        f.write(s['file'])
    with open(params, 'wb') as f:
        f.write(K.astype('<f8').tobytes() + np.asarray(small['mean'], '<f4').tobytes() + np.asarray(small['std'], '<f4').tobytes())
        f.write(struct.pack('<4i', 0, 0, 0, 0))
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH',)}
    r = subprocess.run(['timeout', '-k', '10', '120', exe, small['path'], params, str(s['w']), str(s['h']), frame] +
                       [repr(float(v)) for v in [fx, fy, cx, cy] + dist], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().split('\n')
    assert lines[0] == 'engine_detect_lens: DLA-34 %d NV12 frames of %dx%d (pitch 256) rectified on a 128x256 canvas' % (B, s['h'], s['w']), lines[0]
    live = np.argwhere(rec[..., 31] >= 1)
    kept = int((rows[..., 14] == 2).sum())
    assert lines[-1] == 'engine_detect_lens: %d detections, %d KITTI rows, rectified frame 0 sums to %d' % (len(live), kept, total), lines[-1]
    assert len(lines) == len(live) + 2 and len(live) > 0
    for line, (b, i) in zip(lines[1:-1], live):
        head, _, tail = line.partition(' | ')
        v = head.split()
        assert (int(v[0]), int(v[1]), int(v[2])) == (b, i, int(rec[b, i, 0]))
        assert np.array_equal(np.array([float(x) for x in v[3:]], np.float32), rec[b, i, [1, 20, 21, 22, 23]])
        assert bool(tail) == (rows[b, i, 14] == 2)
        if tail:
            assert np.array_equal(np.array([float(x) for x in tail.split()]), rows[b, i])
