"""GPU (-m gpu): the apply fold - the apply pass of the spatial-softmax fusion run in the epilogue of the persistent 256 x 256
conv that computes z_in (runtime.hip: rtm3d_op_softmax_fuse's peephole, conv_mfma256.hip: RES >= 2).

The yardstick of every case is the UNFUSED path of the same build (RTM3D_NO_APPLY_FOLD=1, read by the recorder at every
rtm3d_op_softmax_fuse), which tests/test_gpu_kernels.py, test_gpu_tail.py and test_gpu_parity.py tie to torch and the oracle: the
fused path must give its bytes (np.array_equal / torch.equal on z and on the logit maps).  Every case also asserts that the fold did
or did not fire: a folded conv's slot reports 0 bytes in rtm3d_op_info (its work is accounted to the fusion's slot).

Shapes are the smallest that admission routes as the case needs (conv_mfma256_route, conv_mfma256_halo_supported: the halo route wants
Wm % 32 == 0 and Hm % 8 == 0; the persistent route wants >= 4 K-tiles): a 1x1 256 -> 256 conv has exactly 4 (the non-temporal
pixel operand, XNT = 1), a 3x3 64 -> 256 conv 9 (XNT = 0).  24 x 40 maps have 960 pixels per image: tiles that straddle two images
(statistics per pixel) next to tiles inside one (statistics per tile), and a partial last tile whose padded rows store the last
pixel's value again.  The ticket counters of the persistent kernels cannot be read through the ABI; what stands in for "they are
back at zero" is a second persistent conv behind the fusion in the same replay (no reset in between) and three replays with equal
bytes."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rtm3d_amd                                             # noqa: E402
from rtm3d_amd import plan as plan_mod, _lib, weights, engine    # noqa: E402

SWITCH = 'RTM3D_NO_APPLY_FOLD'


@pytest.fixture(autouse=True)
def _restore_switch():
    old = os.environ.get(SWITCH)
    yield
    if old is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = old


def _set_switch(off):
    if off is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = '1' if off else '0'


def _op_table(lib, ctx):
    """[(kernel name, bytes)] of every recorded op."""
    out = []
    while True:
        fl, by, nm = ctypes.c_double(), ctypes.c_double(), ctypes.c_char_p()
        if lib.rtm3d_op_info(ctx, len(out), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(nm)) != 0:
            return out
        out.append((nm.value.decode(), by.value))


def _folded(lib, ctx):
    """Number of conv slots that launch nothing (their conv runs, fused, in a softmax slot)."""
    return sum(1 for name, by in _op_table(lib, ctx) if 'mfma256' in name and by == 0.0)


def _run(P, feeds, fetch, off, replays=1, graph=False):
    """Records P with the switch set to `off`, runs it `replays` times; returns (number of folded convs, [fetched maps per replay])."""
    _set_switch(off)
    R = plan_mod.RealizedPlan(P, 0)
    try:
        n_fold = _folded(R.lib, R.ctx)
        if graph:
            R.set_graph(True)
        for s, arr in feeds:
            arr = np.ascontiguousarray(arr, np.float32)
            _lib.check(R.lib.rtm3d_tensor_upload(R.ctx, R.tids[s.tid], s.coff, s.C, arr.ctypes.data_as(ctypes.c_void_p)))
        xin = torch.zeros(16, device='cuda')
        outs = [torch.zeros(16, device='cuda') for _ in range(4)]
        got = []
        for _ in range(replays):
            R.forward(torch.cuda.current_stream().cuda_stream, xin.data_ptr(), [o.data_ptr() for o in outs])
            torch.cuda.synchronize()
            got.append([R.download(s) for s in fetch])
        if graph:
            assert R.graph_stats()[2], 'the context left graph mode'
        return n_fold, got
    finally:
        R.close()


def _check(P, feeds, fetch, expect_fold, replays=1, graph=False):
    """Unfused reference once, then the default recording: bytes equal in every replay, and the fold fired or not as expected."""
    n_ref, ref = _run(P, feeds, fetch, off=True)
    assert n_ref == 0
    n_fold, got = _run(P, feeds, fetch, off=None, replays=replays, graph=graph)
    assert n_fold == (1 if expect_fold else 0), (n_fold, expect_fold)
    for r in ref[0]:
        assert np.isfinite(r).all() and np.abs(r).max() > 0
    for rep in got:
        for a, b in zip(rep, ref[0]):
            assert np.array_equal(a, b), float(np.abs(a - b).max())
    return ref[0]


def _w(rng, cout, cin, k, gain=1.0):
    return (rng.standard_normal((cout, cin, k, k)) * gain / np.sqrt(cin * k * k)).astype(np.float32)


class Fusion:
    """x0 --conv--> z0, z = z0 + sum u_i softmax(u_i), then a second persistent conv on z (it draws its tiles from the same ticket
    counters, with no reset in between)."""

    def __init__(self, B, H, W, n_u, k=1, relu=False, seed=0, u_pads=(0, 1, 0), tail=True):
        rng = np.random.default_rng(seed)
        self.B, self.H, self.W, self.rng = B, H, W, rng
        cin = 256 if k == 1 else 64
        P = self.P = plan_mod.Plan(B, H * 4, W * 4)
        self.x0 = P.tensor(H, W, cin, 1)
        self.z0 = P.tensor(H, W, 256, 0)
        self.us = [P.tensor(H, W, 256, u_pads[i]) for i in range(n_u)]
        self.z = P.tensor(H, W, 256, 6)
        self.w0, self.b0 = _w(rng, 256, cin, k), (rng.standard_normal(256) * 0.2).astype(np.float32)
        self.k, self.relu, self.tail = k, relu, tail
        self.feeds = [(self.x0, rng.standard_normal((B, cin, H, W)).astype(np.float32))]
        self.fetch = [self.z]

    def producer(self, **kw):
        self.P.conv(self.x0, self.z0, self.w0, self.b0, relu=self.relu, name='z0conv', **kw)
        self.P.ops[-1]['variant'] = _lib.CONV_MFMA256

    def feed_us(self, scales=(1.0, 3.0, 6.0)):
        for u, s in zip(self.us, scales):
            self.feeds.append((u, (self.rng.standard_normal((self.B, 256, self.H, self.W)) * s).astype(np.float32)))

    def fuse(self):
        self.P.softmax_fuse(self.z0, self.z, self.us, name='fuse')
        if self.tail:
            y = self.P.tensor(self.H, self.W, 256, 0)
            self.P.conv(self.z, y, _w(self.rng, 256, 256, 1), np.zeros(256, np.float32), name='tail')
            self.P.ops[-1]['variant'] = _lib.CONV_MFMA256
            self.fetch.append(y)


@pytest.mark.parametrize('n_u', [1, 2, 3])
def test_fold_with_partials_from_halo_producers(n_u):
    """The u maps come from transposed convs on the halo-tile kernel, whose epilogues emit the softmax partials: the folded slot
    launches the combine pass and the fused conv only.  16 x 64 maps (four tiles per image), 1x1 producer (XNT = 1)."""
    B, H, W = 2, 8, 32
    f = Fusion(B, 2 * H, 2 * W, n_u, u_pads=(0, 0, 0))
    f.producer()
    xs = [f.P.tensor(H, W, 256, 1) for _ in range(n_u)]
    for x, u, sc in zip(xs, f.us, (1.0, 2.5, 6.0)):
        f.P.deconv(x, u, (f.rng.standard_normal((256, 256, 4, 4)) * sc / 32).astype(np.float32), name='up')
        f.P.ops[-1]['variant'] = _lib.CONV_MFMA256
        f.feeds.append((x, f.rng.standard_normal((B, 256, H, W)).astype(np.float32)))
    f.fuse()
    _set_switch(None)
    R = plan_mod.RealizedPlan(f.P, 0)
    try:
        assert sorted(R.lowering['stat_slots'].values()) == list(range(n_u))
        assert R.kernel_names()[0] == 'conv1x1_mfma256'
    finally:
        R.close()
    _check(f.P, f.feeds, f.fetch + f.us, expect_fold=True)


@pytest.mark.parametrize('n_u,k,relu', [(3, 3, True), (2, 1, False)])
def test_fold_with_the_reduce_pass_straddling_tiles_and_replays(n_u, k, relu):
    """24 x 40 maps, which the halo route refuses: the partials come from the stand-alone reduce pass.  B = 3: 2880 pixels = 11.25
    tiles - tiles inside one image, tiles that straddle two, a partial last tile.  Three replays."""
    f = Fusion(3, 24, 40, n_u, k=k, relu=relu, seed=3)
    f.producer()
    f.feed_us()
    f.fuse()
    _check(f.P, f.feeds, f.fetch, expect_fold=True, replays=3)


def test_fold_with_a_transposed_conv_producer():
    """z0 from a transposed conv, as in the network's neck (kfpn_up3+kfpn_proj3+head2): the four sub-pixel phases are four groups
    with out_scale 2 that write every pixel of z0 once between them.  Iteration map 12 x 20 (240 pixels per image, B = 3: tiles
    that straddle images and a partial last tile in every phase), 16 K-tiles."""
    f = Fusion(3, 24, 40, 3, seed=13)
    x = f.P.tensor(12, 20, 256, 1)
    f.P.deconv(x, f.z0, (f.rng.standard_normal((256, 256, 4, 4)) / 32).astype(np.float32), name='z0conv')
    f.P.ops[-1]['variant'] = _lib.CONV_MFMA256
    f.feeds = [(x, f.rng.standard_normal((3, 256, 12, 20)).astype(np.float32))]
    f.feed_us()
    f.fuse()
    _set_switch(None)
    R = plan_mod.RealizedPlan(f.P, 0)
    try:
        assert R.kernel_names()[0] == 'deconv4x4_phase_mfma256'      # the generic persistent kernel
    finally:
        R.close()
    _check(f.P, f.feeds, f.fetch, expect_fold=True, replays=2)


def test_fold_through_the_graph_replay():
    f = Fusion(2, 24, 40, 3, k=3, seed=4)
    f.producer()
    f.feed_us()
    f.fuse()
    _check(f.P, f.feeds, f.fetch, expect_fold=True, replays=3, graph=True)


def test_fold_with_peaked_inputs():
    """One pixel far above the rest (exponentials that underflow to zero everywhere else), and a map of equal values (S = H * W), as
    in test_gpu_kernels.py::test_softmax_fuse_with_peaked_inputs.  12 x 20: both tiles straddle images."""
    B, H, W = 2, 12, 20
    f = Fusion(B, H, W, 3, seed=5)
    f.producer()
    f.feed_us((1.0, 3.0, 6.0))
    f.feeds[1][1][:, :, 3, 4] += 9.0
    f.feeds[2][1][:, :, 7, 11] += 200.0                      # exp(u - M) underflows everywhere else
    f.feeds[3][1][...] = 1.5                                  # equal values: softmax = 1 / (H * W)
    f.fuse()
    z, _ = _check(f.P, f.feeds, f.fetch, expect_fold=True)
    assert np.isfinite(z).all()


# ---------------------------------------------------------------------------------------------- the fold must not fire
def test_no_fold_when_z0_is_read_by_an_op_in_between():
    f = Fusion(2, 24, 40, 2, seed=6)
    f.producer()
    f.feed_us()
    y = f.P.tensor(12, 20, 256, 0)
    f.P.maxpool(f.z0, y, 2, 2, 0, name='reader')
    f.fuse()
    _check(f.P, f.feeds, f.fetch + [y], expect_fold=False)


def test_fold_is_undone_when_z0_is_read_by_a_later_op():
    """The reader is recorded BEHIND the fusion: the fold, already made, is taken back."""
    f = Fusion(2, 24, 40, 2, seed=7)
    f.producer()
    f.feed_us()
    f.fuse()
    y = f.P.tensor(12, 20, 256, 0)
    f.P.maxpool(f.z0, y, 2, 2, 0, name='reader')
    _check(f.P, f.feeds, f.fetch + [y, f.z0], expect_fold=False)


def test_no_fold_when_the_producer_has_a_residual():
    f = Fusion(2, 24, 40, 2, seed=8)
    r = f.P.tensor(24, 40, 256, 0)
    f.producer(res=r)
    f.feeds.append((r, f.rng.standard_normal((2, 256, 24, 40)).astype(np.float32)))
    f.feed_us()
    f.fuse()
    _check(f.P, f.feeds, f.fetch, expect_fold=False)


def test_no_fold_when_the_producer_has_two_groups():
    """Two of the four sub-pixel phases of a transposed conv write z0 (the other pixels keep the tensor's zeros): two groups, both
    with 256 channels at offset 0, out_scale 2.  They do not write every pixel of z0, so the fold must leave them alone (all FOUR
    phases fold: test_fold_with_a_transposed_conv_producer)."""
    f = Fusion(2, 24, 40, 2, seed=9)
    x = f.P.tensor(12, 20, 256, 1)
    f.P.deconv(x, f.z0, (f.rng.standard_normal((256, 256, 4, 4)) / 32).astype(np.float32), name='z0conv')
    op = f.P.ops[-1]
    op.update(groups=2, variant=_lib.CONV_MFMA256, w=op['w'][:2], bias=op['bias'][:2],
              **{k: op[k][:2] for k in ('inp', 'out', 'res', 'taps', 'out_off')})
    f.feeds = [(x, f.rng.standard_normal((2, 256, 12, 20)).astype(np.float32))]
    f.feed_us()
    f.fuse()
    _set_switch(None)
    R = plan_mod.RealizedPlan(f.P, 0)
    try:
        assert R.kernel_names()[0] == 'deconv4x4_phase_mfma256'      # the generic persistent kernel
    finally:
        R.close()
    _check(f.P, f.feeds, f.fetch, expect_fold=False)


def test_no_fold_when_the_producer_is_on_the_halo_route():
    f = Fusion(2, 16, 64, 2, k=3, seed=10)                   # 3x3 on a 16 x 64 map: the halo-tile kernel
    f.producer()
    f.feed_us()
    f.fuse()
    _set_switch(None)
    R = plan_mod.RealizedPlan(f.P, 0)
    try:
        assert R.kernel_names()[0] == 'conv3x3_mfma256_halo'
    finally:
        R.close()
    _check(f.P, f.feeds, f.fetch, expect_fold=False)


def test_no_fold_when_z_in_is_not_a_conv_output():
    f = Fusion(2, 24, 40, 3, seed=11)
    f.feeds = [(f.z0, f.rng.standard_normal((2, 256, 24, 40)).astype(np.float32))]
    f.feed_us()
    f.fuse()
    _check(f.P, f.feeds, f.fetch, expect_fold=False)


def test_the_switch_is_read_at_every_recording():
    f = Fusion(2, 24, 40, 1, seed=12)
    f.producer()
    f.feed_us()
    f.fuse()
    for off, want in ((True, 0), (False, 1), (True, 0), (None, 1)):
        n, _ = _run(f.P, f.feeds, f.fetch, off=off)
        assert n == want, (off, n)


# ---------------------------------------------------------------------------------------------- the whole network
def _model(dev):
    cfg = rtm3d_amd.kitti_config('DLA-34')
    m = rtm3d_amd.create_model(cfg).to(dev).eval()
    m.load_state_dict(weights.synth_state_dict('DLA-34', 1, 'trained', heat_bias=-3.0))
    return m


def _model_run(m, x, off, dev, graph=None):
    _set_switch(off)
    m.use_graph = graph
    m._drop_plans()
    logits = [t.clone() for t in m.forward_logits(x)]
    torch.cuda.synchronize()
    B, _, H, W = x.shape
    plan = m._plan_for(B, H, W, dev, 'dense')
    return _folded(plan.lib, plan.ctx), logits, plan.download(plan.plan.named['z'])


def test_whole_network_many_tiles_per_workgroup_and_engine_file(tmp_path):
    """DLA-34 at B = 3, 384 x 1280: the z0 conv has 360 tiles - several per workgroup, one list per XCD.  The same through an
    engine file (the loader replays the recorded ABI calls, so it folds on its own)."""
    dev = torch.device('cuda', 0)
    m = _model(dev)
    B, H, W = 3, 384, 1280
    x = weights.synth_images(B, H, W).to(dev)
    n0, want, z_want = _model_run(m, x, True, dev)
    assert n0 == 0
    for rep in range(2):
        n1, got, z_got = _model_run(m, x, None, dev)
        assert n1 == 1
        assert np.array_equal(z_got, z_want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    path = str(tmp_path / 'e.rtm3d')
    m.save_engine(path, B, H, W)
    eng = engine.Engine(path, dev)
    try:
        assert _folded(eng.lib, eng.ctx) == 1
        for _ in range(3):
            got = eng.forward_logits(x)
            torch.cuda.synchronize()
            for a, b in zip(got, want):
                assert torch.equal(a, b)
    finally:
        eng.close()
        m._drop_plans()


def test_whole_network_small_through_the_graph_replay(monkeypatch):
    """B = 2, 64 x 128 (a 16 x 32 map: two tiles per image), the 256 x 256 kernels admitted from one tile on; hipGraph replay."""
    monkeypatch.setattr(plan_mod, 'V2_MIN_TILES', 1)
    monkeypatch.setattr(plan_mod, 'V2_MIN_TILES_SHALLOW', 1)
    dev = torch.device('cuda', 0)
    m = _model(dev)
    x = weights.synth_images(2, 64, 128).to(dev)
    n0, want, z_want = _model_run(m, x, True, dev, graph=True)
    assert n0 == 0
    n1, got, z_got = _model_run(m, x, None, dev, graph=True)
    assert n1 == 1
    assert np.array_equal(z_got, z_want)
    for _ in range(3):                                      # the first call captured the graph; these replay it
        again = m.forward_logits(x)
        torch.cuda.synchronize()
        for a, b, c in zip(again, got, want):
            assert torch.equal(a, c) and torch.equal(b, c)
    m._drop_plans()
