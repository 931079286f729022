"""GPU (-m gpu): the 256 px x 256 ch conv family (conv_mfma256.hip: one-tile and generic persistent kernels, conv_mfma256_halo.hip,
conv_mfma256_lattice.hip) over every route and tile schedule its admission accepts, against a float64 reference of the same
operation on fp16-rounded operands.

Every case first asserts the route it claims (the op name, admit_mfma256) and the tile regime it claims (tests/conv256_tiles.py:
one list or per-XCD lists, empty lists, the guaranteed run of consecutive tiles per workgroup, the lattice ring bases that run
reaches).  Then it checks the numbers with the output tensor poisoned: NaN in every output slice (a skipped tile cannot pass), a
finite sentinel in the channels outside the slices (must be untouched), and a zero border (the next conv reads it as padding),
read back raw from the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import plan as plan_mod, _lib     # noqa: E402
from tests import conv256_tiles as tl            # noqa: E402
from tests.conv_harness import SENTINEL, every_pair_order, f16, raw_read, raw_write   # noqa: E402

CUS = 256                       # the tile mirror's CU count (MI355X, SPX: 8 XCDs x 32)


def setup_module():
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, 'the tile mirror assumes %d CUs' % CUS


def spec(route, B, H, W, cin, cout, kind='conv', k=3, dil=1, groups=1, relu=True, res=False, in_P=None, out_P=1, in_extra=0,
         out_lo=0, out_hi=0, expect=None):
    """One conv256 op: its input map H x W, the route it must take and what the tile mirror must say about it (`expect`)."""
    if in_P is None:
        in_P = max(dil * (k - 1) // 2, 1)
    return dict(route=route, B=B, H=H, W=W, cin=cin, cout=cout, kind=kind, k=k, dil=dil, groups=groups if kind == 'conv' else 4,
                relu=relu, res=res, in_P=in_P, out_P=out_P, in_extra=in_extra, out_lo=out_lo, out_hi=out_hi, expect=expect or {})


def check_regime(sp):
    """The tile regime of spec sp (tests/conv256_tiles.py) against what the case claims."""
    r = tl.tiles(sp['route'], sp['B'] * sp['H'] * sp['W'], sp['cout'], sp['groups'], sp['cin'], CUS)
    for key, want in sp['expect'].items():
        assert r[key] == want, (key, r[key], want, r)
    return r


class Conv(object):
    """A conv256 op of a plan with an output tensor of its own and the host images of its operands.  shared: an earlier Conv of
    the same spec whose input (and residual) tensor and weights this one reuses."""

    def __init__(self, P, sp, rng, shared=None):
        self.sp = sp
        B, H, W, cin, cout, G = P.B, sp['H'], sp['W'], sp['cin'], sp['cout'], sp['groups']
        assert B == sp['B']
        deconv = sp['kind'] == 'deconv'
        gin = 1 if deconv else G
        if shared is None:
            self.xt = P.tensor(H, W, sp['in_extra'] + gin * cin, sp['in_P'])
            img = np.zeros((B, H + 2 * sp['in_P'], W + 2 * sp['in_P'], sp['in_extra'] + gin * cin), np.float16)
            img[:, sp['in_P']:sp['in_P'] + H, sp['in_P']:sp['in_P'] + W] = f16(rng.standard_normal(img.shape[:1] + (H, W, img.shape[3])))
            self.x_img = img
            if deconv:
                self.w = f16(rng.standard_normal((cin, cout, 4, 4)) / np.sqrt(cin * 4)).astype(np.float32)
                self.b = None
            else:
                k = sp['k']
                self.w = [f16(rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32) for _ in range(G)]
                self.b = [rng.standard_normal(cout).astype(np.float32) for _ in range(G)]
            self.rt, self.r_img = None, None
            if sp['res']:
                assert G == 1
                self.rt = P.tensor(H, W, 64 + cout, 1)
                r = np.zeros((B, H + 2, W + 2, 64 + cout), np.float16)
                r[:, 1:H + 1, 1:W + 1] = f16(rng.standard_normal((B, H, W, 64 + cout)))
                self.r_img = r
        else:
            self.xt, self.x_img, self.w, self.b, self.rt, self.r_img = shared.xt, shared.x_img, shared.w, shared.b, shared.rt, shared.r_img
        Ho, Wo = (2 * H, 2 * W) if deconv else (H, W)
        self.Ho, self.Wo = Ho, Wo
        nw = cout if deconv else G * cout              # output channels the op writes
        self.yt = P.tensor(Ho, Wo, sp['out_lo'] + nw + sp['out_hi'], sp['out_P'])
        self.wlo, self.whi = sp['out_lo'], sp['out_lo'] + nw
        if deconv:
            P.deconv(P.sub(self.xt, sp['in_extra'], cin), P.sub(self.yt, sp['out_lo'], cout), self.w, name='t')
        elif G == 1:
            rs = P.sub(self.rt, 64, cout) if sp['res'] else None
            P.conv(P.sub(self.xt, sp['in_extra'], cin), P.sub(self.yt, sp['out_lo'], cout), self.w[0], self.b[0], dil=sp['dil'],
                   relu=sp['relu'], res=rs, name='t')
        else:
            P.grouped_conv([P.sub(self.xt, sp['in_extra'] + g * cin, cin) for g in range(G)],
                           [P.sub(self.yt, sp['out_lo'] + g * cout, cout) for g in range(G)], self.w, self.b, dil=sp['dil'],
                           relu=sp['relu'], name='t')
        self.shared = shared                            # (same operands and weights: the same reference)
        self.op = P.ops[-1]
        self.op['variant'] = _lib.CONV_MFMA256
        # the poisoned output image: zero border, sentinel outside the written channels, NaN inside
        Po = sp['out_P']
        img = np.zeros((B, Ho + 2 * Po, Wo + 2 * Po, self.yt.C), np.float16)
        img[:, Po:Po + Ho, Po:Po + Wo] = SENTINEL
        img[:, Po:Po + Ho, Po:Po + Wo, self.wlo:self.whi] = np.nan
        self.poison = img
        self.ref = None

    def reference(self, dev='cuda'):
        """float64 result of the op's taps (the plan's statement of the conv) on the fp16 operands: (B, Ho, Wo, written channels),
        rounded to fp16 like the kernel's store."""
        op, sp = self.op, self.sp
        Pi, s = sp['in_P'], op['out_scale']
        Hm, Wm, cin, cout = op['Hm'], op['Wm'], op['cin'], op['cout']
        assert op['in_stride'] == 1
        X = torch.from_numpy(self.x_img).to(dev, torch.float64)
        Wt = torch.from_numpy(op['w']).to(dev, torch.float64)                      # (G, taps, cout, cin)
        out = torch.full((sp['B'], self.Ho, self.Wo, self.whi - self.wlo), float('nan'), dtype=torch.float64, device=dev)
        for g in range(op['groups']):
            c0 = op['inp'][g].coff
            acc = torch.from_numpy(op['bias'][g]).to(dev, torch.float64).expand(sp['B'], Hm, Wm, cout).clone()
            for t, (dy, dx) in enumerate(op['taps'][g]):
                xs = X[:, Pi + dy:Pi + dy + Hm, Pi + dx:Pi + dx + Wm, c0:c0 + cin]
                acc += xs @ Wt[g, t].T
            if op['res'][g] is not None:
                assert s == 1 and op['out_off'][g] == (0, 0)
                rc = op['res'][g].coff
                acc += torch.from_numpy(self.r_img[:, 1:Hm + 1, 1:Wm + 1, rc:rc + cout]).to(dev, torch.float64)
            if op['relu']:
                acc = acc.relu()
            oy, ox = op['out_off'][g]
            cc = op['out'][g].coff - self.wlo
            out[:, oy::s, ox::s, cc:cc + cout] = acc
        assert not torch.isnan(out).any(), 'the reference does not cover the output slice'
        return out.cpu().numpy().astype(np.float16).astype(np.float32)

    def check(self, got):
        """got: raw device image of the output tensor after the forward."""
        Po = self.sp['out_P']
        border = np.ones(got.shape[:3], bool)
        border[:, Po:Po + self.Ho, Po:Po + self.Wo] = False
        assert not got.view(np.uint16)[border].any(), 'the output border was written'
        inner = got[:, Po:Po + self.Ho, Po:Po + self.Wo]
        outside = np.concatenate([inner[..., :self.wlo], inner[..., self.whi:]], -1)
        assert (outside.view(np.uint16) == SENTINEL.view(np.uint16)).all(), 'channels outside the output slice were written'
        val = inner[..., self.wlo:self.whi].astype(np.float32)
        assert np.isfinite(val).all(), '%d output values never written (NaN poison)' % int((~np.isfinite(val)).sum())
        src = self.shared or self
        if src.ref is None:
            src.ref = src.reference()
        ref = src.ref
        np.testing.assert_allclose(val, ref, rtol=2e-3, atol=2e-3 * max(1.0, float(np.abs(ref).max())))


def _forward(R, convs):
    for c in convs:
        raw_write(R, c.yt, c.poison)
    xin = torch.zeros(16, device='cuda')
    outs = [torch.zeros(16, device='cuda') for _ in range(4)]
    R.forward(torch.cuda.current_stream().cuda_stream, xin.data_ptr(), [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    return [raw_read(R, c.yt) for c in convs]


def run_plan(P, convs, replays=0, graph=False):
    """Record P, assert every op's route, upload the operands, run one poisoned forward and check every output; then
    `replays` eager replays and (graph) one hipGraph replay, each re-poisoned, all bit-identical to the first."""
    R = plan_mod.RealizedPlan(P, 0)
    try:
        names = R.kernel_names()
        assert [tl.route_of(n) for n in names] == [c.sp['route'] for c in convs], names
        done = set()
        for c in convs:
            if id(c.x_img) not in done:
                raw_write(R, c.xt, c.x_img)
                done.add(id(c.x_img))
            if c.rt is not None and id(c.r_img) not in done:
                raw_write(R, c.rt, c.r_img)
                done.add(id(c.r_img))
        first = _forward(R, convs)
        for c, got in zip(convs, first):
            c.check(got)
        later = [_forward(R, convs) for _ in range(replays)]
        if graph:
            R.set_graph(True)
            later.append(_forward(R, convs))
            captures, _, enabled = R.graph_stats()
            assert captures == 1 and enabled, R.graph_stats()
        for outs in later:
            for a, b in zip(first, outs):
                np.testing.assert_array_equal(a.view(np.uint16), b.view(np.uint16))
        return names
    finally:
        R.close()


def run_one(sp, seed):
    check_regime(sp)
    P = plan_mod.Plan(sp['B'], sp['H'] * 4, sp['W'] * 4)
    c = Conv(P, sp, np.random.default_rng(seed))
    run_plan(P, [c])


ALL8 = tl.reachable_bases(1)
assert ALL8 == [0, 2, 4, 6, 8, 10, 12, 14]

CASES = {
    # ---- lattice (dilation 6): the halo-row ring carried across tiles; ring base of a workgroup's k-th tile = 10 * cpt * k mod 16
    'lattice_cpt1_run8': spec('lattice', 4, 96, 320, 64, 1024, dil=6, expect=dict(total=1920, one_list=False, run=8, bases=ALL8)),
    'lattice_cpt2_run4': spec('lattice', 4, 96, 320, 128, 512, dil=6, expect=dict(total=960, run=4, bases=[0, 4, 8, 12])),
    'lattice_cpt3_nt3_run9': spec('lattice', 6, 96, 320, 192, 768, dil=6, expect=dict(NT=3, total=2160, run=9, bases=ALL8)),
    'lattice_cpt8_run2': spec('lattice', 2, 96, 320, 512, 512, dil=6, expect=dict(total=480, run=2, bases=[0])),
    # other shapes its eligibility admits
    'lattice_groups2_nt2': spec('lattice', 2, 48, 64, 64, 512, dil=6, groups=2, in_extra=64, expect=dict(NT=2, groups=2, total=96)),
    'lattice_groups4': spec('lattice', 1, 48, 64, 64, 256, dil=6, groups=4, expect=dict(groups=4, total=48, empty=2)),
    'lattice_no_relu': spec('lattice', 2, 48, 64, 128, 256, dil=6, relu=False, expect=dict(total=24)),
    'lattice_in_border7_out_border0': spec('lattice', 1, 48, 64, 64, 256, dil=6, in_P=7, out_P=0, expect=dict(total=12)),
    'lattice_out_border2_slice256': spec('lattice', 1, 48, 64, 128, 256, dil=6, out_P=2, out_lo=256, out_hi=256, expect=dict(total=12)),
    'lattice_b1_two_empty_lists': spec('lattice', 1, 48, 32, 64, 256, dil=6, expect=dict(total=6, empty=2, run=1)),
    # its limits: more than 1024 bias floats, a residual -> the generic persistent kernel
    'lattice_shape_nbias1280_generic': spec('persistent', 1, 48, 32, 64, 1280, dil=6, expect=dict(NT=5, total=30, one_list=True)),
    'lattice_shape_residual_generic': spec('persistent', 1, 48, 64, 64, 256, dil=6, res=True, expect=dict(total=12)),
    # ---- halo (3x3 dilation 1 and the transposed-conv phases on maps covered by 8 x 32 tiles)
    'halo_nt2_per_xcd': spec('halo', 5, 64, 128, 64, 512, expect=dict(NT=2, total=320, one_list=False, run=2)),
    'halo_nt3': spec('halo', 2, 32, 64, 128, 768, expect=dict(NT=3, total=48, one_list=True)),
    'halo_nt4': spec('halo', 2, 16, 64, 64, 1024, expect=dict(NT=4, total=32)),
    'halo_no_relu': spec('halo', 2, 16, 64, 128, 256, relu=False, expect=dict(total=8)),
    'halo_in_border2_slice128': spec('halo', 2, 16, 64, 64, 256, in_P=2, in_extra=64, out_lo=128, out_hi=128, expect=dict(total=8)),
    'halo_deconv_two_rounds': spec('halo', 3, 64, 128, 256, 256, kind='deconv', k=4, expect=dict(groups=4, total=384, one_list=False, run=2)),
    'halo_256_tiles_one_list': spec('halo', 8, 64, 128, 64, 256, expect=dict(total=256, one_list=True, run=1)),
    'halo_257_tiles_per_xcd': spec('halo', 257, 8, 32, 64, 256, expect=dict(total=257, one_list=False, run=2)),
    'halo_shape_nbias1280_generic': spec('persistent', 1, 16, 64, 64, 1280, expect=dict(NT=5, total=20)),
    # ---- generic persistent and one-tile: the ksteps >= 4 and 2048-bias limits
    'conv1x1_cin192_1tile': spec('1tile', 2, 24, 40, 192, 256, k=1),
    'conv1x1_cin192_res_1tile': spec('1tile', 2, 24, 40, 192, 256, k=1, res=True),
    'conv1x1_cin256': spec('persistent', 2, 24, 40, 256, 256, k=1, expect=dict(total=8)),
    'conv1x1_cin256_res': spec('persistent', 2, 24, 40, 256, 256, k=1, res=True, expect=dict(total=8)),
    'cout2048_persistent': spec('persistent', 1, 16, 32, 64, 2048, expect=dict(NT=8, total=16)),
    'cout2304_1tile': spec('1tile', 1, 16, 32, 64, 2304, expect=dict(NT=9)),
    # 256 / 257 tiles on ragged maps (65535 / 65661 pixels): the one-list boundary of each persistent variant
    'plain_256_tiles': spec('persistent', 1, 255, 257, 64, 256, expect=dict(total=256, one_list=True)),
    'plain_257_tiles': spec('persistent', 1, 129, 509, 64, 256, expect=dict(total=257, one_list=False, run=2)),
    'x_once_256_tiles': spec('persistent', 1, 255, 257, 256, 256, k=1, expect=dict(total=256, one_list=True)),
    'x_once_257_tiles': spec('persistent', 1, 129, 509, 256, 256, k=1, expect=dict(total=257, one_list=False)),
    'res_256_tiles': spec('persistent', 1, 255, 257, 256, 256, k=1, res=True, expect=dict(total=256, one_list=True)),
    'res_257_tiles': spec('persistent', 1, 129, 509, 256, 256, k=1, res=True, expect=dict(total=257, one_list=False)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_conv256_route_and_schedule(name):
    run_one(CASES[name], seed=sum(map(ord, name)))


# ---- several conv256 launches of different list regimes in ONE plan: the eight ticket counters are shared and reset only by the
# last draw of each launch (zero_counters runs once, at the head of the replay); a counter left non-zero would make the next
# launch that uses it start part-way down its list and skip tiles
CHAIN = {
    'lattice_empty_lists': spec('lattice', 1, 48, 32, 64, 256, dil=6, expect=dict(total=6, empty=2)),
    'lattice_rounds': spec('lattice', 1, 96, 320, 64, 1024, dil=6, expect=dict(total=480, one_list=False, run=2)),
    'halo_one_list': spec('halo', 1, 16, 64, 64, 256, expect=dict(total=4, one_list=True)),
    'halo_per_xcd': spec('halo', 1, 64, 320, 64, 1024, expect=dict(total=320, one_list=False, run=2)),
    'generic_one_list': spec('persistent', 1, 20, 36, 256, 256, k=1, expect=dict(total=3, one_list=True)),
    'generic_per_xcd_res': spec('persistent', 1, 96, 360, 256, 512, k=1, res=True, expect=dict(total=270, one_list=False, run=2)),
}


def test_conv256_counter_chain():
    keys = list(CHAIN)
    order = every_pair_order(len(keys))
    pairs = {(a, b) for a, b in zip(order, order[1:])}
    assert len(order) == len(keys) * (len(keys) - 1) + 1 and len(pairs) == len(keys) * (len(keys) - 1)
    for sp in CHAIN.values():
        check_regime(sp)
    P = plan_mod.Plan(1, 96 * 4, 360 * 4)
    rng = np.random.default_rng(5)
    first, convs = {}, []
    for i in order:
        c = Conv(P, CHAIN[keys[i]], rng, shared=first.get(i))
        first.setdefault(i, c)
        convs.append(c)
    run_plan(P, convs, replays=3, graph=True)
