"""GPU (-m gpu): the 128-pixel conv kernels (conv_mfma.hip: one-stage conv_mfma_kernel, conv_mfma_deep_kernel, deep with split-K)
and the halo kernels (conv64_halo.hip, conv128_halo.hip, conv64s2_halo.hip) over every route and regime their admission
accepts, against a float64 reference of the op's taps on fp16-rounded operands.

Every case first asserts its route (the op name) and its regime (tests/conv128_routes.py: BN, split count and K ranges, the
halo kernels' `single` / ticket regime).  Then it checks the numbers with every output poisoned: NaN in the written slice (a
skipped tile cannot pass), a sentinel in the other channels and past an fp32 NCHW slot (must be untouched), and a zero border
(the next conv reads it as padding), all read back raw from the device.  The same holds for a space-to-depth copy.  CASES is
importable without a GPU: tests/test_conv128_routes.py checks it against the mirror and against the product plans' regimes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import plan as plan_mod, _lib                                        # noqa: E402
from tests import conv128_routes as cr                                               # noqa: E402
from tests.conv_harness import SENTINEL, every_pair_order, f16, raw_read, raw_write   # noqa: E402

CUS = 256                       # the mirror's CU count (MI355X, SPX: 8 XCDs x 32)
KERNEL = {'mfma128': _lib.CONV_MFMA128, 'c64_halo': _lib.CONV_C64_HALO, 'c128_halo': _lib.CONV_C128_HALO, 'c64s2_halo': _lib.CONV_C64S2_HALO}
NCHW_PAST = 256                 # sentinel floats behind an NCHW slot


def setup_module():
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, 'the mirror assumes %d CUs' % CUS


def spec(route, B, H, W, cin, cout, kind='conv', k=3, stride=1, dil=1, groups=1, bn=64, relu=True, res=False, nchw=False, s2d='',
         ntaps=None, in_P=None, out_P=1, in_extra=0, out_lo=0, out_hi=0, s_lo=0, s_hi=0, expect=None):
    """One conv op on an H x W input map.  kind: 'conv' (k x k, stride, dilation, groups), 'deconv' (the four transposed-conv
    phases: groups 4, out_scale 2), 'tapdc' (ntaps taps with per-tap channel offsets, a project fold's form).  s2d: '' / 'copy'
    (space-to-depth copy beside the output) / 'only' (only the copy) / 'input' (conv64s2 reads the copy of its input)."""
    kernel = 'mfma128' if route in cr.MFMA128_ROUTES else route
    if in_P is None:
        in_P = max(dil * (k - 1) // 2, 1) if kind == 'conv' else 1
    if kind == 'conv':
        Hm, Wm, nt, so = (H - 1) // stride + 1, (W - 1) // stride + 1, k * k, 1
    elif kind == 'deconv':
        Hm, Wm, nt, so, groups, relu = H, W, 4, 2, 4, False
    else:
        assert kind == 'tapdc' and ntaps
        Hm, Wm, nt, so = H, W, ntaps, 1
    return dict(route=route, kernel=kernel, B=B, H=H, W=W, cin=cin, cout=cout, kind=kind, k=k, stride=stride, dil=dil, groups=groups,
                bn=bn if kernel == 'mfma128' else (128 if kernel == 'c128_halo' else None), relu=relu, res=res, nchw=nchw, s2d=s2d,
                ntaps=nt, Hm=Hm, Wm=Wm, out_scale=so, in_P=in_P, out_P=out_P, in_extra=in_extra, out_lo=out_lo, out_hi=out_hi,
                s_lo=s_lo, s_hi=s_hi, expect=expect or {})


def mirror(sp):
    if sp['kernel'] == 'mfma128':
        return cr.admit_mfma128(sp['B'] * sp['Hm'] * sp['Wm'], sp['cin'], sp['cout'], sp['ntaps'], sp['groups'], sp['bn'], sp['nchw'], CUS)
    return cr.halo(sp['kernel'], sp['B'], sp['Hm'], sp['Wm'], sp['cout'], CUS)


def regime(sp):
    """The case's regime key (tests/conv128_routes.py: regime_key), as the coverage guard compares it with the product plans'."""
    r = mirror(sp)
    halo = sp['kernel'] != 'mfma128'
    return cr.regime_key(sp['kernel'], sp['route'], sp['bn'] if not halo else None, 1 if halo else r['ks'], sp['nchw'], sp['res'],
                         sp['s2d'], sp['groups'] > 1, sp['kind'] == 'tapdc', sp['stride'], sp['out_scale'], r['single'] if halo else None)


def check_regime(sp):
    r = mirror(sp)
    if sp['kernel'] == 'mfma128':
        assert r['route'] == sp['route'], (r['route'], sp['route'], r)
    for key, want in sp['expect'].items():
        assert r[key] == want, (key, r[key], want, r)
    return r


def _tapdc_taps(n):
    """n taps within +-1 pixel with per-tap channel offsets 0, 64 or 128 (behind the input slice: a fold's second operand)."""
    return [((i // 3) % 3 - 1, i % 3 - 1) for i in range(n)], [64 * ((i + i // 9) % 3) for i in range(n)]


class Conv(object):
    """One op of a plan with tensors of its own, the host images of its operands and its poisoned outputs."""

    def __init__(self, P, sp, rng, slot=1):
        self.sp = sp
        B, H, W, cin, cout, G = P.B, sp['H'], sp['W'], sp['cin'], sp['cout'], sp['groups']
        assert B == sp['B']
        kind, Pi = sp['kind'], sp['in_P']
        gin = 1 if kind == 'deconv' else G
        self.cin_total = sp['in_extra'] + gin * cin + (128 if kind == 'tapdc' else 0)
        self.xt = P.tensor(H, W, self.cin_total, Pi)
        img = np.zeros((B, H + 2 * Pi, W + 2 * Pi, self.cin_total), np.float16)
        img[:, Pi:Pi + H, Pi:Pi + W] = f16(rng.standard_normal((B, H, W, self.cin_total)))
        self.x_img = img
        xs = [P.sub(self.xt, sp['in_extra'] + g * cin, cin) for g in range(gin)]
        Hm, Wm, so = sp['Hm'], sp['Wm'], sp['out_scale']
        self.Ho, self.Wo = Hm * so, Wm * so
        self.rt = self.r_img = None
        if sp['res']:
            self.rt = P.tensor(Hm, Wm, 64 + cout, 1)
            r = np.zeros((B, Hm + 2, Wm + 2, 64 + cout), np.float16)
            r[:, 1:Hm + 1, 1:Wm + 1] = f16(rng.standard_normal((B, Hm, Wm, 64 + cout)))
            self.r_img = r
        rs = P.sub(self.rt, 64, cout) if sp['res'] else None
        nw = cout if kind == 'deconv' else G * cout              # output channels the op writes
        self.nw, self.slot = nw, (slot if sp['nchw'] else 0)
        self.yt, self.wlo, self.whi = None, sp['out_lo'], sp['out_lo'] + nw
        if not sp['nchw']:
            self.yt = P.tensor(self.Ho, self.Wo, sp['out_lo'] + nw + sp['out_hi'], sp['out_P'])
        ys = [P.sub(self.yt, sp['out_lo'] + (0 if kind == 'deconv' else g * cout), cout) if self.yt else None for g in range(G)]
        b = [rng.standard_normal(cout).astype(np.float32) for _ in range(G)]
        name = 't%d' % len(P.ops)
        if kind == 'deconv':
            w = f16(rng.standard_normal((cin, cout, 4, 4)) / np.sqrt(cin * 4)).astype(np.float32)
            P.deconv(xs[0], ys[0], w, name=name)
        elif kind == 'tapdc':
            taps, dcs = _tapdc_taps(sp['ntaps'])
            w = f16(rng.standard_normal((cout, cin, len(taps))) / np.sqrt(cin * len(taps))).astype(np.float32)
            P.conv_taps(xs, ys, [w], b, taps, Hm, Wm, relu=sp['relu'], name=name, out_nchw=self.slot)
            P.ops[-1]['tap_dc'] = [dcs]
        else:
            k, d = sp['k'], sp['dil']
            ws = [f16(rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32) for _ in range(G)]
            if G == 1:
                P.conv(xs[0], ys[0], ws[0], b[0], stride=sp['stride'], dil=d, relu=sp['relu'], res=rs, name=name, out_nchw=self.slot,
                       out_hw=(Hm, Wm) if sp['nchw'] else None)
            elif sp['nchw']:
                pad = d * (k - 1) // 2
                taps = [(ky * d - pad, kx * d - pad) for ky in range(k) for kx in range(k)]
                P.conv_taps(xs, ys, [w.reshape(cout, cin, k * k) for w in ws], b, taps, Hm, Wm, relu=sp['relu'], name=name, out_nchw=self.slot)
            else:
                assert sp['stride'] == 1 and not sp['res']
                P.grouped_conv(xs, ys, ws, b, dil=d, relu=sp['relu'], name=name)
        self.op = P.ops[-1]
        self.op['variant'] = KERNEL[sp['kernel']]
        if sp['kernel'] == 'mfma128':
            self.op['bn_tile'] = sp['bn']
        # space-to-depth tensors: the copy this op writes, or the copy of its input it reads
        self.st = self.s_img = None
        if sp['s2d'] in ('copy', 'only'):
            self.st = P.tensor(self.Ho // 2, self.Wo // 2, sp['s_lo'] + 4 * cout + sp['s_hi'], 1)
        elif sp['s2d'] == 'input':
            assert G == 1 and H % 2 == 0 and W % 2 == 0 and Pi == 1
            self.st = P.tensor(H // 2, W // 2, sp['s_lo'] + 4 * cin + sp['s_hi'], 1)
            s = np.zeros((B, H // 2 + 2, W // 2 + 2, self.st.C), np.float16)
            s[:, 1:-1, 1:-1] = f16(rng.standard_normal((B, H // 2, W // 2, self.st.C)))
            s[:, 1:-1, 1:-1, sp['s_lo']:sp['s_lo'] + 4 * cin] = self.to_s2d(img[:, 1:-1, 1:-1, sp['in_extra']:sp['in_extra'] + cin])
            self.s_img = s
        self.poison()
        self.ref = None

    @staticmethod
    def to_s2d(a):
        """(B, H, W, C) -> (B, H / 2, W / 2, 4 C): pixel (y, x) to (y >> 1, x >> 1), channels ((y & 1) * 2 + (x & 1)) * C + c."""
        B, H, W, C = a.shape
        return a.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C)

    def poison(self):
        sp, B = self.sp, self.sp['B']
        self.y_poison = self.s_poison = self.o_poison = None
        if self.yt is not None:
            Po = sp['out_P']
            img = np.zeros((B, self.Ho + 2 * Po, self.Wo + 2 * Po, self.yt.C), np.float16)
            img[:, Po:Po + self.Ho, Po:Po + self.Wo] = SENTINEL
            if sp['s2d'] != 'only':                # (an s2d-only op must leave its plan output tensor untouched)
                img[:, Po:Po + self.Ho, Po:Po + self.Wo, self.wlo:self.whi] = np.nan
            self.y_poison = img
        if sp['s2d'] in ('copy', 'only'):
            img = np.zeros((B, self.Ho // 2 + 2, self.Wo // 2 + 2, self.st.C), np.float16)
            img[:, 1:-1, 1:-1] = SENTINEL
            img[:, 1:-1, 1:-1, sp['s_lo']:sp['s_lo'] + 4 * sp['cout']] = np.nan
            self.s_poison = img
        if sp['nchw']:
            n = B * self.nw * self.Ho * self.Wo
            o = torch.full((n + NCHW_PAST,), float('nan'), device='cuda')
            o[n:] = float(SENTINEL)
            self.o_poison = o

    def upload(self, R):
        raw_write(R, self.xt, self.x_img)
        if self.rt is not None:
            raw_write(R, self.rt, self.r_img)
        if self.s_img is not None:
            raw_write(R, self.st, self.s_img)

    def lowered(self, L):
        """The launch of this op with the space-to-depth decisions a plan cannot always express (the recorder's descriptor)."""
        assert L['kind'] == 'conv' and L['name'] == self.op['name'], (L['kind'], L['name'])
        s = self.sp['s2d']
        if s in ('copy', 'only'):
            L['s2d_out'], L['write_out'] = (self.st, self.sp['s_lo']), s == 'copy'
        elif s == 'input':
            L['in_s2d'] = (self.st, self.sp['s_lo'])

    def reference(self, dev='cuda'):
        """float64 result of the op's taps on the fp16 operands: (B, Ho, Wo, written channels)."""
        op, sp = self.op, self.sp
        Pi, s, sc = sp['in_P'], op['in_stride'], op['out_scale']
        Hm, Wm, cin, cout = op['Hm'], op['Wm'], op['cin'], op['cout']
        X = torch.from_numpy(self.x_img).to(dev, torch.float64)
        Wt = torch.from_numpy(op['w']).to(dev, torch.float64)                      # (G, taps, cout, cin)
        out = torch.full((sp['B'], self.Ho, self.Wo, self.nw), float('nan'), dtype=torch.float64, device=dev)
        for g in range(op['groups']):
            c0 = op['inp'][g].coff
            acc = torch.from_numpy(op['bias'][g]).to(dev, torch.float64).expand(sp['B'], Hm, Wm, cout).clone()
            for t, (dy, dx) in enumerate(op['taps'][g]):
                dc = op['tap_dc'][g][t] if 'tap_dc' in op else 0
                xs = X[:, Pi + dy:Pi + dy + (Hm - 1) * s + 1:s, Pi + dx:Pi + dx + (Wm - 1) * s + 1:s, c0 + dc:c0 + dc + cin]
                acc += xs @ Wt[g, t].T
            if op['res'][g] is not None:
                rc = op['res'][g].coff
                acc += torch.from_numpy(self.r_img[:, 1:Hm + 1, 1:Wm + 1, rc:rc + cout]).to(dev, torch.float64)
            if op['relu']:
                acc = acc.relu()
            oy, ox = op['out_off'][g]
            cc = g * cout if sp['nchw'] else op['out'][g].coff - self.yt.coff - self.wlo
            out[:, oy::sc, ox::sc, cc:cc + cout] = acc
        assert not torch.isnan(out).any(), 'the reference does not cover the output'
        return out.cpu().numpy()

    def check(self, got):
        """got: {'y': raw output tensor, 's': raw space-to-depth tensor, 'o': NCHW slot} after the forward."""
        sp = self.sp
        if self.ref is None:
            self.ref = self.reference()
        ref = self.ref
        tol = dict(rtol=2e-3, atol=2e-3 * max(1.0, float(np.abs(ref).max())))
        ref16 = ref.astype(np.float16).astype(np.float32)
        if self.yt is not None:
            y, Po = got['y'], sp['out_P']
            border = np.ones(y.shape[:3], bool)
            border[:, Po:Po + self.Ho, Po:Po + self.Wo] = False
            assert not y.view(np.uint16)[border].any(), 'the output border was written'
            inner = y[:, Po:Po + self.Ho, Po:Po + self.Wo]
            if sp['s2d'] == 'only':
                assert (inner.view(np.uint16) == SENTINEL.view(np.uint16)).all(), 'an s2d-only op wrote its output tensor'
            else:
                outside = np.concatenate([inner[..., :self.wlo], inner[..., self.whi:]], -1)
                assert (outside.view(np.uint16) == SENTINEL.view(np.uint16)).all(), 'channels outside the output slice were written'
                val = inner[..., self.wlo:self.whi].astype(np.float32)
                assert np.isfinite(val).all(), '%d output values never written (NaN poison)' % int((~np.isfinite(val)).sum())
                np.testing.assert_allclose(val, ref16, **tol)
        if sp['s2d'] in ('copy', 'only'):
            st = got['s']
            border = np.ones(st.shape[:3], bool)
            border[:, 1:-1, 1:-1] = False
            assert not st.view(np.uint16)[border].any(), 'the space-to-depth border was written'
            inner = st[:, 1:-1, 1:-1]
            lo, hi = sp['s_lo'], sp['s_lo'] + 4 * sp['cout']
            outside = np.concatenate([inner[..., :lo], inner[..., hi:]], -1)
            assert (outside.view(np.uint16) == SENTINEL.view(np.uint16)).all(), 'channels outside the s2d slice were written'
            val = inner[..., lo:hi].astype(np.float32)
            assert np.isfinite(val).all(), '%d s2d values never written (NaN poison)' % int((~np.isfinite(val)).sum())
            np.testing.assert_allclose(val, self.to_s2d(ref16), **tol)
        if sp['nchw']:
            o = got['o']
            n = sp['B'] * self.nw * self.Ho * self.Wo
            assert (o[n:] == np.float32(SENTINEL)).all(), 'floats past the NCHW slot were written'
            val = o[:n].reshape(sp['B'], self.nw, self.Ho, self.Wo)
            assert np.isfinite(val).all(), '%d NCHW values never written (NaN poison)' % int((~np.isfinite(val)).sum())
            np.testing.assert_allclose(val, ref.transpose(0, 3, 1, 2).astype(np.float32), **tol)


def _forward(R, convs):
    for c in convs:
        c.poison()
        if c.y_poison is not None:
            raw_write(R, c.yt, c.y_poison)
        if c.s_poison is not None:
            raw_write(R, c.st, c.s_poison)
    xin = torch.zeros(16, device='cuda')
    outs = [torch.zeros(16, device='cuda') for _ in range(4)]
    for c in convs:
        if c.o_poison is not None:
            assert outs[c.slot - 1].numel() == 16, 'two NCHW ops share slot %d' % c.slot
            outs[c.slot - 1] = c.o_poison
    R.forward(torch.cuda.current_stream().cuda_stream, xin.data_ptr(), [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    return [{'y': raw_read(R, c.yt) if c.yt is not None else None,
             's': raw_read(R, c.st) if c.s_poison is not None else None,
             'o': c.o_poison.cpu().numpy() if c.o_poison is not None else None} for c in convs]


def realize(P, convs):
    """RealizedPlan of P with every launch carrying its conv's space-to-depth decisions."""
    lower = plan_mod.lower

    def lower_with_s2d(plan):
        low = lower(plan)
        assert len(low['launches']) == len(convs), [L['name'] for L in low['launches']]
        for L, c in zip(low['launches'], convs):
            c.lowered(L)
        return low
    plan_mod.lower = lower_with_s2d
    try:
        return plan_mod.RealizedPlan(P, 0)
    finally:
        plan_mod.lower = lower


def run_plan(P, convs, replays=0, graph=False):
    """Record P, assert every op's route, upload the operands, run one poisoned forward and check every output; then
    `replays` eager replays and (graph) one hipGraph replay, each re-poisoned, all bit-identical to the first."""
    R = realize(P, convs)
    try:
        names = R.kernel_names()
        assert [cr.route_of(n) for n in names] == [c.sp['route'] for c in convs], names
        for c in convs:
            c.upload(R)
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
                for key in a:
                    if a[key] is not None:
                        np.testing.assert_array_equal(a[key].view(np.uint32 if key == 'o' else np.uint16),
                                                      b[key].view(np.uint32 if key == 'o' else np.uint16))
        return names
    finally:
        R.close()


def run_one(sp, seed):
    check_regime(sp)
    P = plan_mod.Plan(sp['B'], sp['H'] * 4, sp['W'] * 4)
    run_plan(P, [Conv(P, sp, np.random.default_rng(seed))])


OS, DEEP, SPLIT = 'one_stage', 'deep', 'deep_splitk'
C64, C128, C64S2 = 'c64_halo', 'c128_halo', 'c64s2_halo'

CASES = {
    # ---- one-stage kernel (conv_mfma_kernel): BN 16 / 32 always; BN 64 / 128 above `cus` workgroups (264 pixel tiles here)
    'os_bn16': spec(OS, 1, 20, 30, 64, 16, bn=16, expect=dict(MT=5, empty_xcds=3)),
    'os_bn16_res': spec(OS, 2, 24, 40, 128, 32, bn=16, res=True, out_lo=8, out_hi=16, expect=dict(NT=2)),
    'os_bn32': spec(OS, 2, 24, 40, 64, 32, bn=32, expect=dict(MT=15)),
    'os_bn32_res': spec(OS, 1, 12, 20, 192, 64, bn=32, res=True, expect=dict(MT=2, NT=2, empty_xcds=6)),
    'os_bn64': spec(OS, 1, 66, 512, 64, 64, expect=dict(wgs=264)),
    'os_bn64_res': spec(OS, 1, 66, 512, 64, 64, res=True, out_P=0, expect=dict(wgs=264)),
    'os_bn128': spec(OS, 1, 66, 512, 64, 128, bn=128, expect=dict(wgs=264)),
    'os_bn128_res': spec(OS, 1, 66, 512, 64, 128, bn=128, res=True, in_extra=64, expect=dict(wgs=264)),
    'os_ragged_m_nt2': spec(OS, 2, 45, 301, 64, 128, expect=dict(MT=212, NT=2, wgs=424)),
    'os_257_workgroups': spec(OS, 1, 257, 128, 64, 64, expect=dict(wgs=257)),
    'os_stride2_bn128': spec(OS, 1, 132, 1024, 64, 128, stride=2, bn=128, expect=dict(wgs=264)),
    'os_dil6': spec(OS, 1, 66, 512, 64, 64, dil=6, expect=dict(wgs=264)),
    'os_deconv_groups4': spec(OS, 1, 36, 256, 64, 64, kind='deconv', expect=dict(wgs=288)),
    'os_tapdc_bn64': spec(OS, 1, 66, 512, 64, 64, kind='tapdc', ntaps=5, expect=dict(wgs=264)),
    'os_tapdc_bn128': spec(OS, 1, 66, 512, 64, 128, kind='tapdc', ntaps=3, bn=128, expect=dict(wgs=264)),
    'os_x_once_1x1': spec(OS, 1, 66, 512, 128, 64, k=1, expect=dict(wgs=264, NT=1)),
    'os_s2d_copy_bn64': spec(OS, 1, 66, 512, 64, 64, s2d='copy', s_lo=64, s_hi=8, expect=dict(wgs=264)),
    'os_s2d_copy_bn128_res': spec(OS, 1, 66, 512, 64, 128, bn=128, res=True, s2d='copy', expect=dict(wgs=264)),
    'os_s2d_only_bn128': spec(OS, 1, 66, 512, 64, 128, bn=128, s2d='only', s_lo=128, expect=dict(wgs=264)),
    'os_s2d_only_bn128_res': spec(OS, 1, 66, 512, 128, 128, bn=128, res=True, s2d='only', expect=dict(wgs=264)),
    # the fp32 NCHW epilogue (EPI = 1): ragged cout, groups at channel offsets g * cout
    'nchw_bn16_cout2': spec(OS, 1, 20, 30, 64, 2, bn=16, nchw=True, expect=dict(NT=1, cout_pad=16)),
    'nchw_bn16_cout3': spec(OS, 2, 5, 5, 256, 3, bn=16, nchw=True, relu=False),
    'nchw_bn16_cout20': spec(OS, 1, 24, 40, 64, 20, bn=16, nchw=True, expect=dict(NT=2)),
    'nchw_bn32_cout40': spec(OS, 2, 24, 40, 128, 40, bn=32, nchw=True, expect=dict(NT=2)),
    'nchw_bn64_cout72': spec(OS, 1, 24, 40, 64, 72, bn=64, nchw=True, expect=dict(NT=2, route=OS)),
    'nchw_bn64_groups2_cout3': spec(OS, 1, 12, 20, 64, 3, bn=64, groups=2, nchw=True),
    'nchw_bn16_groups4_cout20': spec(OS, 2, 9, 13, 64, 20, bn=16, groups=4, nchw=True, in_extra=64),
    # ---- deep kernel, ksplit 1 (BN 64 / 128, at most `cus` workgroups)
    'deep_bn64_ksteps1': spec(DEEP, 1, 16, 128, 64, 64, k=1, expect=dict(ksteps=1, ks=1)),
    'deep_bn128_ksteps2': spec(DEEP, 1, 16, 128, 128, 128, k=1, bn=128, expect=dict(ksteps=2, ks=1)),
    'deep_bn64_ksteps3': spec(DEEP, 1, 16, 128, 192, 64, k=1, expect=dict(ksteps=3, ks=1)),
    'deep_bn128_3x3': spec(DEEP, 1, 136, 128, 64, 128, bn=128, expect=dict(wgs=136, ks=1)),
    'deep_ksteps7': spec(DEEP, 1, 16, 128, 448, 64, k=1, expect=dict(ksteps=7, ks=1)),
    'deep_129_workgroups': spec(DEEP, 1, 129, 128, 64, 64, expect=dict(wgs=129, ks=1)),
    'deep_256_workgroups': spec(DEEP, 1, 256, 128, 64, 64, expect=dict(wgs=256, ks=1)),
    'deep_res': spec(DEEP, 1, 136, 128, 64, 64, res=True, expect=dict(wgs=136)),
    'deep_stride2': spec(DEEP, 1, 272, 256, 64, 64, stride=2, expect=dict(wgs=136)),
    'deep_tapdc': spec(DEEP, 1, 16, 128, 64, 64, kind='tapdc', ntaps=7, expect=dict(ksteps=7)),
    'deep_deconv_groups4': spec(DEEP, 1, 8, 128, 64, 64, kind='deconv', expect=dict(wgs=32, ksteps=4)),
    'deep_groups2_1x1': spec(DEEP, 1, 16, 128, 64, 64, k=1, groups=2, expect=dict(wgs=32, ksteps=1)),
    'deep_s2d_copy': spec(DEEP, 1, 16, 128, 64, 64, k=1, s2d='copy', s_lo=8, expect=dict(ksteps=1)),
    'deep_s2d_copy_bn128_res': spec(DEEP, 1, 136, 128, 64, 128, bn=128, res=True, s2d='copy', expect=dict(wgs=136)),
    # ---- split-K: ks = min(cus // wgs, ksteps // 4, 16)
    'split2_wgs128_uneven': spec(SPLIT, 1, 64, 256, 64, 64, expect=dict(wgs=128, ks=2, ranges=[(0, 4), (4, 9)])),
    'split2_ksteps8': spec(SPLIT, 1, 16, 128, 512, 64, k=1, expect=dict(ksteps=8, ks=2)),
    'split3': spec(SPLIT, 1, 40, 256, 128, 64, expect=dict(wgs=80, ks=3)),
    'split4_uneven': spec(SPLIT, 1, 32, 256, 128, 64, expect=dict(wgs=64, ks=4, ranges=[(0, 4), (4, 9), (9, 13), (13, 18)])),
    'split5': spec(SPLIT, 1, 51, 128, 192, 64, expect=dict(wgs=51, ks=5)),
    'split6': spec(SPLIT, 1, 40, 128, 192, 64, expect=dict(wgs=40, ks=6)),
    'split8': spec(SPLIT, 1, 32, 128, 256, 64, expect=dict(wgs=32, ks=8)),
    'split9': spec(SPLIT, 1, 28, 128, 256, 64, expect=dict(wgs=28, ks=9)),
    'split16_bn128': spec(SPLIT, 1, 16, 128, 512, 128, bn=128, expect=dict(wgs=16, ks=16, ksteps=72)),
    'split_ragged_nt2': spec(SPLIT, 2, 13, 21, 256, 128, expect=dict(MT=5, NT=2, ks=9)),
    'split2_s2d_copy': spec(SPLIT, 1, 16, 128, 64, 64, s2d='copy', s_hi=64, expect=dict(ks=2)),
    # stride 2, residual, project folds (tap_dc), transposed-conv phases at the split counts of the product plans
    'split2_stride2': spec(SPLIT, 1, 32, 256, 64, 64, stride=2, expect=dict(wgs=16, ks=2)),
    'split3_stride2': spec(SPLIT, 1, 80, 512, 128, 64, stride=2, expect=dict(wgs=80, ks=3)),
    'split4_stride2': spec(SPLIT, 1, 64, 512, 128, 64, stride=2, expect=dict(wgs=64, ks=4)),
    'split6_stride2': spec(SPLIT, 1, 80, 256, 192, 64, stride=2, expect=dict(wgs=40, ks=6)),
    'split8_stride2': spec(SPLIT, 1, 64, 256, 256, 64, stride=2, expect=dict(wgs=32, ks=8)),
    'split2_res': spec(SPLIT, 1, 16, 128, 64, 64, res=True, expect=dict(ks=2)),
    'split3_res': spec(SPLIT, 1, 40, 256, 128, 64, res=True, expect=dict(ks=3)),
    'split4_res': spec(SPLIT, 1, 32, 256, 128, 64, res=True, expect=dict(ks=4)),
    'split6_res': spec(SPLIT, 1, 40, 128, 192, 64, res=True, expect=dict(ks=6)),
    'split8_res_bn128': spec(SPLIT, 1, 32, 128, 256, 128, bn=128, res=True, expect=dict(ks=8)),
    'split8_res': spec(SPLIT, 1, 32, 128, 256, 64, res=True, expect=dict(ks=8)),
    'split2_tapdc': spec(SPLIT, 1, 16, 128, 64, 64, kind='tapdc', ntaps=8, expect=dict(ksteps=8, ks=2)),
    'split3_tapdc': spec(SPLIT, 1, 16, 128, 64, 64, kind='tapdc', ntaps=13, expect=dict(ks=3, ranges=[(0, 4), (4, 8), (8, 13)])),
    'split4_tapdc': spec(SPLIT, 1, 16, 128, 64, 64, kind='tapdc', ntaps=19, expect=dict(ks=4)),
    'split6_tapdc': spec(SPLIT, 1, 40, 128, 64, 64, kind='tapdc', ntaps=27, expect=dict(ks=6)),
    'split8_tapdc': spec(SPLIT, 1, 32, 128, 64, 64, kind='tapdc', ntaps=38, expect=dict(ks=8)),
    'split2_deconv': spec(SPLIT, 1, 16, 128, 128, 64, kind='deconv', expect=dict(wgs=64, ks=2)),
    'split3_deconv': spec(SPLIT, 1, 16, 128, 192, 64, kind='deconv', expect=dict(wgs=64, ks=3)),
    'split4_deconv_nt2': spec(SPLIT, 1, 8, 128, 256, 128, kind='deconv', expect=dict(wgs=64, ks=4)),
    # ---- conv64_halo: the four epilogue templates, the ticket regimes (total 1 / 256 single; 257 / 258 / 259 / 768 tickets)
    'c64_plain_total1': spec(C64, 1, 8, 32, 64, 64, expect=dict(total=1, single=True)),
    'c64_res_total256': spec(C64, 4, 64, 256, 64, 64, res=True, expect=dict(total=256, single=True)),
    'c64_s2d_total257': spec(C64, 1, 8, 8224, 64, 64, s2d='copy', expect=dict(total=257, single=False, mod3=2)),
    'c64_res_s2d_total258': spec(C64, 2, 8, 4128, 64, 64, res=True, s2d='copy', s_lo=64, expect=dict(total=258, mod3=0, first_draw_busy=86)),
    'c64_total259_slices': spec(C64, 7, 296, 32, 64, 64, in_P=2, out_P=0, in_extra=64, out_lo=64, out_hi=8, expect=dict(total=259, mod3=1)),
    'c64_res_total768': spec(C64, 4, 96, 512, 64, 64, res=True, relu=False, expect=dict(total=768, first_draw_busy=256)),
    'c64_s2d_single': spec(C64, 1, 16, 64, 64, 64, s2d='copy', expect=dict(total=4, single=True)),
    'c64_res_s2d_single': spec(C64, 2, 16, 64, 64, 64, res=True, s2d='copy', expect=dict(total=8, single=True)),
    # ---- conv128_halo: cin x cout multiples of 128 with a residual; the same ticket boundaries
    'c128_total1': spec(C128, 1, 8, 32, 128, 128, expect=dict(total=1, single=True)),
    'c128_total256': spec(C128, 4, 64, 256, 128, 128, expect=dict(total=256, single=True)),
    'c128_total257': spec(C128, 1, 8, 8224, 128, 128, res=True, expect=dict(total=257, mod3=2)),
    'c128_total258': spec(C128, 1, 8, 4128, 128, 256, expect=dict(total=258, mod3=0)),
    'c128_total259_slices': spec(C128, 7, 296, 32, 128, 128, in_P=2, out_P=0, in_extra=64, out_lo=64, out_hi=8, expect=dict(total=259, mod3=1)),
    'c128_total768_res': spec(C128, 4, 96, 256, 128, 256, res=True, expect=dict(total=768, first_draw_busy=256)),
}
for _ci in (128, 256, 384, 512):
    for _co in (128, 256, 384):
        CASES['c128_cin%d_cout%d_res' % (_ci, _co)] = spec(C128, 1, 16, 64, _ci, _co, res=True, expect=dict(total=4 * _co // 128, single=True))
CASES.update({
    # ---- conv64s2_halo: input 2 Ho or 2 Ho - 1 rows / columns, the space-to-depth input at a non-zero channel base
    'c64s2_even_single': spec(C64S2, 2, 16, 64, 64, 128, stride=2, expect=dict(total=4, single=True)),
    'c64s2_odd_single': spec(C64S2, 2, 15, 63, 64, 128, stride=2, in_extra=64, out_lo=8, expect=dict(total=4, single=True)),
    'c64s2_even_tickets': spec(C64S2, 2, 128, 576, 64, 128, stride=2, expect=dict(total=288, single=False, mod3=0)),
    'c64s2_odd_tickets': spec(C64S2, 1, 2063, 63, 64, 128, stride=2, relu=False, expect=dict(total=258, single=False)),
    'c64s2_s2d_input_single': spec(C64S2, 1, 16, 128, 64, 128, stride=2, s2d='input', s_lo=64, s_hi=8, expect=dict(total=4, single=True)),
    'c64s2_s2d_input_tickets': spec(C64S2, 2, 128, 576, 64, 128, stride=2, s2d='input', s_lo=128, expect=dict(total=288, single=False)),
})


@pytest.mark.parametrize('name', list(CASES))
def test_conv128_route_and_regime(name):
    run_one(CASES[name], seed=sum(map(ord, name)))


def test_deep_ksplit1_is_bit_identical_to_one_stage():
    """conv_mfma.hip: the deep kernel with ksplit == 1 gives the same bits as conv_mfma_kernel.  One image as a B = 1 launch (240
    pixel tiles: deep, no split) and the same image as image 0 of a B = 2 launch (480 tiles: one-stage)."""
    H, W, cin, cout = 96, 320, 64, 128
    rng = np.random.default_rng(3)
    x = f16(rng.standard_normal((2, H, W, cin)))
    w = f16(rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    got = {}
    for B, route in ((1, DEEP), (2, OS)):
        assert cr.admit_mfma128(B * H * W, cin, cout, 9, 1, 128, cus=CUS)['route'] == route
        P = plan_mod.Plan(B, H * 4, W * 4)
        xt, yt = P.tensor(H, W, cin, 1), P.tensor(H, W, cout, 1)
        P.conv(xt, yt, w, b, relu=True, name='t')
        P.ops[-1].update(variant=_lib.CONV_MFMA128, bn_tile=128)
        img = np.zeros((B, H + 2, W + 2, cin), np.float16)
        img[:, 1:-1, 1:-1] = x[:B]
        R = plan_mod.RealizedPlan(P, 0)
        try:
            assert [cr.route_of(n) for n in R.kernel_names()] == [route], R.kernel_names()
            raw_write(R, xt, img)
            outs = [torch.zeros(16, device='cuda') for _ in range(4)]
            R.forward(torch.cuda.current_stream().cuda_stream, outs[0].data_ptr(), [o.data_ptr() for o in outs])
            torch.cuda.synchronize()
            got[route] = raw_read(R, yt)[0]
        finally:
            R.close()
    np.testing.assert_array_equal(got[DEEP].view(np.uint16), got[OS].view(np.uint16))


# ---- split-K ops of different (wgs, ks, groups) and halo ops in ONE plan: the split ops share the arrival counters (re-armed
# by each tile's last arrival) and one fp32 slab that grows as larger split ops are recorded (earlier ops' pointers are
# patched); the halo ops draw tickets.  Regime 0 has the smallest slab and is recorded first.
CHAIN = {
    'split2_deconv_groups4': spec(SPLIT, 1, 16, 128, 128, 64, kind='deconv', expect=dict(wgs=64, ks=2, slab_floats=64 * 2 * 8192)),
    'split16_wgs16': spec(SPLIT, 1, 16, 128, 512, 64, expect=dict(wgs=16, ks=16, slab_floats=16 * 16 * 8192)),
    'split3_wgs80_res': spec(SPLIT, 1, 40, 256, 128, 64, res=True, expect=dict(wgs=80, ks=3, slab_floats=80 * 3 * 8192)),
    'split5_tapdc': spec(SPLIT, 1, 51, 128, 64, 64, kind='tapdc', ntaps=20, expect=dict(wgs=51, ks=5)),
    'c64_tickets': spec(C64, 1, 8, 8224, 64, 64, expect=dict(total=257, single=False)),
    'c128_single': spec(C128, 1, 16, 64, 128, 256, res=True, expect=dict(total=8, single=True)),
}


def test_conv128_counter_chain():
    keys = list(CHAIN)
    slabs = [mirror(CHAIN[k])['slab_floats'] for k in keys[:4]]
    assert slabs[0] < min(slabs[1:]), slabs
    order = every_pair_order(len(keys))
    pairs = {(a, b) for a, b in zip(order, order[1:])}
    assert len(order) == len(keys) * (len(keys) - 1) + 1 and len(pairs) == len(keys) * (len(keys) - 1) and order[0] == 0
    for sp in CHAIN.values():
        check_regime(sp)
    P = plan_mod.Plan(1, 64 * 4, 8224 * 4)
    rng = np.random.default_rng(5)
    convs = [Conv(P, CHAIN[keys[i]], rng) for i in order]
    run_plan(P, convs, replays=3, graph=True)


def test_nchw_output_group_offsets_and_residual_are_refused():
    """An fp32 NCHW slot holds cout * groups channels: admission refuses a group whose channels leave it or overlap another
    group's, and a residual (the NCHW epilogue adds none); a refusal records nothing."""
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.rtm3d_ctx_create(0, ctypes.byref(ctx)))
    try:
        def tensor(C):
            tid = ctypes.c_int()
            _lib.check(lib.rtm3d_tensor_create(ctx, 1, 8, 16, C, 1, ctypes.byref(tid)))
            return tid.value

        def blob(nbytes):
            arr = np.zeros(nbytes, np.uint8)
            bid = ctypes.c_int()
            _lib.check(lib.rtm3d_blob_create(ctx, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, ctypes.byref(bid)))
            return bid.value

        def n_ops():
            n = 0
            while lib.rtm3d_op_info(ctx, n, None, None, None) == 0:
                n += 1
            return n
        t_in, t_res = tensor(128), tensor(64)
        d = _lib.ConvDesc()
        d.in_tensor, d.out_tensor, d.res_tensor, d.s2d_tensor, d.softmax_stat_slot = t_in, -1, -1, 0, -1
        d.Hm, d.Wm, d.in_stride, d.out_scale, d.cin, d.cout, d.groups, d.ntaps = 8, 16, 1, 1, 64, 3, 2, 1
        d.in_coff[1] = 64
        d.kernel, d.bn_tile, d.out_nchw_f32, d.out_H, d.out_W = _lib.CONV_MFMA128, 16, 1, 8, 16
        d.w_blob, d.bias_blob = blob(2 * 16 * 64 * 2), blob(2 * 16 * 4)
        for offs, what in (((0, 0), b'overlap'), ((0, 2), b'overlap'), ((0, 4), b'outside'),
                           ((-3, 3), b'outside'), ((1, 3), b'overlap')):
            d.out_coff[0], d.out_coff[1] = offs
            n = n_ops()
            assert lib.rtm3d_op_conv(ctx, ctypes.byref(d)) != 0 and what in lib.rtm3d_last_error(), (offs, lib.rtm3d_last_error())
            assert n_ops() == n
        for offs in ((0, 3), (3, 0)):
            d.out_coff[0], d.out_coff[1] = offs
            assert lib.rtm3d_op_conv(ctx, ctypes.byref(d)) == 0, lib.rtm3d_last_error()
        d.groups, d.cout, d.out_coff[0], d.res_tensor = 1, 64, 0, t_res
        d.w_blob, d.bias_blob = blob(64 * 64 * 2), blob(64 * 4)
        n = n_ops()
        assert lib.rtm3d_op_conv(ctx, ctypes.byref(d)) != 0 and b'residual' in lib.rtm3d_last_error(), lib.rtm3d_last_error()
        assert n_ops() == n
    finally:
        lib.rtm3d_ctx_destroy(ctx)
