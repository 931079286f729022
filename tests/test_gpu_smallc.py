"""GPU (-m gpu): the register-direct small-channel conv kernels (conv_smallc.hip: conv_smallc_kernel, conv_smallc_rows_kernel,
nchw_to_nhwc4_kernel) over every launch instance and every edge of its own, against a numpy float64 reference.

Every case first asserts the op name and the regime the host mirror (tests/smallc_routes.py) gives for it.  Then one op runs
with its input a channel slice of a wider tensor and its output a slice with neighbours; every written value is poisoned with
NaN, the other channels hold a sentinel, the border is zero, and the whole padded images of both tensors are read back raw.

Two kinds of numeric check:
- exact (the default): integer inputs (|x| <= 40) and weights and biases that are multiples of 2^-9, so that in units of
  2^-9 the sum of |w x| plus |bias| of every output stays below 2^24 (tests/test_smallc_routes.py checks that from the
  reference alone).  Every partial sum is then an fp32 number whatever the order, so the kernel's fp32 value is the exact
  result and rounds ONCE to fp16, like the float64 reference: the comparison is bit for bit.  Weights differ per tap, input
  channel and output channel and inputs per pixel, so a wrong tap, a swapped channel half or lane group changes the bits.
  Every input pixel no tap reads, every channel outside the input slice and the fourth image channel of the cin = 4 cases
  (zero weights) hold +-30000: none may reach an output.  For cin = 4 that covers the pixel right of tap (ky, 6), which the
  kernel loads with the packer's zero weights.
- random: Gaussian operands rounded to fp16; per output |got - fp16(ref)| <= ulp16(ref) + K 2^-24 sum |w||x| with K the
  products the instance sums per output (32 per MFMA K-step, <= 288): one fp16 rounding plus the fp32 accumulation bound
  (K - 1 additions and the bias addition, each within 2^-24 relative of a partial sum that sum |w||x| bounds; fp16 products
  are exact in fp32).  The bound comes from the reference operands; the largest observed ratio per instance is recorded.

Instances and how a descriptor reaches them (launch_conv_smallc): the stride-1 16 -> 16 conv with the plain 3x3 taps is
packed by filter rows (6 K-steps) and runs the vertical-walk kernel; a stride-2 or dilated 16 -> 16 conv keeps the 5-step
packing and runs conv_smallc_kernel<16,1,5,8>.  conv_smallc_kernel<4,1,7,8> (4 -> 16 off the vertical walk) is reached by a
stride-2 7x7 4 -> 16 conv, which Plan.conv / Plan.stem_mfma record as they do the ResNet stem; no product plan has one.
out_scale = 2 reaches kernel 3 only through the C ABI (Plan.deconv records four groups, which kernel 3 refuses) and is not
run here.  CASES is importable without a GPU: tests/test_smallc_routes.py checks it against the mirror, against the product
plans' regimes and for the exactness condition."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import plan as plan_mod, _lib                                         # noqa: E402
from tests import smallc_routes as sr                                                 # noqa: E402
from tests.conv_harness import SENTINEL, every_pair_order, f16, raw_read, raw_write   # noqa: E402
from tests.util import record_measurement                                             # noqa: E402

BIG = 30000.0           # fp16-exact; what no output may see
WQ = 2.0 ** -9          # quantum of the exact cases' weights and biases (inputs are integers)


def spec(B, H, W, cin, cout, k=None, stride=1, dil=1, taps=None, relu=True, mode='exact', ramp=False, in_lo=0, in_hi=0, in_P=None,
         out_lo=0, out_hi=0, out_P=1, expect=None):
    """One conv on B images of an H x W input map.  taps: an explicit (dy, dx) list (Plan.conv_taps, stride 1) instead of the
    k x k / dilation `dil` grid.  The input is channels [in_lo, in_lo + cin) of a tensor with border in_P, the output channels
    [out_lo, out_lo + cout) of a tensor with border out_P."""
    k = k or (7 if cin == 4 else 3)
    if taps is None:
        pad = dil * (k - 1) // 2
        tl = [(ky * dil - pad, kx * dil - pad) for ky in range(k) for kx in range(k)]
    else:
        assert stride == 1
        tl = list(taps)
    reach = max(max(abs(dy), abs(dx)) for dy, dx in tl)
    if in_P is None:
        in_P = max(reach, 4 if cin == 4 else 1)
    assert in_P >= reach and (cin != 4 or (in_lo == 0 and in_hi == 0))
    rows_packing = cin == 16 and cout == 16 and stride == 1 and tl == plan_mod._TAPS3
    return dict(B=B, H=H, W=W, cin=cin, cout=cout, k=k, stride=stride, dil=dil, explicit=taps is not None, taps=tl, relu=relu, mode=mode,
                ramp=ramp, in_lo=in_lo, in_hi=in_hi, in_P=in_P, out_lo=out_lo, out_hi=out_hi, out_P=out_P, rows_packing=rows_packing,
                Hm=(H - 1) // stride + 1, Wm=(W - 1) // stride + 1, expect=expect or {})


def mirror(sp):
    return sr.launch(sp['B'], sp['H'], sp['W'], sp['cin'], sp['cout'], len(sp['taps']), sp['stride'], 1, sp['rows_packing'])


def regime(sp):
    return sr.regime_key(mirror(sp), sp['relu'])


def check_regime(sp):
    r = mirror(sp)
    for key, want in sp['expect'].items():
        assert r[key] == want, (key, r[key], want, r)
    return r


def operands(sp, seed):
    """Host operands of a case: the whole padded input image (B, Hp, Wp, C) fp16, weights (taps, cout, cin) and bias (cout)
    fp32.  Pure numpy: the CPU suite computes the exactness condition from them."""
    rng = np.random.default_rng(seed)
    B, H, W, cin, cout, Pi, s = sp['B'], sp['H'], sp['W'], sp['cin'], sp['cout'], sp['in_P'], sp['stride']
    C, nt = sp['in_lo'] + cin + sp['in_hi'], len(sp['taps'])
    Hp, Wp = H + 2 * Pi, W + 2 * Pi
    if sp['mode'] == 'exact':
        if sp['ramp']:          # an integer ramp in y: a stale or doubly shifted operand row changes every output
            yy, xx, cc = np.meshgrid(np.arange(Hp), np.arange(Wp), np.arange(C), indexing='ij')
            x = np.broadcast_to((yy - Hp // 2) + (xx + cc) % 3, (B, Hp, Wp, C)).astype(np.float64)
        else:
            x = rng.integers(-15, 16, (B, Hp, Wp, C)).astype(np.float64)
        kk, co = np.arange(nt * cin).reshape(nt, 1, cin), np.arange(cout).reshape(1, cout, 1)
        w = (((kk * 67 + co * 29) % 1021) - 510) * WQ
        b = ((np.arange(cout) * 37) % 201 - 100) * (32 * WQ)
    else:
        x = rng.standard_normal((B, Hp, Wp, C))
        w = rng.standard_normal((nt, cout, cin)) / np.sqrt(nt * cin)
        b = rng.standard_normal(cout)
    if cin == 4:                # three image channels: the fourth has zero weights and must not be seen
        w[:, :, 3] = 0.0
        x[..., 3] = BIG
    used = np.zeros((Hp, Wp), bool)
    for dy, dx in sp['taps']:
        used[Pi + dy:Pi + dy + (sp['Hm'] - 1) * s + 1:s, Pi + dx:Pi + dx + (sp['Wm'] - 1) * s + 1:s] = True
    x[:, ~used] = BIG
    x[..., :sp['in_lo']] = BIG
    x[..., sp['in_lo'] + cin:] = -BIG
    x16, w16 = f16(x), f16(w).astype(np.float32)
    if sp['mode'] == 'exact':
        assert np.array_equal(x16.astype(np.float64), x) and np.array_equal(w16.astype(np.float64), w)
    return {'x': x16, 'w': w16, 'b': b.astype(np.float32)}


def reference(sp, ops, absolute=False):
    """float64 result (B, Hm, Wm, cout) of the taps on the operands, before ReLU; absolute: sum |w||x| (no bias)."""
    Pi, s, Hm, Wm, lo = sp['in_P'], sp['stride'], sp['Hm'], sp['Wm'], sp['in_lo']
    x = ops['x'][..., lo:lo + sp['cin']].astype(np.float64)
    w, b = ops['w'].astype(np.float64), ops['b'].astype(np.float64)
    if absolute:
        x, w, b = np.abs(x), np.abs(w), np.zeros_like(b)
    acc = np.broadcast_to(b, (sp['B'], Hm, Wm, sp['cout'])).copy()
    for t, (dy, dx) in enumerate(sp['taps']):
        acc += x[:, Pi + dy:Pi + dy + (Hm - 1) * s + 1:s, Pi + dx:Pi + dx + (Wm - 1) * s + 1:s] @ w[t].T
    return acc


def exactness_units(sp, ops):
    """Largest sum |w x| + |bias| over the outputs, in units of the input quantum (1) times the weight quantum (WQ)."""
    return float((reference(sp, ops, absolute=True) + np.abs(ops['b'].astype(np.float64))).max() / WQ)


def ulp16(r):
    """Spacing of fp16 at |r| (float64 array)."""
    e = np.floor(np.log2(np.maximum(np.abs(r), 2.0 ** -14)))
    return 2.0 ** (e - 10)


class SmallC(object):
    """One kernel-3 op of a plan with tensors of its own."""

    def __init__(self, P, sp, seed):
        self.sp, self.seed = sp, seed
        cin, cout = sp['cin'], sp['cout']
        assert P.B == sp['B']
        self.xt = P.tensor(sp['H'], sp['W'], sp['in_lo'] + cin + sp['in_hi'], sp['in_P'])
        self.yt = P.tensor(sp['Hm'], sp['Wm'], sp['out_lo'] + cout + sp['out_hi'], sp['out_P'])
        xs, ys = P.sub(self.xt, sp['in_lo'], cin), P.sub(self.yt, sp['out_lo'], cout)
        self.ops = operands(sp, seed)
        w, b, name = self.ops['w'], self.ops['b'], 't%d' % len(P.ops)
        if sp['explicit']:
            P.conv_taps([xs], [ys], [w.transpose(1, 2, 0)], [b], sp['taps'], sp['Hm'], sp['Wm'], relu=sp['relu'], name=name)
        else:
            k = sp['k']
            P.conv(xs, ys, w.transpose(1, 2, 0).reshape(cout, cin, k, k), b, stride=sp['stride'], dil=sp['dil'], relu=sp['relu'], name=name)
        assert np.array_equal(P.ops[-1]['w'][0], w) and P.ops[-1]['taps'][0] == sp['taps']
        self.ref = None

    def upload(self, R):
        raw_write(R, self.xt, self.ops['x'])

    def poison(self, R):
        sp, Po = self.sp, self.sp['out_P']
        img = np.zeros((sp['B'], sp['Hm'] + 2 * Po, sp['Wm'] + 2 * Po, self.yt.C), np.float16)
        img[:, Po:Po + sp['Hm'], Po:Po + sp['Wm']] = SENTINEL
        img[:, Po:Po + sp['Hm'], Po:Po + sp['Wm'], sp['out_lo']:sp['out_lo'] + sp['cout']] = np.nan
        raw_write(R, self.yt, img)

    def read(self, R):
        return {'y': raw_read(R, self.yt), 'x': raw_read(R, self.xt)}

    def check(self, got, label=''):
        sp, Po = self.sp, self.sp['out_P']
        assert np.array_equal(got['x'].view(np.uint16), self.ops['x'].view(np.uint16)), 'the input tensor was written'
        y = got['y']
        border = np.ones(y.shape[:3], bool)
        border[:, Po:Po + sp['Hm'], Po:Po + sp['Wm']] = False
        assert not y.view(np.uint16)[border].any(), 'the output border was written'
        inner = y[:, Po:Po + sp['Hm'], Po:Po + sp['Wm']]
        lo, hi = sp['out_lo'], sp['out_lo'] + sp['cout']
        outside = np.concatenate([inner[..., :lo], inner[..., hi:]], -1)
        assert (outside.view(np.uint16) == SENTINEL.view(np.uint16)).all(), 'channels outside the output slice were written'
        val = np.ascontiguousarray(inner[..., lo:hi])
        assert np.isfinite(val).all(), '%d output values never written (NaN poison)' % int((~np.isfinite(val)).sum())
        if self.ref is None:
            self.ref = reference(sp, self.ops)
        ref = np.maximum(self.ref, 0.0) if sp['relu'] else self.ref
        ref16 = ref.astype(np.float16)
        if not sp['relu']:
            assert (ref16 < 0).mean() > 0.2, 'the case has no negative results to pass through'
        if sp['mode'] == 'exact':
            bad = val.view(np.uint16) != ref16.view(np.uint16)
            first = tuple(np.argwhere(bad)[0]) if bad.any() else None
            assert not bad.any(), '%d of %d outputs differ in bits; first at (n, y, x, c) = %s: got %r, expected %r' % (
                int(bad.sum()), bad.size, first, float(val[first]), float(ref16[first]))
            return 0.0
        K = 32 * mirror(sp)['ksteps']
        assert K <= 288
        bound = ulp16(ref) + K * 2.0 ** -24 * reference(sp, self.ops, absolute=True)
        ratio = np.abs(val.astype(np.float64) - ref16.astype(np.float64)) / bound
        worst = float(ratio.max())
        print('%s: largest |got - ref16| / bound = %.4f' % (label, worst))
        assert worst <= 1.0, (label, worst, tuple(np.unravel_index(ratio.argmax(), ratio.shape)))
        return worst


def _forward(R, convs):
    for c in convs:
        c.poison(R)
    xin = torch.zeros(16, device='cuda')
    outs = [torch.zeros(16, device='cuda') for _ in range(4)]
    R.forward(torch.cuda.current_stream().cuda_stream, xin.data_ptr(), [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    return [c.read(R) for c in convs]


def run_plan(P, convs, replays=0, label=''):
    """Record P, assert every op's name, run one poisoned forward and check every output; `replays` more forwards, each
    re-poisoned, must give the same bits.  Returns the first forward's raw images and the random cases' ratios."""
    R = plan_mod.RealizedPlan(P, 0)
    try:
        assert R.kernel_names() == [sr.op_name(c.sp['cin']) for c in convs], R.kernel_names()
        for c in convs:
            c.upload(R)
        first = _forward(R, convs)
        ratios = [c.check(got, label) for c, got in zip(convs, first)]
        for _ in range(replays):
            for a, b in zip(first, _forward(R, convs)):
                for key in a:
                    np.testing.assert_array_equal(a[key].view(np.uint16), b[key].view(np.uint16))
        return first, ratios
    finally:
        R.close()


def case_seed(name):
    return sum(map(ord, name))


def run_one(name, sp):
    check_regime(sp)
    P = plan_mod.Plan(sp['B'], sp['H'], sp['W'])
    return run_plan(P, [SmallC(P, sp, case_seed(name))], label=name)


T4_64, T4_16, T16_16, T16_32, T32_64, T32_64P = (('tile',) + v[0] for v in (sr.TILE_INSTANCES[k] for k in (
    (4, 64, 49), (4, 16, 49), (16, 16, 9), (16, 32, 9), (32, 64, 9), (32, 64, 1))))
R4_16, R16_16 = ('rows',) + sr.ROWS_INSTANCES[(4, 16, 49)], ('rows',) + sr.ROWS_INSTANCES[(16, 16, 9)]
# nine taps in no grid: distinct pixels within +-3, neither row-major nor equally spaced
SCATTER9 = [(-3, 2), (0, 0), (2, -3), (-1, -2), (3, 3), (1, 1), (-2, 0), (0, -1), (2, 2)]


def _tile(inst, **kw):
    return dict(instance=inst, **kw)


CASES = {
    # ---- conv_smallc_kernel<4,4,7,8>: ResNet conv1 (7x7 stride 2, 4 -> 64), 16-byte stores
    'c1_product_rows_b2': spec(2, 32, 1280, 4, 64, stride=2, expect=_tile(T4_64, M=20480, m_mod16=0, ntiles_mod8=0, idle_waves=0,
                                                                          row_straddles=0, image_straddles=0, grid=(40, 1), store_bytes=16)),
    'c1_odd_h_w': spec(1, 37, 51, 4, 64, stride=2, relu=False, in_P=6, out_P=0, out_lo=8, out_hi=8,
                       expect=_tile(T4_64, Hm=19, Wm=26, M=494, m_mod16=14, ntiles=31, ntiles_mod8=7, idle_waves=0, grid=(1, 1))),
    'c1_most_waves_return': spec(1, 8, 16, 4, 64, stride=2, expect=_tile(T4_64, M=32, ntiles=2, idle_waves=3, grid=(1, 1))),
    'c1_image_straddle_coff8_c72': spec(3, 10, 12, 4, 64, stride=2, out_P=2, out_lo=8,
                                        expect=_tile(T4_64, M=90, m_mod16=10, ntiles=6, image_straddles=2, store_bytes=16)),
    'c1_random': spec(2, 33, 70, 4, 64, stride=2, mode='random',
                      expect=_tile(T4_64, Hm=17, Wm=35, M=1190, m_mod16=6, ntiles=75, ntiles_mod8=3, idle_waves=2, grid=(3, 1))),
    # ---- conv_smallc_kernel<4,1,7,8>: 7x7 stride 2, 4 -> 16 (8-byte stores into a 28-channel tensor)
    'stem16_s2': spec(2, 21, 30, 4, 16, stride=2, out_lo=8, out_hi=4, expect=_tile(T4_16, Hm=11, Wm=15, M=330, m_mod16=10, store_bytes=8)),
    'stem16_s2_no_relu': spec(1, 32, 64, 4, 16, stride=2, relu=False, in_P=5, out_P=0, expect=_tile(T4_16, M=512, m_mod16=0, idle_waves=0)),
    'stem16_s2_random': spec(3, 9, 23, 4, 16, stride=2, mode='random', relu=False, expect=_tile(T4_16, M=180, image_straddles=2)),
    # ---- conv_smallc_rows_kernel<4,1,7,1,32>: DLA base_layer (7x7 stride 1, 4 -> 16)
    'rows4_h20_w16': spec(1, 20, 16, 4, 16, expect=dict(instance=R4_16, tiles_x=1, strips_y=1, last_rows=20, nwaves=1, nwaves_mod4=1, grid=(1, 1))),
    'rows4_h32_w17_b2': spec(2, 32, 17, 4, 16, relu=False, out_P=0, out_lo=8, out_hi=4,
                             expect=dict(instance=R4_16, tiles_x=2, w_mod16=1, strips_y=1, h_mod32=0, last_rows=32, nwaves=4, nwaves_mod4=0)),
    'rows4_h33_w40': spec(1, 33, 40, 4, 16, in_P=6, out_P=2,
                          expect=dict(instance=R4_16, tiles_x=3, w_mod16=8, strips_y=2, h_mod32=1, last_rows=1, nwaves=6, nwaves_mod4=2)),
    'rows4_h70_w16': spec(1, 70, 16, 4, 16, ramp=True, expect=dict(instance=R4_16, strips_y=3, last_rows=6, nwaves=3, nwaves_mod4=3)),
    'rows4_h64_w32_full': spec(1, 64, 32, 4, 16, expect=dict(instance=R4_16, w_mod16=0, h_mod32=0, nwaves=4, nwaves_mod4=0, grid=(1, 1))),
    'rows4_h40_w16_b2': spec(2, 40, 16, 4, 16, relu=False, expect=dict(instance=R4_16, strips_y=2, last_rows=8, nwaves=4, nwaves_mod4=0)),
    'rows4_random': spec(2, 70, 40, 4, 16, mode='random', expect=dict(instance=R4_16, nwaves=18, nwaves_mod4=2, grid=(5, 1))),
    # ---- conv_smallc_rows_kernel<16,1,3,2,32>: DLA level0 (3x3 stride 1, 16 -> 16, 6-step packing)
    'rows16_h20_w16': spec(1, 20, 16, 16, 16, ramp=True, in_lo=16, in_hi=8, expect=dict(instance=R16_16, nwaves=1, nwaves_mod4=1, last_rows=20)),
    'rows16_h32_w17_b2': spec(2, 32, 17, 16, 16, relu=False, in_P=3, out_P=0, out_lo=8, out_hi=4,
                              expect=dict(instance=R16_16, w_mod16=1, h_mod32=0, nwaves=4, nwaves_mod4=0)),
    'rows16_h33_w40': spec(1, 33, 40, 16, 16, ramp=True, in_hi=16, out_P=2,
                           expect=dict(instance=R16_16, w_mod16=8, h_mod32=1, last_rows=1, nwaves=6, nwaves_mod4=2)),
    'rows16_h70_w16_ramp': spec(1, 70, 16, 16, 16, ramp=True, in_lo=8, expect=dict(instance=R16_16, strips_y=3, last_rows=6, nwaves_mod4=3)),
    'rows16_h64_w32_full': spec(1, 64, 32, 16, 16, expect=dict(instance=R16_16, w_mod16=0, h_mod32=0, nwaves_mod4=0)),
    'rows16_h40_w16_b2': spec(2, 40, 16, 16, 16, ramp=True, in_hi=8, expect=dict(instance=R16_16, strips_y=2, last_rows=8, nwaves=4, nwaves_mod4=0)),
    'rows16_random': spec(2, 70, 40, 16, 16, mode='random', in_lo=8, expect=dict(instance=R16_16, nwaves=18, nwaves_mod4=2)),
    # ---- conv_smallc_kernel<16,1,5,8>: 16 -> 16 in the 5-step packing (stride 2, or taps the vertical walk does not take)
    'c16_s2': spec(2, 21, 30, 16, 16, stride=2, in_lo=8, in_hi=8, out_lo=8, out_hi=4, expect=_tile(T16_16, M=330, m_mod16=10, store_bytes=8)),
    'c16_dil2': spec(1, 20, 24, 16, 16, dil=2, relu=False, in_P=3, out_P=0, expect=_tile(T16_16, M=480, ntiles=30, ntiles_mod8=6, row_straddles=10)),
    'c16_s2_random': spec(1, 64, 64, 16, 16, stride=2, mode='random', expect=_tile(T16_16, M=1024, m_mod16=0, idle_waves=0, grid=(2, 1))),
    # ---- conv_smallc_kernel<16,2,5,8>: DLA level1 (3x3 stride 2, 16 -> 32), 16-byte stores
    'c32_s2_full': spec(1, 32, 64, 16, 32, stride=2, expect=_tile(T16_32, M=512, m_mod16=0, ntiles_mod8=0, idle_waves=0, row_straddles=0, store_bytes=16)),
    'c32_s2_ragged_coff8_c40': spec(2, 21, 30, 16, 32, stride=2, relu=False, in_lo=16, in_P=2, out_P=0, out_lo=8,
                                    expect=_tile(T16_32, M=330, m_mod16=10, ntiles=21, ntiles_mod8=5, idle_waves=1)),
    'c32_scatter_taps': spec(1, 12, 20, 16, 32, taps=SCATTER9, in_P=3, expect=_tile(T16_32, M=240, ntiles=15)),
    'c32_dil2_s2': spec(1, 18, 26, 16, 32, stride=2, dil=2, out_P=2, expect=_tile(T16_32, M=117, m_mod16=5)),
    'c32_random': spec(3, 9, 23, 16, 32, stride=2, mode='random', in_hi=8, expect=_tile(T16_32, M=180, image_straddles=2)),
    # ---- conv_smallc_kernel<32,2,9,8>, grid.y = 2: DLA level2 tree1.conv1 (3x3 stride 2, 32 -> 64)
    'c64_s2_full': spec(1, 32, 64, 32, 64, stride=2, expect=_tile(T32_64, M=512, idle_waves=0, grid=(1, 2), grid_y=2, store_bytes=16)),
    'c64_s2_narrow_map': spec(1, 32, 16, 32, 64, stride=2, expect=_tile(T32_64, M=128, m_mod16=0, ntiles_mod8=0, idle_waves=3, row_straddles=8)),
    'c64_s2_ragged_coff8_c72': spec(2, 21, 30, 32, 64, stride=2, relu=False, in_lo=8, in_hi=8, out_P=0, out_lo=8,
                                    expect=_tile(T32_64, M=330, ntiles=21, grid=(1, 2))),
    'c64_dil2': spec(1, 12, 20, 32, 64, dil=2, in_P=3, out_P=2, expect=_tile(T32_64, M=240, ntiles=15, ntiles_mod8=7)),
    'c64_scatter_taps': spec(2, 7, 9, 32, 64, taps=SCATTER9, relu=False, expect=_tile(T32_64, M=126, image_straddles=1)),
    'c64_random': spec(1, 66, 70, 32, 64, stride=2, mode='random', expect=_tile(T32_64, M=1155, m_mod16=3, ntiles=73, grid=(3, 2))),
    # ---- conv_smallc_kernel<32,4,1,8>: DLA level2 project (1x1, 32 -> 64, no ReLU), two swapped tile pairs
    'proj_full': spec(1, 16, 32, 32, 64, k=1, relu=False, expect=_tile(T32_64P, M=512, m_mod16=0, ntiles_mod8=0, idle_waves=0, store_bytes=16)),
    'proj_narrow_map': spec(1, 16, 8, 32, 64, k=1, relu=False, in_P=0, expect=_tile(T32_64P, M=128, idle_waves=3, row_straddles=8)),
    'proj_image_straddle_coff8_c72': spec(3, 5, 6, 32, 64, k=1, in_lo=32, out_lo=8, out_P=2,
                                          expect=_tile(T32_64P, M=90, m_mod16=10, ntiles=6, image_straddles=2)),
    'proj_ragged': spec(2, 19, 26, 32, 64, k=1, relu=False, in_hi=8, out_P=0, out_hi=8, expect=_tile(T32_64P, M=988, m_mod16=12, ntiles=62, ntiles_mod8=6)),
    'proj_random': spec(2, 17, 35, 32, 64, k=1, mode='random', relu=False, expect=_tile(T32_64P, M=1190, ntiles=75, idle_waves=2)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_smallc_instance_and_regime(name):
    sp = CASES[name]
    _, ratios = run_one(name, sp)
    if sp['mode'] == 'random':
        inst = '%s<%s>' % (mirror(sp)['instance'][0], ','.join(map(str, mirror(sp)['instance'][1:])))
        record_measurement('smallc_random_error', '%s %s' % (inst, name), ratios[0])


# ---- every instance next to every other in ONE context: the kernels keep no state between launches (no tickets, no counters),
# so the chain and a replay of it must give each case's own bits
CHAIN = {
    't4_64': spec(2, 10, 12, 4, 64, stride=2, out_lo=8, expect=_tile(T4_64)),
    't4_16': spec(2, 9, 13, 4, 16, stride=2, relu=False, expect=_tile(T4_16)),
    'r4_16': spec(2, 33, 17, 4, 16, expect=dict(instance=R4_16, last_rows=1)),
    'r16_16': spec(2, 33, 17, 16, 16, ramp=True, in_lo=8, expect=dict(instance=R16_16, last_rows=1)),
    't16_16': spec(2, 9, 13, 16, 16, stride=2, expect=_tile(T16_16)),
    't16_32': spec(2, 9, 13, 16, 32, stride=2, relu=False, expect=_tile(T16_32)),
    't32_64': spec(2, 9, 13, 32, 64, stride=2, expect=_tile(T32_64, grid_y=2)),
    't32_64p': spec(2, 5, 7, 32, 64, k=1, relu=False, expect=_tile(T32_64P)),
}


def test_smallc_chain_carries_no_state():
    keys = list(CHAIN)
    assert {mirror(CHAIN[k])['instance'] for k in keys} == set(sr.INSTANCES)
    order = every_pair_order(len(keys))
    pairs = {(a, b) for a, b in zip(order, order[1:])}
    assert len(order) == len(keys) * (len(keys) - 1) + 1 and len(pairs) == len(keys) * (len(keys) - 1)
    alone = {k: run_one(k, CHAIN[k])[0][0] for k in keys}
    P = plan_mod.Plan(2, 64, 64)
    convs = [SmallC(P, CHAIN[keys[i]], case_seed(keys[i])) for i in order]
    first, _ = run_plan(P, convs, replays=1, label='chain')
    for i, got in zip(order, first):
        np.testing.assert_array_equal(got['y'].view(np.uint16), alone[keys[i]]['y'].view(np.uint16))


# fp32 values whose fp16 rounding is decided by ties and range ends (numpy rounds to nearest, ties to even)
_TIES = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20,
                  2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25, 65504.0, 65519.0,
                  65520.0, -65520.0, 65504.0 * (1 + 2.0 ** -11), -65504.0 * (1 + 2.0 ** -11), 0.0, -0.0, 1e-30, 3.0e38], np.float32)


@pytest.mark.parametrize('B,H,W,border', [(3, 5, 7, 4), (1, 33, 17, 6), (2, 16, 16, 4)])
def test_input_nhwc4(B, H, W, border):
    """rtm3d_op_input_nhwc4: fp32 NCHW image -> NHWC4 fp16, bit for bit numpy's rounding; fourth channel zero, border untouched."""
    m = sr.nchw_to_nhwc4(B, H, W)
    assert m['idle'] == {(3, 5, 7): 151, (1, 33, 17): 207, (2, 16, 16): 0}[(B, H, W)]
    rng = np.random.default_rng(B * 1000 + H)
    img = (rng.standard_normal((B, 3, H, W)) * 4).astype(np.float32)
    flat = img.reshape(-1)
    where = rng.permutation(flat.size)[:3 * len(_TIES)]
    flat[where] = np.tile(_TIES, 3)
    P = plan_mod.Plan(B, H, W)
    x4 = P.tensor(H, W, 4, border)
    P.input_nhwc4(x4)
    R = plan_mod.RealizedPlan(P, 0)
    try:
        assert R.kernel_names() == ['nchw_f32_to_nhwc4_f16'], R.kernel_names()
        pre = np.full((B, H + 2 * border, W + 2 * border, 4), SENTINEL, np.float16)
        pre[:, border:border + H, border:border + W] = np.nan
        raw_write(R, x4, pre)
        d_in = torch.from_numpy(img).cuda()
        outs = [torch.zeros(16, device='cuda') for _ in range(4)]
        R.forward(torch.cuda.current_stream().cuda_stream, d_in.data_ptr(), [o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        got = raw_read(R, x4)
    finally:
        R.close()
    with np.errstate(over='ignore'):
        want = pre.copy()
        want[:, border:border + H, border:border + W, :3] = img.transpose(0, 2, 3, 1).astype(np.float16)
        want[:, border:border + H, border:border + W, 3] = 0.0
    assert np.isinf(want[:, border:-border, border:-border, :3]).any() and (want.view(np.uint16) == 0x8000).any()
    bad = got.view(np.uint16) != want.view(np.uint16)
    assert not bad.any(), (int(bad.sum()), [tuple(i) for i in np.argwhere(bad)[:4]])


def test_smallc_refusals_are_named_and_record_nothing():
    """admit_smallc through the C ABI: every descriptor kernel 3 cannot run is refused with its reason and records nothing,
    the tap geometries the vertical-walk and cin = 4 instances do not honour among them."""
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.rtm3d_ctx_create(0, ctypes.byref(ctx)))
    try:
        def tensor(H, W, C, pad):
            tid = ctypes.c_int()
            _lib.check(lib.rtm3d_tensor_create(ctx, 1, H, W, C, pad, ctypes.byref(tid)))
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

        def conv(t_i, t_o, cin, cout, k=3, stride=1, dil=1, ksteps=None, taps=None, bbytes=None, **fields):
            d = _lib.ConvDesc()
            d.in_tensor, d.out_tensor, d.res_tensor, d.s2d_tensor, d.softmax_stat_slot = t_i, t_o, -1, 0, -1
            d.Hm, d.Wm = (8, 16) if stride == 1 else (4, 8)
            d.in_stride, d.out_scale, d.cin, d.cout, d.groups = stride, 1, cin, cout, 1
            pad = dil * (k - 1) // 2
            taps = taps or [(ky * dil - pad, kx * dil - pad) for ky in range(k) for kx in range(k)]
            d.ntaps = len(taps)
            for t, (dy, dx) in enumerate(taps):
                d.tap_dy[0][t], d.tap_dx[0][t] = dy, dx
            if ksteps is None:
                ksteps = 7 if cin == 4 else (5 if cin == 16 else len(taps))
            d.kernel, d.w_blob, d.bias_blob = _lib.CONV_SMALLC, blob((cout // 16) * ksteps * 64 * 8 * 2), blob(cout * 4 if bbytes is None else bbytes)
            for f, v in fields.items():
                setattr(d, f, v)
            return d

        def refused(d, what):
            n = n_ops()
            rc = lib.rtm3d_op_conv(ctx, ctypes.byref(d))
            err = lib.rtm3d_last_error()
            assert rc != 0 and what in err, (what, err)
            assert n_ops() == n, 'a refused descriptor recorded an op'

        def accepted(d, name):
            n = n_ops()
            assert lib.rtm3d_op_conv(ctx, ctypes.byref(d)) == 0, lib.rtm3d_last_error()
            got = ctypes.c_char_p()
            _lib.check(lib.rtm3d_op_info(ctx, n, None, None, ctypes.byref(got)))
            assert got.value == name and n_ops() == n + 1, got.value

        x4, x4p3, x8 = tensor(8, 16, 4, 4), tensor(8, 16, 4, 3), tensor(8, 16, 8, 4)
        x16, x32, x20, x64 = tensor(8, 16, 16, 2), tensor(8, 16, 32, 2), tensor(8, 16, 20, 2), tensor(8, 16, 64, 2)
        y16, y64, y16h, y32h, y64h, y36h = (tensor(8, 16, 16, 1), tensor(8, 16, 64, 1), tensor(4, 8, 16, 1), tensor(4, 8, 32, 1),
                                            tensor(4, 8, 64, 1), tensor(4, 8, 36, 1))
        coff = lambda *v: (ctypes.c_int * 4)(*v)
        refused(conv(x16, y64, 16, 64), b'no kernel for cin=16 cout=64 ntaps=9')
        refused(conv(x32, y64, 32, 64, k=5), b'no kernel for cin=32 cout=64 ntaps=25')
        refused(conv(x64, y16, 8, 16), b'no kernel for cin=8')
        refused(conv(x32, y16, 16, 16, groups=2, in_coff=coff(0, 16)), b'groups=2')
        refused(conv(x16, y16, 16, 16, res_tensor=tensor(8, 16, 16, 1)), b'smallc): residual')
        refused(conv(x16, -1, 16, 16, out_nchw_f32=1, out_H=8, out_W=16), b'NCHW output')
        refused(conv(x16, y16, 16, 16, ksteps=4), b'weight blob size')
        refused(conv(x16, y16h, 16, 16, stride=2, ksteps=6), b'weight blob size')        # the row packing on a stride-2 launch
        refused(conv(x32, y64, 32, 64, k=1, ksteps=2), b'weight blob size')
        refused(conv(x16, y16, 16, 16, bbytes=32 * 4), b'bias blob size')
        refused(conv(x4p3, y16, 4, 16, k=7), b'border of 4')                              # (every tap inside: the eighth pixel is not)
        tdc = ((ctypes.c_int * _lib.MAX_TAPS) * _lib.MAX_GROUPS)()
        tdc[0][3] = 8
        refused(conv(x32, y16, 16, 16, tap_dc=tdc), b'per-tap channel offsets')
        # operand alignment
        refused(conv(x8, y16, 4, 16, k=7), b'cin=4 reads a 4-channel')
        refused(conv(x20, y16, 16, 16), b'16-byte operand loads')
        refused(conv(x16, y36h, 16, 32, stride=2), b'16-byte stores')
        # tap geometry: the vertical walk takes the dense row-major grid only; cin = 4 needs adjacent kx
        refused(conv(x16, y16, 16, 16, dil=2, ksteps=6), b'tap geometry')
        t3 = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
        refused(conv(x16, y16, 16, 16, ksteps=6, taps=t3[3:6] + t3[:3] + t3[6:]), b'tap geometry')
        refused(conv(x16, y16, 16, 16, ksteps=6, taps=[(dx, dy) for dy, dx in t3]), b'tap geometry')
        t7 = [(ky - 3, kx - 3) for ky in range(7) for kx in range(7)]
        refused(conv(x4, y16, 4, 16, k=7, taps=t7[7:14] + t7[:7] + t7[14:]), b'tap geometry')
        refused(conv(x4, y16, 4, 16, k=7, taps=[(dy, -dx) for dy, dx in t7]), b'tap geometry')
        refused(conv(x4, y64h, 4, 64, k=7, stride=2, taps=[(dy, -dx) for dy, dx in t7]), b'tap geometry')
        refused(conv(x4, y64h, 4, 64, k=7, stride=2, taps=[(dx, dy) for dy, dx in t7]), b'tap geometry')
        refused(conv(x4, y16, 4, 16, k=7, taps=[(dy, dx + 1) for dy, dx in t7]), b'right of tap')
        # what the instances do take
        accepted(conv(x16, y16, 16, 16, ksteps=6), b'conv_smallc_regmfma')
        accepted(conv(x16, y16, 16, 16, dil=2), b'conv_smallc_regmfma')                  # 5-step packing: per-tile kernel, any taps
        accepted(conv(x16, y32h, 16, 32, stride=2, taps=t3[::-1]), b'conv_smallc_regmfma')
        accepted(conv(x4, y16, 4, 16, k=7), b'stem7x7_regmfma')
        accepted(conv(x4, y64h, 4, 64, k=7, stride=2, taps=t7[7:14] + t7[:7] + t7[14:]), b'stem7x7_regmfma')   # rows in any order off the walk
    finally:
        lib.rtm3d_ctx_destroy(ctx)
