"""GPU (-m gpu): the tail of the forward path - the spatial-softmax fusion (pool_softmax.hip: reduce, combine, apply<1/2/3>) with
its own reduce pass and with the partials a halo-route producer writes from its epilogue (conv_mfma256_halo.hip, 4-tap and 9-tap),
the logit convs (conv_headout.hip, 8- and 16-row tiles), the k x k max-pool, and the peak-patch gather and mask of the sparse
heads (sparse_heads.hip) - over every regime their launch code can choose, one op per plan through the C ABI.

Every case first asserts its op names and its regime (tests/tail_regimes.py), then the numbers with every output poisoned and read
back raw: NaN in every slice the op must write, SENTINEL in every other channel, a zero border; afterwards everything outside the
written slice is bit-identical and every written value is finite.  The fp32 logit buffers have SENTINEL guard words on both sides.
CASES is importable without a GPU: tests/test_tail_regimes.py checks it against the mirror and the product plans' regimes.

References and tolerances
- max-pool, gather, mask: bit-equal to a NumPy restatement.  The k x k max-pool is "max over the window of the ZERO-padded
  input" (the tensor's border), which one case with negative input pins.
- logit convs: (a) exact-integer cases (inputs in -2..2, weights in -1..1, integer biases: every partial sum is an integer below
  2^24) are bit-equal to the float64 reference; (b) random cases obey |got - ref| <= (K + 1) * 2^-24 * (|x| conv |w| + |b|),
  K = 2304, per element.
- softmax fusion: float64 reference on the fp16 operands, rounded once to fp16.  The same formula in plain fp32 PyTorch, on
  the inputs of the own-reduce cases of this file, is up to 1.58 fp16 ulp of the result away from the float64 reference
  (measured on the host: 0.001 ulp where the result is of the size of its terms, 0.13 - 1.58 in the cases with a few results
  of 1e-5 that are the difference of z_in and a softmax term of order 1; each GPU case prints its own figure as well).  With
  M_FP32 = 1.6 the kernel gets TOL_ULP = 2 * M_FP32 + 1 = 4.2 ulp against the rounded reference.  The bound of
  test_gpu_kernels.py::test_softmax_fuse_with_peaked_inputs (rtol 3e-3, atol 3e-3 x max|ref|) is asserted as well, so this is
  nowhere looser.  z_in is kept at least 0.25 away from zero, which keeps such differences rare.  On the MI355X the kernels are
  1 ulp off at most in 17 of the 20 case runs and 2 - 4 ulp where the fp32 formula itself is 0.4 - 3.4 ulp off.

No case is left out of the GPU run."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import plan as plan_mod, _lib                                          # noqa: E402
from tests import conv256_tiles as ct                                                  # noqa: E402
from tests import tail_regimes as tr                                                   # noqa: E402
from tests.conv_harness import SENTINEL, _hip_memcpy, every_pair_order, f16, raw_read, raw_write   # noqa: E402
from tests.test_gpu_fused import _Ctx, _refusals, conv_f64, dev64                      # noqa: E402

CUS = 256
M_FP32 = 1.6
TOL_ULP = 2 * M_FP32 + 1
GUARD = 4096                    # SENTINEL words on both sides of every fp32 logit buffer
K_HEAD = 2304                   # products per logit: 9 taps x 256 channels
D2D = 3                         # hipMemcpyKind


def setup_module():
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, 'the mirror assumes %d CUs' % CUS


# ---------------------------------------------------------------------------------------------------------------- case specs
def sm(B, H, W, n_u, u_pads=(0, 1, 0), zi_pad=0, zo_pad=6, producer=None, wide_in=False, replay=False, expect=None):
    """A fusion of n_u operands on an H x W map.  producer: None (the operands are inputs: the reduce pass runs), 'deconv' (each
    operand is the output of a 4-tap transposed conv of an H/2 x W/2 map) or 'conv3x3' (of a 9-tap conv): the producers' epilogues
    write the partials, and a SECOND fusion of the same operands in the same plan takes the stand-alone reduce pass.  wide_in:
    the last producer reads the upper half of a 512-channel tensor.  replay: a second forward on new producer inputs."""
    return dict(kind='softmax_fuse', B=B, H=H, W=W, n_u=n_u, u_pads=tuple(u_pads[:n_u]), zi_pad=zi_pad, zo_pad=zo_pad, producer=producer,
                wide_in=wide_in, replay=replay, expect=expect or {})


def ho(B, H, W, couts, in_P=1, exact=True, expect=None):
    return dict(kind='headout', B=B, H=H, W=W, nheads=len(couts), couts=tuple(couts), in_P=in_P, exact=exact, expect=expect or {})


def mp(B, H, W, C, k, stride, pad, in_lo=0, in_hi=0, o_lo=0, o_hi=0, in_P=1, o_P=0, negative=False, expect=None):
    """A k x k max-pool of an H x W input map."""
    return dict(kind='maxpool', B=B, H=H, W=W, C=C, k=k, stride=stride, pad=pad, in_lo=in_lo, in_hi=in_hi, o_lo=o_lo, o_hi=o_hi,
                in_P=in_P, o_P=o_P, negative=negative, expect=expect or {})


def pool_out_hw(sp):
    return (sp['H'] + 2 * sp['pad'] - sp['k']) // sp['stride'] + 1, (sp['W'] + 2 * sp['pad'] - sp['k']) // sp['stride'] + 1


def producer_domain(sp):
    """(groups, Hm, Wm, ntaps) of a fusion case's producers."""
    if sp['producer'] == 'deconv':
        return 4, sp['H'] // 2, sp['W'] // 2, 4
    return 1, sp['H'], sp['W'], 9


def partial_chunks(sp):
    if not sp.get('producer'):
        return 0
    g, Hm, Wm, _ = producer_domain(sp)
    return tr.stat_chunks(g, Hm, Wm)


def producer_tiles(sp):
    g, Hm, Wm, _ = producer_domain(sp)
    return ct.tiles('halo', sp['B'] * Hm * Wm, 256, groups=g, cin=256, cus=CUS)


def mirror(sp, second=False):
    """The mirror's view of a case; second: the stand-alone fusion behind a producer case."""
    k = sp['kind']
    if k == 'softmax_fuse':
        return tr.softmax_fuse(sp['B'], sp['H'], sp['W'], sp['n_u'], CUS, 0 if second else partial_chunks(sp))
    if k == 'headout':
        return tr.headout(sp['B'], sp['H'], sp['W'], sp['nheads'], CUS, sp['in_P'])
    Ho, Wo = pool_out_hw(sp)
    return tr.maxpool(sp['B'], Ho, Wo, sp['C'])


def regimes(sp):
    """The regime keys a case runs (tests/tail_regimes.py: regime_key), as the coverage guard compares them with the plans'."""
    k = sp['kind']
    if k == 'softmax_fuse':
        keys = [tr.regime_key(k, B=sp['B'], H=sp['H'], W=sp['W'], n_u=sp['n_u'], partial_chunks=partial_chunks(sp))]
        if sp['producer']:
            keys.append(tr.regime_key(k, B=sp['B'], H=sp['H'], W=sp['W'], n_u=sp['n_u']))
            keys.append(tr.regime_key('stat_producer', ntaps=producer_domain(sp)[3], one_list=producer_tiles(sp)['one_list']))
        return keys
    if k == 'headout':
        return [tr.regime_key(k, B=sp['B'], H=sp['H'], W=sp['W'], nheads=sp['nheads'], couts=sp['couts'], in_P=sp['in_P'])]
    Ho, Wo = pool_out_hw(sp)
    return [tr.regime_key(k, k=sp['k'], stride=sp['stride'], pad=sp['pad'], B=sp['B'], Ho=Ho, Wo=Wo, C=sp['C'])]


def check_regime(sp):
    r = mirror(sp)
    for key, want in sp['expect'].items():
        if key == 'one_list':
            assert producer_tiles(sp)['one_list'] == want, (key, producer_tiles(sp))
        elif key == 'grid_mod8':
            assert r['grid'][0] % 8 == want, (key, r)
        else:
            assert r[key] == want, (key, r[key], want, r)
    return r


CASES = {
    # ---- softmax fusion with its own reduce pass: n_u 1 / 2 / 3, chunks < 16 / == 16 / > 16, xsplit 1 / 2 / 4 / 8, short and
    # empty last segments, W < 32, W % 8 != 0, rows_per_chunk 2 with an odd H, different borders of every operand
    'sm_nu1_w20': sm(2, 12, 20, 1, u_pads=(1,), expect=dict(small=True, chunks=12, parts_busy=12, xsplit=1, seg_w=24, last_seg_w=20,
                                                            reduce_tail=True, apply_tail=True)),
    'sm_nu2_h16_w72': sm(1, 16, 72, 2, u_pads=(0, 2), zi_pad=1, zo_pad=2,
                         expect=dict(chunks=16, parts_busy=16, xsplit=2, seg_w=40, seg_widths=[40, 32], apply_tail=True)),
    'sm_nu3_h17_w130': sm(1, 17, 130, 3, u_pads=(1, 0, 6), zi_pad=6, zo_pad=0,
                          expect=dict(chunks=17, xsplit=4, seg_w=40, seg_widths=[40, 40, 40, 10], reduce_tail=True)),
    'sm_nu1_xsplit8_empty_segment': sm(1, 9, 258, 1, u_pads=(0,), expect=dict(chunks=9, xsplit=8, seg_w=40, last_seg_w=0,
                                                                              seg_widths=[40] * 6 + [18, 0])),
    'sm_nu3_rows2_odd_h': sm(52, 19, 40, 3, expect=dict(small=False, rows_per_chunk=2, chunks=10, last_chunk_rows=1, xsplit=1,
                                                        reduce_grid=(10, 52, 3))),
    'sm_nu2_rows2_w36': sm(128, 8, 36, 2, u_pads=(1, 0), expect=dict(small=False, rows_per_chunk=2, chunks=4, xsplit=1, seg_w=40,
                                                                     last_seg_w=36, reduce_tail=True)),
    'sm_product_416_b1': sm(1, 104, 320, 3, u_pads=(0, 0, 0), expect=dict(small=True, chunks=104, xsplit=8, seg_w=40,
                                                                          reduce_grid=(104, 1, 3), apply_grid=(832, 1, 1))),
    'sm_product_384_b1': sm(1, 96, 320, 3, u_pads=(0, 0, 0), expect=dict(small=True, chunks=96, xsplit=8, seg_w=40, apply_tail=True)),
    'sm_product_416_b2': sm(2, 104, 320, 3, u_pads=(0, 0, 0), expect=dict(small=True, chunks=104, xsplit=4, seg_w=80)),
    'sm_product_416_rows2': sm(31, 34, 256, 3, u_pads=(0, 0, 0), expect=dict(small=False, rows_per_chunk=2, chunks=17, xsplit=4,
                                                                             seg_w=64, last_seg_w=64)),
    # ---- partials from the producers' epilogues: n_u 1 / 2 / 3, 4-tap and 9-tap, one list and per-XCD lists (several rounds),
    # B > 1, fewer than / exactly / more than 16 runs per image
    'smp_deconv_nu1_8runs': sm(1, 16, 64, 1, u_pads=(0,), producer='deconv', replay=True,
                               expect=dict(reduce_runs=False, combine_chunks=8, parts_busy=8, one_list=True)),
    'smp_conv9_nu2_16runs': sm(2, 16, 128, 2, u_pads=(0, 1), zi_pad=1, zo_pad=6, producer='conv3x3', replay=True,
                               expect=dict(reduce_runs=False, combine_chunks=16, xsplit=4, seg_w=32, one_list=True)),
    'smp_conv9_nu3_18runs': sm(1, 24, 96, 3, producer='conv3x3', expect=dict(combine_chunks=18, parts_busy=16, one_list=True)),
    'smp_conv9_nu1_rounds': sm(33, 16, 128, 1, u_pads=(0,), producer='conv3x3', expect=dict(combine_chunks=16, one_list=False)),
    'smp_deconv_nu3_rounds': sm(17, 16, 256, 3, u_pads=(0, 0, 0), producer='deconv', wide_in=True, replay=True,
                                expect=dict(reduce_runs=False, combine_chunks=32, xsplit=4, seg_w=64, one_list=False)),
    'smp_product_384_b2': sm(2, 96, 320, 3, u_pads=(0, 0, 0), producer='deconv', wide_in=True,
                             expect=dict(reduce_runs=False, combine_chunks=240, xsplit=4, seg_w=80, one_list=True)),
    # ---- logit convs, exact integers: nheads 1..4, cout 1 and 16 on every head position, grids of every residue mod 8, ragged
    # last tile rows / columns, both sides of the 8-row / 16-row switch, halo rows past the border, a border of 2 and 6
    'ho_1tile_cout1': ho(1, 8, 32, (1,), expect=dict(tile_rows=8, grid=(1, 1), grid_mod8=1)),
    'ho_h13_nheads2': ho(1, 13, 32, (16, 1), expect=dict(tile_rows=8, grid=(2, 2), last_rows=5, halo_rows_past=3, grid_mod8=2)),
    'ho_w20_nheads3': ho(3, 8, 20, (1, 16, 1), in_P=2, expect=dict(tile_rows=8, grid=(3, 3), last_cols=20, halo_cols_past=11, grid_mod8=3)),
    'ho_11x37_nheads4': ho(1, 11, 37, (16, 1, 16, 1), expect=dict(tile_rows=8, grid=(4, 4), last_rows=3, last_cols=5, grid_mod8=4)),
    'ho_b5_nheads4_cout1': ho(5, 8, 32, (1, 16, 1, 16), in_P=6, expect=dict(tile_rows=8, grid=(5, 4), grid_mod8=5)),
    'ho_b3_16x32': ho(3, 16, 32, (3, 16, 2, 2), expect=dict(tile_rows=8, grid=(6, 4), grid_mod8=6)),
    'ho_b7_5x31': ho(7, 5, 31, (16, 16), expect=dict(tile_rows=8, grid=(7, 2), last_rows=5, last_cols=31, grid_mod8=7)),
    'ho_b2_16x64_nheads1': ho(2, 16, 64, (3,), expect=dict(tile_rows=8, grid=(8, 1), grid_mod8=0)),
    'ho_switch_below': ho(85, 33, 5, (3, 16, 2, 2), expect=dict(switch_count=1020, tile_rows=8, tiles_y=5, grid=(425, 4), last_rows=1)),
    'ho_switch_at': ho(64, 17, 33, (3, 16, 2, 2), expect=dict(switch_count=1024, tile_rows=16, tiles_y=2, tiles_x=2, grid=(256, 4),
                                                            last_rows=1, last_cols=1, halo_rows_past=15, halo_cols_past=31)),
    'ho_rows16_nheads2': ho(129, 17, 40, (1, 16), in_P=2, expect=dict(switch_count=1032, tile_rows=16, grid=(516, 2), grid_mod8=4,
                                                                      halo_rows_past=14)),
    'ho_rows16_nheads3': ho(58, 40, 40, (16, 1, 16), expect=dict(switch_count=1044, tile_rows=16, tiles_y=3, grid=(348, 3), last_rows=8,
                                                                 grid_mod8=4)),
    'ho_rows16_full_nheads4': ho(32, 32, 128, (3, 16, 2, 2), expect=dict(switch_count=1024, tile_rows=16, grid=(256, 4), last_rows=16,
                                                                         last_cols=32)),
    'ho_rows16_ragged_nheads4': ho(11, 104, 128, (3, 16, 2, 2), expect=dict(tile_rows=16, tiles_y=7, last_rows=8, grid=(308, 4),
                                                                            halo_rows_past=8)),
    'ho_rows16_full_nheads1': ho(128, 32, 128, (3,), expect=dict(switch_count=1024, tile_rows=16, grid=(1024, 1), last_rows=16)),
    'ho_rows16_ragged_nheads1': ho(43, 104, 128, (3,), expect=dict(switch_count=1204, tile_rows=16, tiles_y=7, last_rows=8, grid=(1204, 1))),
    'ho_product_b1': ho(1, 96, 320, (3, 16, 2, 2), expect=dict(switch_count=240, tile_rows=8, grid=(120, 4))),
    # ---- logit convs, random data against the derivable bound
    'ho_random_8rows': ho(2, 11, 37, (3, 16, 2, 2), exact=False, expect=dict(tile_rows=8, grid=(8, 4))),
    'ho_random_16rows': ho(44, 27, 70, (3, 16, 2, 2), exact=False, expect=dict(tile_rows=16, grid=(264, 4), last_rows=11, last_cols=6)),
    'ho_random_nheads1': ho(2, 24, 64, (3,), exact=False, in_P=2, expect=dict(tile_rows=8, grid=(12, 1))),
    # ---- k x k max-pool: both window forms, channel slices on both sides, idle lanes in the last block, negative input
    'mp_2x2_product': mp(2, 48, 160, 128, 2, 2, 0, in_lo=256, o_lo=512, o_hi=512, o_P=1, expect=dict(threads=61440, idle=0)),
    'mp_2x2_idle': mp(1, 10, 14, 8, 2, 2, 0, in_lo=8, in_hi=8, o_lo=8, o_hi=8, expect=dict(threads=35, idle=221)),
    'mp_3x3_product': mp(1, 32, 64, 64, 3, 2, 1, o_P=1, expect=dict(threads=4096, idle=0)),
    'mp_3x3_idle_slices': mp(3, 14, 22, 64, 3, 2, 1, in_lo=16, in_hi=8, o_lo=8, o_hi=16, in_P=2, expect=dict(threads=1848, idle=200)),
    'mp_3x3_negative': mp(2, 16, 24, 64, 3, 2, 1, in_lo=16, negative=True, expect=dict(threads=1536, idle=0)),
    'mp_2x2_negative': mp(2, 6, 10, 16, 2, 2, 0, negative=True, in_P=0, expect=dict(threads=60, idle=196)),
}


# ---------------------------------------------------------------------------------------------------------------- units of a plan
def image(B, H, W, C, P, inner, border=0.0):
    img = np.full((B, H + 2 * P, W + 2 * P, C), border, np.float16)
    img[:, P:P + H, P:P + W] = inner
    return img


def normal(rng, shape):
    return rng.standard_normal(shape, dtype=np.float32)


class Unit(object):
    """One case's ops in a plan.  inputs: [(Slice, image)]; checked: [(Slice, H, W, pad, base image, written channel ranges)]."""

    def __init__(self, P, sp, rng):
        self.sp, self.inputs, self.checked, self.names = sp, [], [], []
        self.build(P, rng)

    def out_tensor(self, P, H, W, C, pad, ranges):
        s = P.tensor(H, W, C, pad)
        self.checked.append((s, H, W, pad, image(self.sp['B'], H, W, C, pad, SENTINEL), ranges))
        return s

    def poisoned(self):
        for s, H, W, pad, base, ranges in self.checked:
            img = base.copy()
            for lo, hi in ranges:
                img[:, pad:pad + H, pad:pad + W, lo:hi] = np.nan
            yield s, img

    def verify(self, raws):
        """Everything outside the written slices bit-identical (the zero border included), every written value finite."""
        inner = {}
        for (s, H, W, pad, base, ranges), got in zip(self.checked, raws):
            written = np.zeros(got.shape, bool)
            for lo, hi in ranges:
                written[:, pad:pad + H, pad:pad + W, lo:hi] = True
            bad = (got.view(np.uint16) != base.view(np.uint16)) & ~written
            assert not bad.any(), '%s: %d values outside the written slice changed (first at %s)' % (
                self.sp['kind'], int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert np.isfinite(got[written]).all(), '%s: %d written values never stored (NaN poison)' % (
                self.sp['kind'], int((~np.isfinite(got[written])).sum()))
            inner[id(s)] = got[:, pad:pad + H, pad:pad + W]
        return inner


def softmax_f64(z, us, dtype=torch.float64):
    out = z.to(dtype).clone()
    for u in us:
        u = u.to(dtype)
        e = (u - u.amax(dim=(1, 2), keepdim=True)).exp()
        out += u * (e / e.sum(dim=(1, 2), keepdim=True))
    return out


def ulp16(a):
    return np.spacing(np.abs(a.astype(np.float16))).astype(np.float64)


def softmax_close(got, z, us, what):
    """got: fp16 (B, H, W, 256); z, us: the fp16 operands.  TOL_ULP fp16 ulp around the once-rounded float64 reference."""
    zt, ut = dev64(z), [dev64(u) for u in us]
    ref = softmax_f64(zt, ut)
    ref16 = ref.cpu().numpy().astype(np.float16)
    m32 = float(((softmax_f64(zt, ut, torch.float32).double() - ref).abs().cpu().numpy() / ulp16(ref16)).max())
    err = np.abs(got.astype(np.float64) - ref16.astype(np.float64)) / ulp16(ref16)
    print('%s: kernel %.3f fp16 ulp from the rounded float64 reference (bound %.2f); the fp32 formula %.4f ulp from the unrounded one'
          % (what, float(err.max()), TOL_ULP, m32))
    assert err.max() <= TOL_ULP, '%s: %.3f ulp at %s' % (what, float(err.max()), np.unravel_index(err.argmax(), err.shape))
    r32 = ref16.astype(np.float32)
    np.testing.assert_allclose(got.astype(np.float32), r32, rtol=3e-3, atol=3e-3 * float(np.abs(r32).max()), err_msg=what)
    return ref16


def fusion_operands(rng, B, H, W, n_u, seg_w):
    """z_in (|z| >= 0.25) and n_u operands of scale 1 / 3 / 6 with a +9 peak per channel; channel 0 of the first is constant over
    the map (weights exactly 1 / HW), channel 1 has its maximum in the last pixel of the last row, channel 2 in the last pixel
    of the first column segment, channel 3 in the last column of a middle row."""
    z = normal(rng, (B, H, W, 256))
    z = f16(np.sign(z) * (0.25 + np.abs(z)))
    us = []
    for i in range(n_u):
        u = normal(rng, (B, H, W, 256)) * (1.0, 3.0, 6.0)[i]
        u[:, 3 % H, 4 % W, :] += 9.0
        if i == 0:
            u[..., 0] = 0.5
            for c, (y, x) in ((1, (H - 1, W - 1)), (2, (0, min(seg_w, W) - 1)), (3, (H // 2, W - 1))):
                u[:, 3 % H, 4 % W, c] -= 9.0
                u[:, y, x, c] = 40.0
        us.append(f16(u))
    return z, us


class Fusion(Unit):
    def build(self, P, rng):
        sp = self.sp
        B, H, W, n = sp['B'], sp['H'], sp['W'], sp['n_u']
        r = mirror(sp)
        self.z_img, u_imgs = fusion_operands(rng, B, H, W, 0 if sp['producer'] else n, r['seg_w'])
        # borders that are not the fusion's to read hold SENTINEL: a row or column offset that is off by the border shows
        self.z0 = P.tensor(H, W, 256, sp['zi_pad'])
        self.inputs.append((self.z0, image(B, H, W, 256, sp['zi_pad'], self.z_img, SENTINEL)))
        self.us, self.xs, self.ws = [], [], []
        for i, pad in enumerate(sp['u_pads']):
            if not sp['producer']:
                u = P.tensor(H, W, 256, pad)
                self.inputs.append((u, image(B, H, W, 256, pad, u_imgs[i], SENTINEL)))
            else:
                u = self.out_tensor(P, H, W, 256, pad, [(0, 256)])
                dec = sp['producer'] == 'deconv'
                hi, wi = (H // 2, W // 2) if dec else (H, W)
                wide = sp['wide_in'] and i == n - 1
                xt = P.tensor(hi, wi, 512 if wide else 256, 1)
                xs = P.sub(xt, 256, 256) if wide else xt
                sc = (1.0, 2.5, 6.0)[i]
                if dec:
                    w = (normal(rng, (256, 256, 4, 4)) * (sc / 32)).astype(np.float32)
                    P.deconv(xs, u, w, name='up%d' % len(P.ops))
                    self.names.append('deconv4x4_phase_mfma256_halo')
                else:
                    w = (normal(rng, (256, 256, 3, 3)) * (sc / 48)).astype(np.float32)
                    P.conv(xs, u, w, (normal(rng, (256,)) * 0.3).astype(np.float32), name='c%d' % len(P.ops))
                    self.names.append('conv3x3_mfma256_halo')
                P.ops[-1]['variant'] = _lib.CONV_MFMA256
                self.xs.append((xt, hi, wi, 512 if wide else 256))
            self.us.append(u)
        self.new_inputs(rng)
        self.z = self.out_tensor(P, H, W, 256, sp['zo_pad'], [(0, 256)])
        self.fuse_ops = [len(P.ops)]
        P.softmax_fuse(self.z0, self.z, self.us, name='fuse%d' % len(P.ops))
        self.names.append('softmax_fuse')
        self.z2 = None
        if sp['producer']:
            # the same operands through the stand-alone reduce pass: the first fusion consumed the producers' partial buffer
            self.z2 = self.out_tensor(P, H, W, 256, 6 - sp['zo_pad'], [(0, 256)])
            self.fuse_ops.append(len(P.ops))
            P.softmax_fuse(self.z0, self.z2, self.us, name='fuse%d' % len(P.ops))
            self.names.append('softmax_fuse')

    def new_inputs(self, rng):
        """(New) inputs of the producers."""
        self.x_inputs = [(xt, image(self.sp['B'], hi, wi, C, 1, f16(normal(rng, (self.sp['B'], hi, wi, C))))) for xt, hi, wi, C in self.xs]

    def check(self, inner, what):
        sp = self.sp
        if sp['producer']:
            us = [inner[id(u)] for u in self.us]                    # the fp16 maps the producers stored ARE the operands
        else:
            us = [img[:, p:p + sp['H'], p:p + sp['W']] for (_, img), p in zip(self.inputs[1:], sp['u_pads'])]
        got = inner[id(self.z)]
        ref16 = softmax_close(got, self.z_img, us, what + ' z')
        if self.z2 is not None:
            got2 = inner[id(self.z2)]
            softmax_close(got2, self.z_img, us, what + ' z (stand-alone reduce pass)')
            d = np.abs(got.astype(np.float64) - got2.astype(np.float64)) / ulp16(ref16)
            assert d.max() <= TOL_ULP, '%s: epilogue partials and reduce pass differ by %.2f ulp' % (what, float(d.max()))
        return got


class HeadOut(Unit):
    def build(self, P, rng):
        sp = self.sp
        B, H, W, n, pad = sp['B'], sp['H'], sp['W'], sp['nheads'], sp['in_P']
        self.ht = P.tensor(H, W, 256 * n, pad)
        if sp['exact']:
            x = rng.integers(-2, 3, (B, H, W, 256 * n)).astype(np.float16)
            self.ws = [rng.integers(-1, 2, (c, 256, 3, 3)).astype(np.float32) for c in sp['couts']]
            self.bs = [rng.integers(-8, 9, c).astype(np.float32) for c in sp['couts']]
        else:
            x = f16(normal(rng, (B, H, W, 256 * n)))
            self.ws = [f16(normal(rng, (c, 256, 3, 3)) / 48).astype(np.float32) for c in sp['couts']]
            self.bs = [normal(rng, (c,)) for c in sp['couts']]
        self.x = x
        img = image(B, H, W, 256 * n, pad, x, SENTINEL)
        img[:, pad - 1:pad + H + 1, pad - 1:pad + W + 1][:, [0, -1]] = 0       # the ring the 3x3 window reads is zero padding;
        img[:, pad - 1:pad + H + 1, pad - 1:pad + W + 1][:, :, [0, -1]] = 0    # wider borders hold SENTINEL: never multiplied
        self.inputs.append((self.ht, img))
        P.headout(self.ht, self.ws, self.bs, name='heads.out%d' % len(P.ops))
        self.names.append('conv3x3_headout_halo')

    def buffers(self):
        """One guarded fp32 buffer per output slot: NaN where head i writes B x cout x H x W logits, SENTINEL around."""
        sp, bufs = self.sp, []
        for i in range(4):
            n = sp['B'] * sp['couts'][i] * sp['H'] * sp['W'] if i < sp['nheads'] else 0
            b = torch.full((n + 2 * GUARD,), float(SENTINEL), device='cuda')
            b[GUARD:GUARD + n] = float('nan')
            bufs.append(b)
        return bufs

    def check_buffers(self, bufs, what):
        sp = self.sp
        B, H, W = sp['B'], sp['H'], sp['W']
        outs = []
        for i, b in enumerate(bufs):
            n = b.numel() - 2 * GUARD
            g = torch.cat([b[:GUARD], b[GUARD + n:]])
            assert bool((g == float(SENTINEL)).all()), '%s: head %d wrote outside its %d logits' % (what, i, n)
            if i >= sp['nheads']:
                continue
            got = b[GUARD:GUARD + n].view(B, sp['couts'][i], H, W)
            assert bool(torch.isfinite(got).all()), '%s: head %d left %d logits unwritten' % (what, i, int((~torch.isfinite(got)).sum()))
            x = dev64(self.x[..., i * 256:(i + 1) * 256])
            w, bias = dev64(self.ws[i]), dev64(self.bs[i])
            ref = conv_f64(x, w, bias).permute(0, 3, 1, 2)
            if sp['exact']:
                assert bool((got.double() == ref).all()), '%s: head %d: %d logits differ from the exact integer result (first at %s)' % (
                    what, i, int((got.double() != ref).sum()), (got.double() != ref).nonzero()[0].tolist())
            else:
                bound = (K_HEAD + 1) * 2.0 ** -24 * conv_f64(x.abs(), w.abs(), bias.abs()).permute(0, 3, 1, 2)
                err = (got.double() - ref).abs()
                print('%s: head %d: largest error / bound = %.3f' % (what, i, float((err / bound).max())))
                assert bool((err <= bound).all()), '%s: head %d: error %.3g over the bound %.3g' % (
                    what, i, float(err.max()), float(bound.flatten()[err.argmax()]))
            outs.append(got.cpu().numpy())
        return outs


class MaxPool(Unit):
    def build(self, P, rng):
        sp = self.sp
        B, H, W, C, pad = sp['B'], sp['H'], sp['W'], sp['C'], sp['in_P']
        Ho, Wo = pool_out_hw(sp)
        it = P.tensor(H, W, sp['in_lo'] + C + sp['in_hi'], pad)
        v = normal(rng, (B, H, W, it.C))
        # (negative: every value below zero, so that a window over the border must give the border's zero)
        self.img = image(B, H, W, it.C, pad, f16(-0.5 - np.abs(v) if sp['negative'] else np.maximum(v, 0)))
        self.inputs.append((it, self.img))
        self.ot = self.out_tensor(P, Ho, Wo, sp['o_lo'] + C + sp['o_hi'], sp['o_P'], [(sp['o_lo'], sp['o_lo'] + C)])
        P.maxpool(P.sub(it, sp['in_lo'], C), P.sub(self.ot, sp['o_lo'], C), sp['k'], sp['stride'], sp['pad'], name='pool%d' % len(P.ops))
        self.names.append('maxpool')

    def check(self, inner, what):
        sp = self.sp
        Ho, Wo = pool_out_hw(sp)
        k, s, C = sp['k'], sp['stride'], sp['C']
        o = sp['in_P'] - sp['pad']
        x = self.img[..., sp['in_lo']:sp['in_lo'] + C].astype(np.float32)
        want = np.max([x[:, o + ky:o + ky + (Ho - 1) * s + 1:s, o + kx:o + kx + (Wo - 1) * s + 1:s] for ky in range(k) for kx in range(k)], axis=0)
        got = inner[id(self.ot)][..., sp['o_lo']:sp['o_lo'] + C]
        np.testing.assert_array_equal(got.astype(np.float32), want, err_msg=what + ': not the max over the window of the zero-padded input')
        if sp['negative'] and sp['pad']:
            assert (got[:, 0] == 0).all() and (got[:, :, 0] == 0).all() and (got[:, 1:, 1:] < 0).all()
        return got


KIND = {'softmax_fuse': Fusion, 'headout': HeadOut, 'maxpool': MaxPool}


# ---------------------------------------------------------------------------------------------------------------- running
def _forward(R, units, bufs):
    for u in units:
        for s, img in u.inputs + getattr(u, 'x_inputs', []):
            raw_write(R, s, img)
        for s, img in u.poisoned():
            raw_write(R, s, img)
    xin = torch.zeros(16, device='cuda')
    R.forward(torch.cuda.current_stream().cuda_stream, xin.data_ptr(), [b.data_ptr() + 4 * GUARD for b in bufs])
    torch.cuda.synchronize()
    return [u.verify([raw_read(R, c[0]) for c in u.checked]) for u in units]


def _no_logits():
    return [torch.full((2 * GUARD,), float(SENTINEL), device='cuda') for _ in range(4)]


def run_units(P, units, what, replays=0, graph=False):
    """Record P, assert the op names, run one poisoned forward and check every unit; then `replays` eager replays and (graph)
    one hipGraph replay, each re-poisoned and bit-identical to the first.  Returns each unit's result of the first forward."""
    R = plan_mod.RealizedPlan(P, 0)
    try:
        assert R.kernel_names() == [n for u in units for n in u.names], R.kernel_names()
        heads = [u for u in units if u.sp['kind'] == 'headout']

        def once():
            bufs = heads[-1].buffers() if heads else _no_logits()
            inner = _forward(R, units, bufs)
            res = []
            for u, i in zip(units, inner):
                if u.sp['kind'] == 'headout':
                    # (every head-out op of a plan writes the same four slots: the last one's logits are what is left)
                    res.append(u.check_buffers(bufs, what) if u is heads[-1] else [])
                else:
                    res.append([u.check(i, what)])
            if not heads:
                assert all(bool((b == float(SENTINEL)).all()) for b in bufs), what + ': a plan without logit convs wrote a logit buffer'
            return res
        for u in units:
            if u.sp['kind'] == 'softmax_fuse' and u.sp['producer']:
                slots = {R.lowering['stat_slots'].get(k) for k in range(len(P.ops))} - {None}
                assert slots >= set(range(u.sp['n_u'])), R.lowering['stat_slots']
        first = once()
        later = [once() for _ in range(replays)]
        if graph:
            R.set_graph(True)
            later.append(once())
            captures, _, enabled = R.graph_stats()
            assert captures == 1 and enabled, R.graph_stats()
        for res in later:
            for a, b in zip(first, res):
                for x, y in zip(a, b):
                    assert x.tobytes() == y.tobytes(), what + ': a replay differs from the first forward'
        for u in units:
            if u.sp['kind'] == 'softmax_fuse' and u.sp['replay']:
                # the partial buffer is rewritten by every forward: new producer inputs, new maps, new statistics
                u.new_inputs(np.random.default_rng(99))
                again = once()
                assert again[units.index(u)][0].tobytes() != first[units.index(u)][0].tobytes()
        return first
    finally:
        R.close()


def run_one(sp, seed, what):
    check_regime(sp)
    P = plan_mod.Plan(sp['B'], 4 * sp['H'], 4 * sp['W'])
    return run_units(P, [KIND[sp['kind']](P, sp, np.random.default_rng(seed))], what)


@pytest.mark.parametrize('name', list(CASES))
def test_tail_op_and_regime(name):
    run_one(CASES[name], seed=sum(map(ord, name)), what=name)


# ---- ops of different regimes in ONE context, every ordered pair back to back, twice and as a graph: the producers' partial
# buffer (taken by the fusion right behind them, never by a later one), the statistics and partial allocations of each fusion
CHAIN = {
    'fusion_reduce': sm(2, 12, 40, 2, u_pads=(0, 1), expect=dict(reduce_runs=True, chunks=12)),
    'fusion_partials': sm(2, 16, 64, 1, u_pads=(0,), producer='deconv', expect=dict(reduce_runs=False, combine_chunks=8)),
    'fusion_partials_9tap': sm(2, 8, 32, 2, u_pads=(1, 0), zo_pad=0, producer='conv3x3', expect=dict(reduce_runs=False, combine_chunks=2)),
    'maxpool': mp(2, 12, 20, 16, 3, 2, 1, in_lo=8, o_lo=8, expect=dict(idle=16)),
    'headout': ho(2, 11, 37, (3, 16), expect=dict(tile_rows=8)),
}


def test_tail_chain_carries_no_state():
    keys = list(CHAIN)
    order = every_pair_order(len(keys))
    assert len({(a, b) for a, b in zip(order, order[1:])}) == len(keys) * (len(keys) - 1)
    single = {k: run_one(sp, seed=i, what='single ' + k)[0] for i, (k, sp) in enumerate(CHAIN.items())}
    P = plan_mod.Plan(2, 64, 256)
    units = [KIND[CHAIN[keys[i]]['kind']](P, CHAIN[keys[i]], np.random.default_rng(i)) for i in order]
    res = run_units(P, units, 'chain', replays=1, graph=True)
    last_head = max(j for j, i in enumerate(order) if keys[i] == 'headout')
    for j, (i, got) in enumerate(zip(order, res)):
        if keys[i] == 'headout' and j != last_head:
            continue
        assert len(got) == len(single[keys[i]])
        for a, b in zip(got, single[keys[i]]):
            assert a.tobytes() == b.tobytes(), 'chain position %d (%s) differs from the op run alone' % (j, keys[i])


# ---------------------------------------------------------------------------------------------------------------- peak patches
def _gather(z_img, zP, n, peaks, topk, slots=None, yx_bytes=None, S=tr.PATCH):
    """rtm3d_gather_peak_patches on a padded z image (B, H + 2 zP, W + 2 zP, 256): (rc, patches, yx)."""
    lib = _lib.load()
    B, Hp, Wp, C = z_img.shape
    z = torch.from_numpy(z_img.view(np.int16)).cuda()
    nslots = B * topk if slots is None else slots
    patch = torch.from_numpy(np.full((max(nslots, 1), S, S, 256), SENTINEL, np.float16).view(np.int16)).cuda()
    yx = torch.full((B * topk, 2), 77, dtype=torch.int32, device='cuda')
    nd, xy = torch.tensor(n, dtype=torch.int32, device='cuda'), torch.tensor(peaks, dtype=torch.float32, device='cuda')
    rc = lib.rtm3d_gather_peak_patches(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.c_void_p(z.data_ptr()), Hp - 2 * zP,
                                       Wp - 2 * zP, C, zP, B, topk, ctypes.c_void_p(nd.data_ptr()), ctypes.c_void_p(xy.data_ptr()),
                                       ctypes.c_void_p(patch.data_ptr()), ctypes.c_void_p(yx.data_ptr()), nslots, S,
                                       yx.numel() * 4 if yx_bytes is None else yx_bytes)
    torch.cuda.synchronize()
    return rc, patch.cpu().numpy().view(np.float16), yx.cpu().numpy()


def edge_peaks(H, W):
    """(y, x): the four corners, a peak on each edge, at distance 1, 2, 7, 8 from the edges, one in the interior."""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2), (H // 2, W - 1),
            (1, 1), (2, 2), (7, 7), (8, 8), (H - 2, W - 2), (H - 3, W - 3), (H - 8, W - 8), (H - 9, W - 9), (H // 2, W // 2)]


@pytest.mark.parametrize('zP', [6, 0, 2])
def test_peak_patch_gather(zP):
    """Every pixel of every patch against patch_cell: z encodes (image, y, x, channel) in exact fp16 integers (channel 0: y + 1,
    1: x + 1, 2: image + 1, c: a mix below 2048), the border of z holds -(that) so that zeros appear only where z's padded tensor
    ends.  Empty slots keep their patch and get yx = -1."""
    B, H, W, topk = 2, 24, 40, 10
    yy, xx, bb, cc = np.meshgrid(np.arange(-zP, H + zP), np.arange(-zP, W + zP), np.arange(B), np.arange(256), indexing='ij')
    enc = np.where(cc == 0, yy + zP + 1, np.where(cc == 1, xx + zP + 1, np.where(cc == 2, bb + 1, (cc * 7 + yy * 3 + xx * 5 + bb * 11) % 2047 + 1)))
    inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    z_img = np.ascontiguousarray(np.where(inside, enc, -enc).transpose(2, 0, 1, 3)).astype(np.float16)
    assert (z_img != 0).all() and (z_img.astype(np.int64) == np.where(inside, enc, -enc).transpose(2, 0, 1, 3)).all()
    pk = edge_peaks(H, W)
    n = [10, 7]
    slots = pk[:10] + pk[10:] + [(5, 5)] * 3                      # (image 1: 7 peaks and three empty slots)
    xy = [(x + (0.25 if i % 2 else 0.0), y + (0.5 if i % 3 == 0 else 0.0)) for i, (y, x) in enumerate(slots)]
    rc, patch, yx = _gather(z_img, zP, n, xy, topk)
    assert rc == 0, _lib.load().rtm3d_last_error()
    for s, (py, px) in enumerate(slots):
        b, rank = divmod(s, topk)
        if rank >= n[b]:
            assert (yx[s] == -1).all() and (patch[s].view(np.uint16) == np.float16(SENTINEL).view(np.uint16)).all(), s
            continue
        assert tuple(yx[s]) == (py, px), (s, yx[s])
        want = np.zeros((tr.PATCH, tr.PATCH, 256), np.float16)
        for r in range(tr.PATCH):
            for c in range(tr.PATCH):
                dy, dx = tr.patch_cell(r, c)
                y, x = py + dy + zP, px + dx + zP
                if 0 <= y < H + 2 * zP and 0 <= x < W + 2 * zP:
                    want[r, c] = z_img[b, y, x]
        bad = patch[s].view(np.uint16) != want.view(np.uint16)
        assert not bad.any(), 'slot %d, peak (%d, %d): patch pixel %s is wrong' % (s, py, px, np.argwhere(bad)[0].tolist())


def test_peak_patch_mask():
    """S = 5 / origin 2 and S = 3 / origin 1 (build_peak_plan) on a SENTINEL fill: exactly the window positions outside the image
    become zero, everything else and every slot with py < 0 stays bit-identical."""
    H, W = 24, 40
    pk = edge_peaks(H, W) + [(-1, -1), (-1, 3)]
    P = plan_mod.Plan(len(pk), tr.PATCH, tr.PATCH)
    P.map_hw = (H, W)
    ts = [(P.tensor(5, 5, 512, 0), 5, 2), (P.tensor(3, 3, 512, 0), 3, 1), (P.tensor(5, 5, 8, 0), 5, 2)]
    for t, S, origin in ts:
        P.patch_mask(t, origin)
    R = plan_mod.RealizedPlan(P, 0)
    try:
        assert R.kernel_names() == ['patch_mask'] * 3
        yx = np.ascontiguousarray(pk, np.int32)
        assert R.blob_bytes(R.yx_blob) == yx.nbytes
        _hip_memcpy(R.lib, R.blob_address(R.yx_blob), yx.ctypes.data, yx.nbytes, 1)
        fill = np.float16(SENTINEL).view(np.uint16)
        for t, S, origin in ts:
            raw_write(R, t, np.full((len(pk), S, S, t.C), SENTINEL, np.float16))
        bufs = _no_logits()
        R.forward(torch.cuda.current_stream().cuda_stream, 0, [b.data_ptr() + 4 * GUARD for b in bufs])
        torch.cuda.synchronize()
        for t, S, origin in ts:
            got = raw_read(R, t).view(np.uint16)
            cleared = 0
            for s, (py, px) in enumerate(pk):
                zero = tr.mask_zeroed(py, px, S, origin, H, W)
                cleared += len(zero)
                for i in range(S):
                    for j in range(S):
                        want = 0 if (i, j) in zero else fill
                        assert (got[s, i, j] == want).all(), ('S', S, 'slot', s, 'peak', (py, px), 'position', (i, j))
            assert cleared > 0
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------- 32-bit offsets
def test_headout_offsets_stay_below_4g_elements():
    """conv_headout_kernel keeps `pix * in_C + head * 256 + ...` in 32 bits.  It cannot wrap: rtm3d_tensor_create refuses every
    tensor of 2^32 - 2 * GUARD elements or more (named: "32-bit offset range"), so the 4 x 256-channel head tensor of 133 images at
    384 x 1280 (or 123 at 416 x 1280) does not exist, and the offset of the last element of any tensor that does fits.  Pinned here:
    the refusal (nothing is created), and - on the largest head tensor at 384 x 1280 that is accepted, 132 images, 8.5 GB, every
    image different - the exact logits of the first and of the last image, whose offsets are the largest the kernel can meet."""
    c = _Ctx()
    try:
        tid = ctypes.c_int(-7)
        for B, H in ((133, 96), (123, 104)):
            assert B * (H + 2) * 322 * 1024 >= 1 << 32 > (B - 1) * (H + 2) * 322 * 1024
            assert c.lib.rtm3d_tensor_create(c.ctx, B, H, 320, 1024, 1, ctypes.byref(tid)) != 0
            err = c.lib.rtm3d_last_error()
            assert err.startswith(b'tensor_create:') and b'32-bit offset range' in err, err
            assert tid.value == -7
        assert c.lib.rtm3d_tensor_create(c.ctx, 1, 8, 32, 256, 1, ctypes.byref(tid)) == 0 and tid.value == 0   # (nothing was created)
    finally:
        c.close()
    B, H, W, couts = 132, 96, 320, (3, 16, 2, 2)
    rng = np.random.default_rng(4)
    P = plan_mod.Plan(B, 4 * H, 4 * W)
    ht = P.tensor(H, W, 1024, 1)
    ws = [rng.integers(-1, 2, (co, 256, 3, 3)).astype(np.float32) for co in couts]
    bs = [rng.integers(-8, 9, co).astype(np.float32) for co in couts]
    P.headout(ht, ws, bs)
    R = plan_mod.RealizedPlan(P, 0)
    try:
        assert tr.headout(B, H, W, 4, CUS)['tile_rows'] == 16
        base, shape, per = R.tensor_info(ht)[0], (H + 2, W + 2, 1024), (H + 2) * (W + 2) * 1024
        assert (B - 1) * per + (H + 1) * (W + 2) * 1024 > 0xF0000000          # the last image's offsets use the top of the range
        img0 = torch.zeros(shape, dtype=torch.float16, device='cuda')
        img0[1:-1, 1:-1] = torch.from_numpy(rng.integers(-2, 3, (H, W, 1024)).astype(np.float16)).cuda()
        for n in range(B):                                                      # image n: image 0 rotated by n channels
            img = torch.roll(img0, n, 2).contiguous()
            torch.cuda.synchronize()
            _hip_memcpy(R.lib, base + 2 * n * per, img.data_ptr(), 2 * per, D2D)
        bufs = [torch.full((B * co * H * W + 2 * GUARD,), float('nan'), device='cuda') for co in couts]
        R.forward(torch.cuda.current_stream().cuda_stream, 0, [b.data_ptr() + 4 * GUARD for b in bufs])
        torch.cuda.synchronize()
        for n in (0, B - 1):
            x = torch.roll(img0, n, 2)[1:-1, 1:-1].double()[None]
            for i, co in enumerate(couts):
                got = bufs[i][GUARD:GUARD + B * co * H * W].view(B, co, H, W)[n]
                ref = conv_f64(x[..., i * 256:(i + 1) * 256], dev64(ws[i]), dev64(bs[i]))[0].permute(2, 0, 1)
                assert bool((got.double() == ref).all()), 'image %d, head %d: %d logits differ' % (n, i, int((got.double() != ref).sum()))
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------- admission
def _conv_desc(c, t_in, t_out, slot, Hm=8, Wm=32, dil=1, kernel=None, out_coff=0):
    d = _lib.ConvDesc()
    d.in_tensor, d.out_tensor, d.res_tensor = t_in, t_out, -1
    d.Hm, d.Wm, d.in_stride, d.out_scale = Hm, Wm, 1, 1
    d.cin, d.cout, d.groups, d.ntaps = 256, 256, 1, 9
    d.out_coff[0] = out_coff
    for t in range(9):
        d.tap_dy[0][t], d.tap_dx[0][t] = dil * (t // 3 - 1), dil * (t % 3 - 1)
    d.w_blob, d.bias_blob = c.blob(9 * 256 * 256 * 2), c.blob(256 * 4)
    d.kernel = _lib.CONV_MFMA256 if kernel is None else kernel
    d.bn_tile = 256 if kernel is None else 64
    d.out_H, d.out_W, d.softmax_stat_slot = Hm, Wm, slot
    return d


def test_fusion_refusals_are_named_and_record_nothing():
    c = _Ctx()
    try:
        z0, z1, u0, u1 = [c.tensor(1, 8, 32, 256, p) for p in (0, 6, 0, 1)]
        u128, z128, u_w64, u_b2 = c.tensor(1, 8, 32, 128, 0), c.tensor(1, 8, 32, 128, 0), c.tensor(1, 8, 64, 256, 0), c.tensor(2, 8, 32, 256, 0)
        fuse = lambda zi, zo, n, us: c.lib.rtm3d_op_softmax_fuse(c.ctx, zi, zo, n, (ctypes.c_int * 4)(*(list(us) + [0] * (4 - len(us)))))
        _refusals(c, fuse, b'op_softmax_fuse', [z0, z1, 1, (u0,)], [
            ({2: 0}, b'bad arguments'), ({2: 4, 3: (u0, u1, u0, u1)}, b'bad arguments'), ({0: 999}, b'bad arguments'), ({1: -1}, b'bad arguments'),
            ({3: (u128,)}, b'u tensor 0 mismatch'), ({2: 2, 3: (u0, u128)}, b'u tensor 1 mismatch'), ({3: (u_w64,)}, b'u tensor 0 mismatch'),
            ({3: (u_b2,)}, b'u tensor 0 mismatch'), ({3: (999,)}, b'u tensor 0 mismatch'),
            ({0: z128}, b'z tensors must be 256-channel'), ({1: z128}, b'z tensors must be 256-channel'), ({1: u_w64}, b'z tensors must be 256-channel'),
        ])
        # producers: slot out of range, wrong kernel, not the halo route, an output that is not the whole 256-channel tensor
        x, x6, wide, o16 = c.tensor(1, 8, 32, 256, 1), c.tensor(1, 8, 32, 256, 6), c.tensor(1, 8, 32, 512, 0), c.tensor(1, 16, 64, 256, 0)
        x16 = c.tensor(1, 16, 64, 256, 1)
        conv = lambda d: c.lib.rtm3d_op_conv(c.ctx, ctypes.byref(d))
        _refusals(c, conv, b'op_conv', [_conv_desc(c, x, u0, 0)], [
            ({0: _conv_desc(c, x, u0, 3)}, b'softmax_stat_slot out of range'),
            ({0: _conv_desc(c, x, u0, 0, kernel=_lib.CONV_MFMA128)}, b'softmax_stat_slot needs kernel = 2'),
            ({0: _conv_desc(c, x6, u0, 0, dil=6)}, b'does not take the halo-tile kernel'),
            ({0: _conv_desc(c, x, wide, 0, out_coff=256)}, b'softmax partials need'),
            ({0: _conv_desc(c, x, wide, 0)}, b'softmax partials need'),
        ])
        # one producer accepted; a second of another shape is refused; a fusion of other operands is refused; the matching one is taken
        n = c.n_ops()
        assert conv(_conv_desc(c, x, u0, 0)) == 0 and c.n_ops() == n + 1 and c.last_name() == b'conv3x3_mfma256_halo', c.lib.rtm3d_last_error()
        _refusals(c, conv, b'op_conv', [None], [({0: _conv_desc(c, x16, o16, 1, Hm=16, Wm=64)}, b'producers of one fusion must have equal shapes')])
        _refusals(c, fuse, b'op_softmax_fuse', [z0, z1, 1, (u0,)], [
            ({3: (u1,)}, b'producers do not match'), ({2: 2, 3: (u0, u1)}, b'producers do not match')])
        assert fuse(z0, z1, 1, (u0,)) == 0 and c.n_ops() == n + 2 and c.last_name() == b'softmax_fuse'
        assert fuse(z0, z1, 1, (u1,)) == 0 and c.n_ops() == n + 3          # (consumed: a later fusion reduces for itself)
    finally:
        c.close()


def test_headout_pool_and_patch_refusals_are_named_and_record_nothing():
    c = _Ctx()
    try:
        h4, h1, h0pad, h3 = c.tensor(1, 8, 32, 1024, 1), c.tensor(1, 8, 32, 256, 1), c.tensor(1, 8, 32, 1024, 0), c.tensor(1, 8, 32, 768, 2)
        w = {n: c.blob(n * 9 * 8 * 64 * 8 * 2) for n in (1, 3, 4)}
        b = {n: c.blob(n * 16 * 4) for n in (1, 3, 4)}
        co = lambda *v: (ctypes.c_int * 4)(*v)
        head = lambda *a: c.lib.rtm3d_op_headout(c.ctx, *a)
        _refusals(c, head, b'op_headout', [h4, w[4], b[4], 4, co(3, 16, 2, 2)], [
            ({3: 0}, b'nheads must be in [1,4]'), ({3: 5}, b'nheads must be in [1,4]'), ({0: 999}, b'bad arguments'), ({4: None}, b'bad arguments'),
            ({4: co(3, 0, 2, 2)}, b'cout must be in [1,16]'), ({4: co(3, 16, 2, 17)}, b'cout must be in [1,16]'), ({4: co(-1, 16, 2, 2)}, b'cout must be in [1,16]'),
            ({0: h0pad}, b'border >= 1'), ({0: h1}, b'nheads x 256 channel'), ({3: 3}, b'nheads x 256 channel'),
            ({1: w[3]}, b'blob size mismatch'), ({2: b[3]}, b'blob size mismatch'), ({1: b[4]}, b'blob size mismatch'), ({1: 999}, b'blob size mismatch'),
        ])
        for args in ([h4, w[4], b[4], 4, co(1, 16, 16, 1)], [h1, w[1], b[1], 1, co(3, 0, 0, 0)], [h3, w[3], b[3], 3, co(16, 1, 16, 99)]):
            n = c.n_ops()
            assert head(*args) == 0 and c.n_ops() == n + 1 and c.last_name() == b'conv3x3_headout_halo', c.lib.rtm3d_last_error()
        # max-pool: in, in_coff, out, out_coff, channels, k, stride, pad
        pi, po, po_big, pi0 = c.tensor(1, 16, 24, 80, 1), c.tensor(1, 8, 12, 64, 0), c.tensor(1, 9, 12, 64, 0), c.tensor(1, 16, 24, 64, 0)
        pool = lambda *a: c.lib.rtm3d_op_maxpool(c.ctx, *a)
        _refusals(c, pool, b'op_maxpool', [pi, 16, po, 0, 64, 3, 2, 1], [
            ({0: 999}, b'bad tensors'), ({2: -1}, b'bad tensors'),
            ({1: 24}, b'bad channel slice'), ({1: 4}, b'bad channel slice'), ({3: 8}, b'bad channel slice'), ({3: 4}, b'bad channel slice'),
            ({4: 60}, b'bad channel slice'), ({4: 72}, b'bad channel slice'),
            ({7: 2}, b'narrower than pool padding'), ({0: pi0, 1: 0}, b'narrower than pool padding'),
            ({2: po_big}, b'window leaves the padded input'), ({5: 5}, b'window leaves the padded input'), ({6: 3}, b'window leaves the padded input'),
        ])
        n = c.n_ops()
        assert pool(pi, 16, po, 0, 64, 3, 2, 1) == 0 and pool(pi0, 0, po, 0, 64, 2, 2, 0) == 0 and c.n_ops() == n + 2 and c.last_name() == b'maxpool'
        # patch mask: tensor, yx blob, img_H, img_W, origin
        sq, rect, bordered, c4 = c.tensor(6, 5, 5, 512, 0), c.tensor(6, 5, 3, 512, 0), c.tensor(6, 5, 5, 512, 1), c.tensor(6, 5, 5, 4, 0)
        yx, yx_short = c.blob(6 * 8), c.blob(5 * 8)
        mask = lambda *a: c.lib.rtm3d_op_patch_mask(c.ctx, *a)
        _refusals(c, mask, b'op_patch_mask', [sq, yx, 96, 320, 2], [
            ({0: 999}, b'bad tensor'), ({0: rect}, b'must be square, borderless'), ({0: bordered}, b'must be square, borderless'),
            ({0: c4}, b'must be square, borderless'), ({4: 5}, b'must be square, borderless'), ({4: -1}, b'must be square, borderless'),
            ({2: 0}, b'must be square, borderless'), ({1: yx_short}, b'2 int32 per slot'), ({1: 999}, b'2 int32 per slot'),
        ])
        n = c.n_ops()
        assert mask(sq, yx, 96, 320, 2) == 0 and c.n_ops() == n + 1 and c.last_name() == b'patch_mask'
    finally:
        c.close()


def test_gather_refusals_are_named_and_write_nothing():
    B, H, W, topk = 1, 24, 40, 4
    z = np.ones((B, H, W, 256), np.float16)
    xy = [(5.0, 5.0)] * topk
    for kw, msg in ((dict(slots=topk - 1), b'cannot hold'), (dict(yx_bytes=8 * topk - 4), b'cannot hold'), (dict(S=5), b'cannot hold')):
        rc, patch, yx = _gather(z, 0, [topk], xy, topk, **kw)
        err = _lib.load().rtm3d_last_error()
        assert rc != 0 and err.startswith(b'gather_peak_patches:') and msg in err, (kw, err)
        assert (patch.view(np.uint16) == np.float16(SENTINEL).view(np.uint16)).all() and (yx == 77).all(), kw
    z128 = np.ones((B, H, W, 128), np.float16)
    rc, patch, yx = _gather(z128, 0, [topk], xy, topk)
    assert rc != 0 and b'256 channels' in _lib.load().rtm3d_last_error() and (yx == 77).all()
