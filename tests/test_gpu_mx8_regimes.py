"""GPU tests of the MXFP8 head ops (csrc/conv_mx8.hip) in every regime of their two kernels and of their admission
(rtm3d_op_conv_mx8 / rtm3d_op_quant_mx8 in runtime.hip).  The cases, and the host mirror that says which regime each one runs, are
in tests/mx8_regimes.py; tests/test_mx8_regimes.py checks there, without a GPU, that every regime is covered.

1. conv: exact data (tests/mx8_ref.py: small integers times power-of-two block scales, the L1 bound asserted on the host, so the
   fp32 result is exact in any summation order) against a float64 conv of the dequantised operands.  Every comparison is an
   equality over the WHOLE padded output tensor: the written slices equal the reference (fp16: its fp16 rounding; MX8: the host
   quantisation of it, scales and codes), every other byte keeps what it held - the border as created, the other channels and
   their scales a sentinel.
2. quant: bit-exact against the host quantiser over slices that are not block-aligned, tensors that are no multiple of 32 wide
   and every fp16 value class, NaNs and infinities included (the rule is stated in rtm3d_amd/mx8.py).
3. refusals: every RT_FAIL of the two ops by its message; afterwards the context still runs its ops and no output has changed.

Measured on the MI355X (two runs, the larger figure): test_conv_mx8_regime_exact[b3_straddle_g4] 0.50 s, [d6_cpt8_m600] 0.34 s,
[t1_m1] 0.18 s when it opens the process's first context, [t2_cpt2_m100] 0.10 s, [t80_scale_hi] 0.08 s, every other conv case
0.01-0.05 s, every quant case and every refusal under 0.005 s; the refusals' shared context takes 0.01 s to set up."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, mx8                                    # noqa: E402
from tests import mx8_ref as ref                                   # noqa: E402
from tests import mx8_regimes as mr                                # noqa: E402
from tests.conv_harness import _hip_memcpy, D2H                    # noqa: E402
from tests.test_gpu_mx8 import Ctx                                 # noqa: E402

SENT_CODE, SENT_SCALE, SENT_F16 = 0x5a, 99, 1234.0                 # what an output holds before the op runs (interior)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def _padded(x_nhwc, P):
    """Raw arrays (codes, scales) of an MX8 tensor holding the interior map x: zero border with scale 127, as created."""
    B, H, W, C = x_nhwc.shape
    c, s = mx8.quantize(x_nhwc)
    d = np.zeros((B, H + 2 * P, W + 2 * P, C), np.uint8)
    sc = np.full((B, H + 2 * P, W + 2 * P, C // 32), 127, np.uint8)
    d[:, P:P + H, P:P + W] = c
    sc[:, P:P + H, P:P + W] = s
    return d, sc


def _sentinel_mx8(c, B, H, W, C, P):
    """An MX8 tensor whose interior holds the sentinel code and scale; -> (id, its raw arrays)."""
    t = c.mx8_tensor(B, H, W, C, P)
    d = np.zeros((B, H + 2 * P, W + 2 * P, C), np.uint8)
    s = np.full((B, H + 2 * P, W + 2 * P, C // 32), 127, np.uint8)
    d[:, P:P + H, P:P + W] = SENT_CODE
    s[:, P:P + H, P:P + W] = SENT_SCALE
    c.upload_raw(t, d, s)
    return t, d, s


def _sentinel_f16(c, B, H, W, C, P):
    """An fp16 tensor whose interior holds the sentinel (uploaded through rtm3d_tensor_upload); -> (id, its padded image)."""
    t = c.f16_tensor(B, H, W, C, P)
    c.upload_f16(t, 0, np.full((B, C, H, W), SENT_F16, np.float32))
    img = np.zeros((B, H + 2 * P, W + 2 * P, C), np.float16)
    img[:, P:P + H, P:P + W] = SENT_F16
    return t, img


def _raw_f16(c, tid):
    """The whole padded image (B, Hp, Wp, C) of an fp16 tensor."""
    base = ctypes.c_void_p()
    v = [ctypes.c_int() for _ in range(5)]
    _lib.check(c.lib.rtm3d_tensor_info(c.ctx, tid, ctypes.byref(base), *[ctypes.byref(i) for i in v]), 'tensor_info')
    B, H, W, C, P = [i.value for i in v]
    out = np.empty((B, H + 2 * P, W + 2 * P, C), np.float16)
    torch.cuda.synchronize()
    _hip_memcpy(c.lib, out.ctypes.data, base, out.nbytes, D2H)
    return out


# ------------------------------------------------------------------------------ conv
@pytest.mark.parametrize('case', mr.CONV_CASES, ids=[c['name'] for c in mr.CONV_CASES])
def test_conv_mx8_regime_exact(dev, case):
    B, H, W, G, cout, Po = case['B'], case['H'], case['W'], case['groups'], case['cout'], case['out_P']
    taps = mr.TAPS[case['taps']]
    x, w, bias = ref.conv_case_data(case)
    xq = mx8.dequantize(*mx8.quantize(x))
    wq = np.stack([mx8.dequantized_weights(w[g]) for g in range(G)])
    y = ref.conv(xq, wq, bias, taps, case['in_coff'], case['relu'])                  # exact: the L1 bound holds
    y32 = [v.astype(np.float32) for v in y]
    assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(y32, y))
    c = Ctx(dev)
    try:
        ti = c.mx8_tensor(B, H, W, case['in_C'], case['in_P'])
        c.upload_raw(ti, *_padded(x, case['in_P']))
        inner = (slice(None), slice(Po, Po + H), slice(Po, Po + W))
        if case['out'] == 'f16':
            assert max(float(np.abs(v).max()) for v in y) < 65504.0
            to, want = _sentinel_f16(c, B, H, W, case['out_C'], Po)
            c.conv(ti, to, True, w, bias, taps, case['in_coff'], case['out_coff'], case['relu'])
            c.run()
            for g in range(G):
                want[inner + (slice(case['out_coff'][g], case['out_coff'][g] + cout),)] = y32[g].astype(np.float16)
            got = _raw_f16(c, to)
            np.testing.assert_array_equal(got[inner], want[inner])
            np.testing.assert_array_equal(got, want)                                  # the border too
        else:
            to, want_d, want_s = _sentinel_mx8(c, B, H, W, case['out_C'], Po)
            c.conv(ti, to, False, w, bias, taps, case['in_coff'], case['out_coff'], case['relu'])
            c.run()
            for g in range(G):
                oc = case['out_coff'][g]
                hc, hs = mx8.quantize(y32[g])
                want_d[inner + (slice(oc, oc + cout),)] = hc
                want_s[inner + (slice(oc // 32, (oc + cout) // 32),)] = hs
                if case['zero_block']:
                    assert (hs[..., 1] == 127).all() and not hc[..., 32:64].any() and (hs[..., 0] != 127).all()
                shift = case['sx'] + case['sw']
                if abs(shift) >= 45:                                                  # the two-factor inverse scale
                    assert (np.abs(hs.astype(int) - 127) >= 50).all() and abs(np.median(hs) - 127 - np.sign(shift) * 60) <= 12
            got_d, got_s = c.download_raw(to, want_d.shape)
            np.testing.assert_array_equal(got_s[inner], want_s[inner])
            np.testing.assert_array_equal(got_d[inner], want_d[inner])
            np.testing.assert_array_equal(got_s, want_s)
            np.testing.assert_array_equal(got_d, want_d)
    finally:
        c.close()


# ------------------------------------------------------------------------------ quant
@pytest.mark.parametrize('q', mr.QUANT_CASES, ids=[q[0] for q in mr.QUANT_CASES])
def test_quant_mx8_regime_bit_exact(dev, q):
    name, B, H, W, in_C, in_coff, channels, in_P, out_C, out_coff, out_P, first = q
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x, where = ref.f16_values(rng, (B, H, W, channels), ref.VALUE_CLASSES, first)
    c = Ctx(dev)
    try:
        tf = c.f16_tensor(B, H, W, in_C, in_P)
        c.upload_f16(tf, 0, np.full((B, in_C, H, W), 30000.0, np.float32))            # a misplaced load changes a scale
        c.upload_f16(tf, in_coff, x.transpose(0, 3, 1, 2))
        tq, want_d, want_s = _sentinel_mx8(c, B, H, W, out_C, out_P)
        c.quant(tf, in_coff, tq, out_coff, channels)
        c.run()
        hc, hs = mx8.quantize(x)
        assert not np.isin(hc, (0x7f, 0xff)).any()
        flat_s = hs.reshape(-1)
        for cls, byte in (('all_nan', 127), ('nan_and_inf', 247), ('pos_inf', 247), ('neg_zero', 127), ('only_2m24', 127 - 24 - 8),
                          ('f16_max', 127 + 15 - 8), ('amax_pow2', 127), ('amax_below_pow2', 126)):
            if cls in where:
                assert flat_s[where[cls]] == byte, (cls, flat_s[where[cls]])
        if 'one_nan' in where:
            b = x.reshape(-1, 32)[where['one_nan']]
            assert flat_s[where['one_nan']] == mx8.scale_bytes(np.nanmax(np.abs(b))) and hc.reshape(-1, 32)[where['one_nan'], 9] == 0x7e
        inner = (slice(None), slice(out_P, out_P + H), slice(out_P, out_P + W))
        want_d[inner + (slice(out_coff, out_coff + channels),)] = hc
        want_s[inner + (slice(out_coff // 32, (out_coff + channels) // 32),)] = hs
        got_d, got_s = c.download_raw(tq, want_d.shape)
        np.testing.assert_array_equal(got_s[inner], want_s[inner])
        np.testing.assert_array_equal(got_d[inner], want_d[inner])
        np.testing.assert_array_equal(got_s, want_s)
        np.testing.assert_array_equal(got_d, want_d)
        # the dequantising download is the host's dequantisation of the raw bytes
        deq = np.empty((B, channels, H, W), np.float32)
        _lib.check(c.lib.rtm3d_tensor_download_mx8(c.ctx, tq, out_coff, channels, deq.ctypes.data_as(ctypes.c_void_p)), 'tensor_download_mx8')
        with np.errstate(over='ignore'):
            host = mx8.dequantize(got_d, got_s)[inner + (slice(out_coff, out_coff + channels),)].astype(np.float32)
        np.testing.assert_array_equal(deq, host.transpose(0, 3, 1, 2))
    finally:
        c.close()


# ------------------------------------------------------------------------------ refusals
RB, RH, RW = 1, 4, 6
R_TAPS = mr.TAPS['col']


class _Refusals(object):
    """One context with a valid conv (MX8 -> MX8), a valid conv (MX8 -> fp16) and a valid quant recorded and run, and
    sentinel-filled outputs that the refused ops name."""
    def __init__(self, dev):
        rng = np.random.default_rng(5)
        self.c = c = Ctx(dev)
        x = ref.exact_blocks(rng, (RB, RH, RW, 128), 1)
        self.w = ref.exact_blocks(rng, (2, 3, 256, 64), 1)
        self.bias = rng.integers(-8, 9, (2, 256)).astype(np.float32)
        self.ti = c.mx8_tensor(RB, RH, RW, 128, 1)
        c.upload_raw(self.ti, *_padded(x, 1))
        self.ti96 = c.mx8_tensor(RB, RH, RW, 96, 1)                      # a channel count that is no multiple of 64
        self.tm_ok = c.mx8_tensor(RB, RH, RW, 512, 1)
        self.tf_ok = c.f16_tensor(RB, RH, RW, 512, 1)
        self.tm, self.tm_d, self.tm_s = _sentinel_mx8(c, RB, RH, RW, 512, 1)
        self.tf, self.tf_img = _sentinel_f16(c, RB, RH, RW, 512, 1)
        self.tm_w7 = c.mx8_tensor(RB, RH, RW + 1, 512, 1)                # another map size
        self.tz = c.f16_tensor(RB, RH, RW, 64, 0)
        c.upload_f16(self.tz, 0, rng.standard_normal((RB, 64, RH, RW)).astype(np.float32))
        self.tz68 = c.f16_tensor(RB, RH, RW, 68, 0)                      # a channel count that is no multiple of 8
        self.tq_ok = c.mx8_tensor(RB, RH, RW, 64, 0)
        self.tq, self.tq_d, self.tq_s = _sentinel_mx8(c, RB, RH, RW, 64, 0)
        self.tq_w7 = c.mx8_tensor(RB, RH, RW + 1, 64, 0)
        c.conv(self.ti, self.tm_ok, False, self.w, self.bias, R_TAPS, [0, 64], [0, 256], True)
        c.conv(self.ti, self.tf_ok, True, self.w, self.bias, R_TAPS, [0, 64], [0, 256], False)
        c.quant(self.tz, 0, self.tq_ok, 0, 64)
        packed = [mx8.pack_conv_weights(self.w[g]) for g in range(2)]
        self.wb = np.concatenate([p[0] for p in packed])
        self.sb = np.concatenate([p[1] for p in packed])
        self.blobs = (c.blob(self.wb), c.blob(self.sb), c.blob(self.bias))
        self.short = (c.blob(self.wb[:-64]), c.blob(self.sb[:-2]), c.blob(self.bias.reshape(-1)[:-1]))
        c.run()
        self.first = self.outputs()

    def outputs(self):
        c = self.c
        return [a.copy() for a in c.download_raw(self.tm_ok, self.tm_d.shape) + c.download_raw(self.tq_ok, self.tq_d.shape)] + [_raw_f16(c, self.tf_ok)]

    def desc(self, **k):
        """The valid MX8 -> MX8 conv into the sentinel tensor, with fields replaced."""
        d = _lib.ConvMx8Desc()
        d.in_tensor, d.out_tensor, d.out_fp16 = k.get('in_tensor', self.ti), k.get('out_tensor', self.tm), k.get('out_fp16', 0)
        d.cin, d.cout, d.groups, d.ntaps = k.get('cin', 64), k.get('cout', 256), k.get('groups', 2), k.get('ntaps', 3)
        for g, (i, o) in enumerate(zip(k.get('in_coff', (0, 64)), k.get('out_coff', (0, 256)))):
            d.in_coff[g], d.out_coff[g] = i, o
        for t, (dy, dx) in enumerate(k.get('taps', R_TAPS)):
            d.tap_dy[t], d.tap_dx[t] = dy, dx
        d.relu = 1
        d.w_blob, d.wscale_blob, d.bias_blob = k.get('blobs', self.blobs)
        return d

    def untouched(self):
        c = self.c
        c.run()
        for a, b in zip(self.first, self.outputs()):
            np.testing.assert_array_equal(a, b)
        d, s = c.download_raw(self.tm, self.tm_d.shape)
        assert np.array_equal(d, self.tm_d) and np.array_equal(s, self.tm_s)
        d, s = c.download_raw(self.tq, self.tq_d.shape)
        assert np.array_equal(d, self.tq_d) and np.array_equal(s, self.tq_s)
        np.testing.assert_array_equal(_raw_f16(c, self.tf), self.tf_img)


@pytest.fixture(scope='module')
def refusals(dev):
    r = _Refusals(dev)
    yield r
    r.c.close()


CONV_REFUSALS = [
    # name, fields of the valid desc to replace (names of the fixture's tensors as strings), the message
    ('cin_not_64', dict(cin=96), r'needs cin % 64 == 0 and cout % 256 == 0 \(cin=96 cout=256\)'),
    ('cout_not_256', dict(cout=128), r'needs cin % 64 == 0 and cout % 256 == 0 \(cin=64 cout=128\)'),
    ('cin_zero', dict(cin=0), r'needs cin % 64 == 0'),
    ('in_C_not_64', dict(in_tensor='ti96', groups=1), r"input tensor's channel count 96 is not a multiple of 64"),
    ('tap_up', dict(taps=[(-2, 0), (0, 0), (1, 0)]), r'tap \(-2,0\) leaves the padded input'),
    ('tap_down', dict(taps=[(-1, 0), (0, 0), (2, 0)]), r'tap \(2,0\) leaves the padded input'),
    ('tap_left', dict(taps=[(-1, 0), (0, -2), (1, 0)]), r'tap \(0,-2\) leaves the padded input'),
    ('tap_right', dict(taps=[(-1, 0), (0, 2), (1, 0)]), r'tap \(0,2\) leaves the padded input'),
    ('in_coff_unaligned', dict(in_coff=(32, 64)), r'input slice \[32, 96\) of a 128-channel tensor'),
    ('in_coff_past_end', dict(in_coff=(0, 128)), r'input slice \[128, 192\) of a 128-channel tensor'),
    ('in_coff_negative', dict(in_coff=(-64, 64)), r'input slice \[-64, 0\)'),
    ('out_coff_f16_not_8', dict(out_fp16=1, out_tensor='tf', out_coff=(4, 260)), r'output slice \[4, 260\) of a 512-channel tensor \(offsets multiples of 8\)'),
    ('out_coff_mx8_not_32', dict(out_coff=(8, 264)), r'output slice \[8, 264\) of a 512-channel tensor \(offsets multiples of 32\)'),
    ('out_coff_past_end', dict(out_coff=(0, 288)), r'output slice \[288, 544\) of a 512-channel tensor'),
    ('out_slices_overlap', dict(out_coff=(0, 224)), r'output slices of groups 0 and 1 overlap'),
    ('w_blob_size', dict(blobs=('short', 0)), r'blob sizes 98240 / 3072 / 2048, expected 98304 / 3072 / 2048'),
    ('wscale_blob_size', dict(blobs=('short', 1)), r'blob sizes 98304 / 3070 / 2048, expected'),
    ('bias_blob_size', dict(blobs=('short', 2)), r'blob sizes 98304 / 3072 / 2044, expected'),
    ('bad_blob', dict(blobs=('bad', 0)), r'bad weight / scale / bias blob'),
    ('out_is_in', dict(out_tensor='ti'), r'the output tensor is the input tensor'),
    ('shape_mismatch', dict(out_tensor='tm_w7'), r'input and output maps differ in shape'),
    ('groups_zero', dict(groups=0), r'groups/ntaps out of range'),
    ('groups_five', dict(groups=5), r'groups/ntaps out of range'),
    ('ntaps_zero', dict(ntaps=0), r'groups/ntaps out of range'),
    ('ntaps_81', dict(ntaps=81), r'groups/ntaps out of range'),
    ('out_fp16_two', dict(out_fp16=2), r'out_fp16 must be 0 or 1'),
    ('bad_input', dict(in_tensor=99), r'bad MX8 input tensor 99'),
    ('bad_mx8_output', dict(out_tensor=99), r'bad MX8 output tensor 99'),
    ('bad_f16_output', dict(out_fp16=1, out_tensor=99), r'bad fp16 output tensor 99'),
]


@pytest.mark.parametrize('name,fields,msg', CONV_REFUSALS, ids=[r[0] for r in CONV_REFUSALS])
def test_conv_mx8_refusal(refusals, name, fields, msg):
    r = refusals
    k = dict(fields)
    for key in ('in_tensor', 'out_tensor'):
        if isinstance(k.get(key), str):
            k[key] = getattr(r, k[key])
    if 'blobs' in k:
        kind, i = k['blobs']
        blobs = list(r.blobs)
        blobs[i] = r.short[i] if kind == 'short' else 9999
        k['blobs'] = tuple(blobs)
    d = r.desc(**k)
    with pytest.raises(RuntimeError, match=msg):
        _lib.check(r.c.lib.rtm3d_op_conv_mx8(r.c.ctx, ctypes.byref(d)), 'op_conv_mx8')
    r.untouched()


def test_conv_mx8_refuses_null(refusals):
    with pytest.raises(RuntimeError, match='null argument'):
        _lib.check(refusals.c.lib.rtm3d_op_conv_mx8(refusals.c.ctx, None), 'op_conv_mx8')
    refusals.untouched()


QUANT_REFUSALS = [
    # name, (input, in_coff, output, out_coff, channels), message
    ('bad_input', (99, 0, 'tq', 0, 64), r'bad tensors \(fp16 input 99, MX8 output'),
    ('bad_output', ('tz', 0, 99, 0, 64), r'bad tensors \(fp16 input \d+, MX8 output 99\)'),
    ('shape_mismatch', ('tz', 0, 'tq_w7', 0, 64), r'input and output maps differ in shape'),
    ('channels_not_32', ('tz', 0, 'tq', 0, 48), r'input slice \[0, 48\) of a 64-channel tensor'),
    ('channels_zero', ('tz', 0, 'tq', 0, 0), r'input slice \[0, 0\)'),
    ('in_coff_not_8', ('tz', 4, 'tq', 0, 32), r'input slice \[4, 36\) of a 64-channel tensor'),
    ('in_past_end', ('tz', 8, 'tq', 0, 64), r'input slice \[8, 72\) of a 64-channel tensor'),
    ('in_C_not_8', ('tz68', 0, 'tq', 0, 64), r'input slice \[0, 64\) of a 68-channel tensor'),
    ('out_coff_not_32', ('tz', 0, 'tq', 16, 32), r'output slice \[16, 48\) \(32-channel blocks\)'),
    ('out_coff_negative', ('tz', 0, 'tq', -32, 32), r'output slice \[-32, 0\)'),
    ('out_past_end', ('tz', 0, 'tq', 32, 64), r'output slice \[32, 96\)'),
]


@pytest.mark.parametrize('name,args,msg', QUANT_REFUSALS, ids=[r[0] for r in QUANT_REFUSALS])
def test_quant_mx8_refusal(refusals, name, args, msg):
    r = refusals
    inp, in_coff, out, out_coff, channels = [getattr(r, a) if isinstance(a, str) else a for a in args]
    with pytest.raises(RuntimeError, match=msg):
        r.c.quant(inp, in_coff, out, out_coff, channels)
    r.untouched()
