"""Opt-in MXFP8 head convolutions (head_precision='mxfp8'), the parts that need no GPU: the host quantiser against an independent
restatement of OCP MX v1.0, the plan the option builds (and the fp16 plan it must leave alone), the C ABI additions and the
refused mode combinations."""
import ctypes
import hashlib
import math
import os
import re

import numpy as np
import pytest
import torch

import rtm3d_amd
from rtm3d_amd import _lib, mx8, plan, weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ quantiser
def _reference_quantize(x):
    """OCP MX v1.0 restated with math.frexp exponents and torch's float8_e4m3fn cast (which does NOT saturate: clamp first)."""
    x = np.asarray(x, np.float32)
    blocks = x.reshape(-1, 32).astype(np.float64)
    codes = np.empty(blocks.shape, np.uint8)
    scales = np.empty(len(blocks), np.uint8)
    for i, b in enumerate(blocks):
        amax = float(np.abs(b).max())
        if amax == 0.0:
            e = 0
        else:
            m, ex = math.frexp(amax)                   # amax = m * 2^ex, m in [0.5, 1)
            e = min(max(ex - 1 - 8, -127), 127)
        scales[i] = e + 127
        y = torch.from_numpy(np.clip(b * 2.0 ** -e, -448.0, 448.0).astype(np.float32))
        codes[i] = y.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return codes.reshape(x.shape), scales.reshape(x.shape[:-1] + (x.shape[-1] // 32,))


def _cases():
    rng = np.random.default_rng(5)
    out = {'random': (rng.standard_normal((64, 128)) * np.exp2(rng.integers(-20, 20, (64, 1)))).astype(np.float32)}
    # ties: amax 256 -> scale 2^0; values halfway between e4m3 neighbours in every binade
    t = np.zeros((16, 32), np.float32)
    t[:, 0] = 256.0
    vals = [1.0625, 1.1875, 2.125, 2.375, 17.0, 19.0, 136.0, 152.0, 0.0029296875, 0.0048828125, 272.0, 304.0, 0.00390625 * 1.0625]
    for j, v in enumerate(vals):
        t[:, 1 + j] = v
        t[::2, 1 + j] *= -1
    out['ties'] = t
    # subnormals: after scaling, values far below the block max land in e4m3's subnormal range (quantum 2^-9)
    s = np.zeros((8, 32), np.float32)
    s[:, 0] = 300.0
    s[:, 1:] = rng.uniform(-0.02, 0.02, (8, 31)).astype(np.float32)
    s[:, 5] = 2.0 ** -10 * 1.5                          # three quarters of the smallest e4m3 subnormal (after scaling): rounds up to it
    out['subnormal'] = s
    out['fp32_subnormal_block'] = np.full((2, 32), 1e-40, np.float32)
    z = rng.standard_normal((4, 96)).astype(np.float32)
    z[1, 32:64] = 0.0
    z[3, :32] = 0.0
    out['zero_block'] = z
    # > 448 after scaling: amax in the top of a binade (e.g. 511 / 2^0 = 511 > 464 would be NaN in torch without a clamp)
    big = rng.uniform(-1, 1, (8, 32)).astype(np.float32) * 500.0
    big[:, 0] = 511.0
    big[:, 1] = -470.0
    big[:, 2] = 460.0
    out['above_448'] = big
    out['huge'] = (rng.standard_normal((4, 64)) * 1e37).astype(np.float32)
    return out


@pytest.mark.parametrize('case', sorted(_cases()))
def test_host_quantiser_matches_independent_restatement(case):
    x = _cases()[case]
    codes, scales = mx8.quantize(x)
    rc, rs = _reference_quantize(x)
    np.testing.assert_array_equal(scales, rs)
    np.testing.assert_array_equal(codes, rc)
    assert not np.isnan(mx8.dequantize(codes, scales)).any()


def test_quantiser_saturates_and_keeps_zero_blocks_at_scale_one():
    x = np.zeros((1, 64), np.float32)
    x[0, 32] = 511.0
    x[0, 33] = -465.0
    c, s = mx8.quantize(x)
    assert s.tolist() == [[127, 127]]                     # floor(log2 511) - 8 = 0; the zero block gets 127 as well
    assert c[0, 32] == 0x7e and c[0, 33] == 0xfe          # 511 and -465 saturate to +-448 (torch's cast would give NaN)
    assert not c[0, :32].any()


def test_dequantize_inverts_exact_values():
    rng = np.random.default_rng(2)
    ints = rng.integers(-8, 9, (16, 64)).astype(np.float32)
    ints[:, ::32] = 8                                     # every block holds an 8
    x = ints * np.exp2(rng.integers(-3, 4, (16, 2))).repeat(32, 1).astype(np.float32)
    c, s = mx8.quantize(x)
    np.testing.assert_array_equal(mx8.dequantize(c, s), x)


def test_weight_packing_layout():
    rng = np.random.default_rng(3)
    wt = rng.standard_normal((9, 512, 128)).astype(np.float32)   # taps, cout, cin
    w, s = mx8.pack_conv_weights(wt)
    codes, sb = mx8.quantize(wt)
    kt = 9 * 2
    w = w.reshape(2, kt, 256, 64)
    s = s.reshape(2, kt, 256, 2)
    for nt, tap, q, row in [(0, 0, 0, 0), (1, 8, 1, 255), (1, 4, 0, 17), (0, 3, 1, 200)]:
        k = tap * 2 + q
        np.testing.assert_array_equal(w[nt, k, row], codes[tap, nt * 256 + row, q * 64:(q + 1) * 64])
        np.testing.assert_array_equal(s[nt, k, row], sb[tap, nt * 256 + row, 2 * q:2 * q + 2])


# ------------------------------------------------------------------------------ plans
def _structure_digest(P):
    """sha256 over the tensors, op kinds, names, slices, taps and array SHAPES of a plan (not the weight values)."""
    h = hashlib.sha256()

    def put(v):
        h.update(repr(v).encode())
    put([sorted(t.items()) for t in P.tensors])
    for op in P.ops:
        for k in sorted(op):
            v = op[k]
            if isinstance(v, np.ndarray):
                put((k, v.shape, str(v.dtype)))
            elif isinstance(v, (list, tuple)):
                put((k, [(s.tid, s.coff, s.C) if hasattr(s, 'tid') else s for s in v]))
            elif hasattr(v, 'tid'):
                put((k, (v.tid, v.coff, v.C)))
            else:
                put((k, v))
    return h.hexdigest()


# digests of the plans built before head_precision existed (B=2, 64 x 128, synthetic 'trained' weights, seed 1)
FP16_PLAN_DIGESTS = {
    ('DLA-34', 1): '9a6e98f4ef28a9f108ebb507fe170ea6240ecd10d7d0dda59ee55288af4efa2d',
    ('DLA-34', 2): '1f3baba530c0b05c82c81057d17e060f72e727a81c6e4fc52de518d7867b9ea8',
    ('DLA-34', 3): '4a31bfe4fadb1a414dd03c8b2e62a795aeb60d3439d7246e8b9cbc44cd9bc880',
    ('RESNET-18', 2): 'afb41510e01ccedb171d91b09d0738880c035913d0519b2701335610374c42f3',
}


@pytest.mark.parametrize('bb,nc', sorted(FP16_PLAN_DIGESTS))
def test_fp16_plan_unchanged(bb, nc):
    sd = weights.synth_state_dict(bb, 1, 'trained', header_num_conv=nc)
    P0 = plan.build_plan(sd, bb, 2, 64, 128, header_num_conv=nc)
    P1 = plan.build_plan(sd, bb, 2, 64, 128, header_num_conv=nc, head_precision='fp16')
    assert _structure_digest(P0) == FP16_PLAN_DIGESTS[(bb, nc)]
    assert _structure_digest(P1) == FP16_PLAN_DIGESTS[(bb, nc)]
    for a, b in zip(P0.ops, P1.ops):
        for k in ('w', 'bias'):
            if k in a and isinstance(a[k], np.ndarray):
                np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize('nc', [1, 2, 3])
def test_mxfp8_plan_ops_and_formats(nc):
    bb = 'DLA-34'
    sd = weights.synth_state_dict(bb, 1, 'trained', header_num_conv=nc)
    P0 = plan.build_plan(sd, bb, 2, 64, 128, header_num_conv=nc)
    P = plan.build_plan(sd, bb, 2, 64, 128, header_num_conv=nc, head_precision='mxfp8')
    # everything up to the fused map z is the fp16 plan's
    kz = next(i for i, op in enumerate(P0.ops) if op['op'] == 'softmax')
    assert [op['name'] for op in P.ops[:kz + 1]] == [op['name'] for op in P0.ops[:kz + 1]]
    heads = P.ops[kz + 1:]
    fmt = lambda s: P.tensors[s.tid].get('fmt', 'fp16')       # noqa: E731
    names = ['heads.quant_z', 'heads.conv_d6'] + ['heads.conv_d1' if k == 1 else 'heads.conv_d1_%d' % k for k in range(1, nc)] + ['heads.out_convs']
    assert [op['name'] for op in heads] == names
    assert [op['op'] for op in heads] == ['quant_mx8'] + ['conv_mx8'] * nc + ['headout']
    q = heads[0]
    assert q['inp'].tid == P.named['z'].tid and fmt(q['out']) == 'mx8' and P.tensors[q['out'].tid]['pad'] == 6
    d6 = heads[1]
    assert d6['groups'] == 1 and d6['cin'] == 256 and d6['cout'] == 1024 and d6['relu']
    assert d6['taps'] == [(dy, dx) for dy in (-6, 0, 6) for dx in (-6, 0, 6)]
    convs = heads[1:1 + nc]
    for k, op in enumerate(convs):
        last = k == nc - 1
        assert op['out_fp16'] == last and all(fmt(o) == ('fp16' if last else 'mx8') for o in op['out'])
        assert all(fmt(i) == 'mx8' for i in op['inp'])
        if k:
            assert op['groups'] == 4 and op['cin'] == op['cout'] == 256 and op['taps'] == [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            assert [i.coff for i in op['inp']] == [0, 256, 512, 768] and op['inp'][0].tid == convs[k - 1]['out'][0].tid
            assert op['out'][0].tid != op['inp'][0].tid
    assert heads[-1]['inp'].tid == convs[-1]['out'][0].tid and fmt(heads[-1]['inp']) == 'fp16'
    assert P.tensors[heads[-1]['inp'].tid]['pad'] >= 1
    # same weights as the fp16 plan's head convs (what gets quantised is the BN-folded fp32 array)
    f16_heads = [op for op in P0.ops[kz + 1:] if op['op'] == 'conv']
    for a, b in zip(f16_heads, convs):
        np.testing.assert_array_equal(a['bias'], b['bias'])
        np.testing.assert_array_equal(a['w'].reshape(b['w'].shape), b['w'])
    assert P.total_flops() == pytest.approx(P0.total_flops())


def test_mxfp8_plan_refuses_peaks_and_bad_names():
    sd = weights.synth_state_dict('DLA-34', 1, 'trained')
    with pytest.raises(NotImplementedError, match='dense heads'):
        plan.build_plan(sd, 'DLA-34', 1, 64, 128, dense_heads=1, head_precision='mxfp8')
    with pytest.raises(ValueError, match='head_precision'):
        plan.build_plan(sd, 'DLA-34', 1, 64, 128, head_precision='fp8')


# ------------------------------------------------------------------------------ C ABI
NEW_EXPORTS = ['rtm3d_tensor_create_mx8', 'rtm3d_tensor_download_mx8', 'rtm3d_tensor_download_mx8_raw', 'rtm3d_tensor_upload_mx8_raw',
               'rtm3d_op_quant_mx8', 'rtm3d_op_conv_mx8']


def test_mx8_prototypes_in_header_and_binding():
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert re.search(r'#define RTM3D_ABI_VERSION 9\b', hdr) and _lib.ABI_VERSION == 9
    for name in NEW_EXPORTS:
        m = re.search(r'\b(?:int|void)\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
    assert 'typedef struct rtm3d_conv_mx8_desc' in hdr


def test_conv_mx8_desc_layout_matches_header():
    import shutil
    import subprocess
    import tempfile
    cc = shutil.which('gcc') or shutil.which('cc')
    if cc is None:
        pytest.fail('no C compiler to check the descriptor layout')
    fields = [f for f, _ in _lib.ConvMx8Desc._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s/include/rtm3d_hip.h"\nint main(){printf("%%zu", sizeof(rtm3d_conv_mx8_desc));%s return 0;}'
           % (REPO, ''.join('printf(" %%zu", offsetof(rtm3d_conv_mx8_desc, %s));' % f for f in fields)))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'l.c')
        open(c, 'w').write(src)
        subprocess.check_call([cc, c, '-o', os.path.join(d, 'l')])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, 'l')]).split()]
    assert vals[0] == ctypes.sizeof(_lib.ConvMx8Desc)
    assert vals[1:] == [getattr(_lib.ConvMx8Desc, f).offset for f in fields]


# ------------------------------------------------------------------------------ refused combinations (raised before any device work)
def test_refused_mode_combinations():
    cfg = rtm3d_amd.kitti_config('DLA-34')
    with pytest.raises(ValueError, match='head_precision'):
        rtm3d_amd.create_model(cfg, head_precision='int8')
    m = rtm3d_amd.create_model(cfg, head_precision='mxfp8')
    assert m.head_precision == 'mxfp8'
    assert rtm3d_amd.create_model(cfg).head_precision == 'fp16'
    x, K = object(), object()
    with pytest.raises(NotImplementedError, match='sparse_heads'):
        m.detect3d(x, K, sparse_heads=True)
    with pytest.raises(ValueError, match='fp32_verify'):
        m.detect3d(x, K, fp32_verify=True)
    m16 = rtm3d_amd.create_model(cfg)
    with pytest.raises(NotImplementedError, match='sparse_heads'):
        m16.detect3d(x, K, sparse_heads=True, head_precision='mxfp8')
    with pytest.raises(ValueError, match='fp32_verify'):
        m16.detect3d(x, K, fp32_verify=True, head_precision='mxfp8')
    with pytest.raises(NotImplementedError):
        m16._plan_for(1, 64, 128, torch.device('cuda', 0), 'peaks', 'mxfp8')
    from rtm3d_amd.pipeline import Detect3DPipeline
    with pytest.raises(NotImplementedError, match='sparse_heads'):
        Detect3DPipeline(m16, 1, 'cuda:0', sparse_heads=True, head_precision='mxfp8')


# ------------------------------------------------------------------------------ non-finite values: the device's rule
def test_quantiser_nan_never_reaches_a_scale():
    """fmax semantics (quant_mx8_kernel): the scale comes from the block's other values, the NaN element becomes sign | 0x7e
    (+-448 in the block's scale), an all-NaN block gets byte 127; code 0x7f / 0xff is never written."""
    nan, nnan = np.float32(np.nan), np.copysign(np.float32(np.nan), np.float32(-1.0))
    x = np.zeros((4, 32), np.float32)
    x[0, :4] = [3.0, nan, -1.5, nnan]                       # one block with NaNs of both signs among finite values
    x[1, :4] = [nan, np.inf, -2.0, nnan]                    # NaN plus an infinity
    x[2, :] = nan                                           # all NaN
    x[2, 1::2] = nnan
    x[3, :3] = [3.0, -1.5, 0.0]                             # block 0 without its NaNs
    c, s = mx8.quantize(x)
    assert s[:, 0].tolist() == [mx8.scale_bytes(np.float32(3.0)), 247, 127, mx8.scale_bytes(np.float32(3.0))]
    assert s[0, 0] == 127 + 1 - 8
    assert c[0, :4].tolist() == [c[3, 0], 0x7e, c[3, 1], 0xfe] and not c[0, 4:].any()
    assert c[1, :4].tolist() == [0x7e, 0x7e, 0x80, 0xfe]    # -2 x 2^-120 rounds to -0
    assert c[2, ::2].tolist() == [0x7e] * 16 and c[2, 1::2].tolist() == [0xfe] * 16
    assert not np.isin(c, (0x7f, 0xff)).any()
    d = mx8.dequantize(c, s)
    assert not np.isnan(d).any() and d[0, 1] == 448.0 * 2.0 ** -7 and d[0, 3] == -448.0 * 2.0 ** -7 and d[2, 0] == 448.0


def test_quantiser_infinities_saturate_at_the_largest_scale():
    x = np.ones((1, 64), np.float32)
    x[0, 3], x[0, 40] = np.inf, -np.inf
    c, s = mx8.quantize(x)
    assert s.tolist() == [[247, 247]] and c[0, 3] == 0x7e and c[0, 40] == 0xfe
    assert not np.delete(c[0], [3, 40]).any()               # 2^-120 rounds to zero


def test_value_classes_of_the_regime_suite_quantise_without_nan_codes():
    from tests import mx8_ref
    rng = np.random.default_rng(4)
    for name in mx8_ref.VALUE_CLASSES:
        b = mx8_ref.value_block(name, rng)
        c, s = mx8.quantize(b[None])
        assert not np.isin(c, (0x7f, 0xff)).any(), name
        if name not in mx8_ref.NAN_CLASSES:
            rc, rs = _reference_quantize(np.where(np.isinf(b), np.sign(b) * np.float32(3e38), b)[None])
            if not np.isinf(b).any():
                np.testing.assert_array_equal(s, rs, name)
                np.testing.assert_array_equal(c, rc, name)
