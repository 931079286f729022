"""GPU (-m gpu): the fused DLA backbone launches - the level tail (conv64_root.hip, all six <POOL, S2D, NORM> instances), the level
entry (conv32s2_fused.hip), the stem (conv_stem_fused.hip, two- and three-layer forms) and the space-to-depth max-pool
(rtm3d_op_maxpool_s2d) - over every regime their admission accepts, against a float64 reference on fp16 operands.

Every case first asserts its op name and its regime (tests/fused_routes.py: the instance, the `single` / ticket regime, the
stem's form, the pool's idle lanes).  Then it checks the numbers with every output poisoned and read back raw from the device:
NaN in every written slice (a skipped tile cannot pass), SENTINEL in every other channel below and above it (must be untouched),
a zero border (the next conv reads it as padding).  Tensors a fused launch never writes (x2, the ordinary root output of a
NORM = 0 launch, the stem's intermediate maps) must come back exactly as uploaded.  CASES is importable without a GPU:
tests/test_fused_routes.py checks it against the mirror and against the product plans' regimes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import plan as plan_mod, _lib                                        # noqa: E402
from tests import fused_routes as fr                                                 # noqa: E402
from tests.conv_harness import SENTINEL, every_pair_order, f16, raw_read, raw_write   # noqa: E402
from tests.test_gpu_conv128 import Conv                                              # noqa: E402

CUS = 256                       # the mirror's CU count (MI355X, SPX: 8 XCDs x 32)
to_s2d = Conv.to_s2d            # (B, H, W, C) -> (B, H / 2, W / 2, 4 C), channels ((y & 1) * 2 + (x & 1)) * C + c


def from_s2d(a):
    B, H2, W2, C4 = a.shape
    return a.reshape(B, H2, W2, 2, 2, C4 // 4).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, C4 // 4)


def setup_module():
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, 'the mirror assumes %d CUs' % CUS


# ---------------------------------------------------------------------------------------------------------------- case specs
def root(B, H, W, pool=True, s2d=False, norm=True, conv_relu=True, root_relu=True, in_lo=0, in_hi=0, out_lo=0, out_hi=0,
         p_lo=0, p_hi=0, s_lo=0, s_hi=0, shared=None, expect=None):
    """A level tail on an H x W map.  shared: the pooled slice and the space-to-depth slice are adjacent in ONE tensor,
    'pool_first' or 's2d_first' (from channel s_lo on; p_lo / p_hi unused)."""
    assert not shared or (pool and s2d)
    return dict(kind='conv64_root', B=B, H=H, W=W, pool=pool, s2d=s2d, norm=norm, conv_relu=conv_relu, root_relu=root_relu,
                in_lo=in_lo, in_hi=in_hi, out_lo=out_lo, out_hi=out_hi, p_lo=p_lo, p_hi=p_hi, s_lo=s_lo, s_hi=s_hi, shared=shared,
                expect=expect or {})


def entry(B, Ho, Wo, in_lo=0, in_hi=0, c_lo=0, c_hi=0, p_lo=0, p_hi=0, c_P=1, p_P=0, shared=False, expect=None):
    """A level entry with an Ho x Wo output map.  shared: the conv slice [c_lo, c_lo + 64) and the project slice right behind
    it in ONE tensor (p_lo / p_hi / p_P unused)."""
    return dict(kind='conv32s2_fused', B=B, Ho=Ho, Wo=Wo, in_lo=in_lo, in_hi=in_hi, c_lo=c_lo, c_hi=c_hi, p_lo=p_lo, p_hi=p_hi,
                c_P=c_P, p_P=p_P, shared=shared, expect=expect or {})


def stem(B, H, W, layers, o_lo=0, o_hi=0, o_P=1, expect=None):
    return dict(kind='stem_fused', B=B, H=H, W=W, layers=layers, o_lo=o_lo, o_hi=o_hi, o_P=o_P, expect=expect or {})


def pool_s2d(B, Ho, Wo, C, in_lo=0, in_hi=0, o_lo=0, o_hi=0, shared=False, expect=None):
    """rtm3d_op_maxpool_s2d of C channels.  shared: input and output are slices of ONE tensor (o_hi unused)."""
    return dict(kind='maxpool_s2d', B=B, Ho=Ho, Wo=Wo, C=C, in_lo=in_lo, in_hi=in_hi, o_lo=o_lo, o_hi=o_hi, shared=shared,
                expect=expect or {})


def mirror(sp):
    k = sp['kind']
    if k == 'conv64_root':
        return fr.conv64_root(sp['B'], sp['H'], sp['W'], sp['pool'], sp['s2d'], sp['norm'], CUS)
    if k == 'conv32s2_fused':
        return fr.conv32s2(sp['B'], sp['Ho'], sp['Wo'], CUS)
    if k == 'stem_fused':
        return fr.stem(sp['B'], sp['H'], sp['W'], sp['layers'])
    return fr.maxpool_s2d(sp['B'], sp['Ho'], sp['Wo'], sp['C'])


def regime(sp):
    """The case's regime key (tests/fused_routes.py: regime_key), as the coverage guard compares it with the product plans'."""
    r, k = mirror(sp), sp['kind']
    if k == 'conv64_root':
        return fr.regime_key(k, single=r['single'], instance=r['instance'], conv_relu=sp['conv_relu'], root_relu=sp['root_relu'])
    if k == 'conv32s2_fused':
        return fr.regime_key(k, single=r['single'])
    if k == 'stem_fused':
        return fr.regime_key(k, layers=sp['layers'])
    return fr.regime_key(k, channels=sp['C'], idle=r['idle'])


def check_regime(sp):
    r = mirror(sp)
    for key, want in sp['expect'].items():
        assert r[key] == want, (key, r[key], want, r)
    return r


def op_name(sp):
    k = sp['kind']
    if k == 'conv64_root':
        return fr.root_name(sp['pool'], sp['s2d'])
    if k == 'conv32s2_fused':
        return 'pool+proj1x1+conv3x3s2_fused'
    if k == 'stem_fused':
        return fr.STEM_NAMES[sp['layers']]
    return 'maxpool_s2d'


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', torch.float64)


def conv_f64(x, w, b, stride=1):
    """x: (B, H, W, cin) float64 (no border), w: (cout, cin, k, k), b: (cout,): k x k conv, zero padding (k - 1) / 2."""
    cout, _, k, _ = w.shape
    p = (k - 1) // 2
    B, H, W, _ = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p))
    acc = b.expand(B, Ho, Wo, cout).clone()
    for ky in range(k):
        for kx in range(k):
            acc += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] @ w[:, :, ky, kx].T
    return acc


def h16(t):
    """Rounded to fp16 (a map the kernel keeps in fp16 before the next layer reads it)."""
    return t.to(torch.float16).to(torch.float64)


def close(got, ref, rtol, what):
    ref = ref.cpu().numpy() if torch.is_tensor(ref) else ref
    np.testing.assert_allclose(got.astype(np.float32), ref.astype(np.float16).astype(np.float32), rtol=rtol,
                               atol=rtol * max(1.0, float(np.abs(ref).max())), err_msg=what)


def weights(rng, cout, cin, k):
    return f16(rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)


def bias(rng, n):
    return (rng.standard_normal(n) * 0.3).astype(np.float32)


def image(rng, B, H, W, C, P, fill=None, relu=False):
    """A padded NHWC image: zero border, N(0, 1) in fp16 (max(., 0) with relu), or `fill` everywhere inside."""
    img = np.zeros((B, H + 2 * P, W + 2 * P, C), np.float16)
    if fill is not None:
        img[:, P:P + H, P:P + W] = fill
    else:
        v = rng.standard_normal((B, H, W, C))
        img[:, P:P + H, P:P + W] = f16(np.maximum(v, 0) if relu else v)
    return img


# ---------------------------------------------------------------------------------------------------------------- the cases
class Case(object):
    """One fused op of a plan with tensors of its own.  self.inputs: [(Slice, image)] uploaded once; self.checked: [(Slice,
    H, W, P, base image, written channel ranges)]: before every forward the tensor is set to its base image with NaN in the
    written ranges; afterwards every channel outside them must equal the base image bit for bit (border included), and
    every written value must be finite."""

    def __init__(self, P, sp, rng):
        self.sp, self.k0 = sp, None
        self.inputs, self.checked = [], []
        self.build(P, rng)
        self.ref = None
        self.seen = False

    def out_tensor(self, P, H, W, C, pad, ranges, base=None):
        s = P.tensor(H, W, C, pad)
        if base is None:
            base = image(None, self.sp['B'], H, W, C, pad, fill=SENTINEL)
        self.checked.append((s, H, W, pad, base, ranges))
        return s

    def lowered(self, L):
        assert L['kind'] == self.sp['kind'], (L['kind'], self.sp['kind'], L['name'])
        self.seen = True

    def poisoned(self):
        for s, H, W, pad, base, ranges in self.checked:
            img = base.copy()
            for lo, hi in ranges:
                img[:, pad:pad + H, pad:pad + W, lo:hi] = np.nan
            yield s, img

    def verify(self, raws):
        """raws: the raw images of self.checked after a forward -> [inner (B, H, W, C) fp16 image] of each."""
        inner = []
        for (s, H, W, pad, base, ranges), got in zip(self.checked, raws):
            written = np.zeros(got.shape, bool)
            for lo, hi in ranges:
                written[:, pad:pad + H, pad:pad + W, lo:hi] = True
            bad = (got.view(np.uint16) != base.view(np.uint16)) & ~written
            assert not bad.any(), '%s: %d values outside the written slices changed (first at %s)' % (
                op_name(self.sp), int(bad.sum()), np.argwhere(bad)[0].tolist())
            vals = got[written]
            assert np.isfinite(vals).all(), '%s: %d written values never stored (NaN poison)' % (op_name(self.sp), int((~np.isfinite(vals)).sum()))
            inner.append(got[:, pad:pad + H, pad:pad + W])
        return inner


class Root(Case):
    """conv64_root.hip: x2 = [ReLU](conv3x3(t) + bc + x1) in fp16, out = [ReLU](root1x1(cat[x2, x1]) + br), pool = 2x2 max of
    out, s2d = out in space-to-depth layout."""

    def build(self, P, rng):
        sp = self.sp
        B, H, W = sp['B'], sp['H'], sp['W']
        self.tt = P.tensor(H, W, sp['in_lo'] + 64 + sp['in_hi'], 1)
        self.t_img = image(rng, B, H, W, self.tt.C, 1)
        self.inputs.append((self.tt, self.t_img))
        # cat = [x2 | x1]: x2 is never written by the fused launch (SENTINEL stays), x1 is read
        cat_img = image(rng, B, H, W, 128, 1)
        cat_img[:, 1:-1, 1:-1, :64] = SENTINEL
        self.x1 = cat_img[:, 1:-1, 1:-1, 64:].copy()
        cat = self.out_tensor(P, H, W, 128, 1, [], base=cat_img)
        self.inputs.append((cat, cat_img))
        self.wc, self.bc = weights(rng, 64, 64, 3), bias(rng, 64)
        self.wr, self.br = weights(rng, 64, 128, 1), bias(rng, 64)
        self.ot = self.out_tensor(P, H, W, sp['out_lo'] + 64 + sp['out_hi'], 1, [(sp['out_lo'], sp['out_lo'] + 64)] if sp['norm'] else [])
        out = P.sub(self.ot, sp['out_lo'], 64)
        self.pool = self.st = None
        if sp['shared']:
            pool_first = sp['shared'] == 'pool_first'
            p0, s0 = (sp['s_lo'], sp['s_lo'] + 64) if pool_first else (sp['s_lo'] + 256, sp['s_lo'])
            t = self.out_tensor(P, H // 2, W // 2, sp['s_lo'] + 320 + sp['s_hi'], 1, [(p0, p0 + 64), (s0, s0 + 256)])
            self.pool, self.st, self.pool_c, self.s_c = t, t, p0, s0
        else:
            if sp['pool']:
                self.pool = self.out_tensor(P, H // 2, W // 2, sp['p_lo'] + 64 + sp['p_hi'], 1, [(sp['p_lo'], sp['p_lo'] + 64)])
                self.pool_c = sp['p_lo']
            if sp['s2d']:
                self.st = self.out_tensor(P, H // 2, W // 2, sp['s_lo'] + 256 + sp['s_hi'], 1, [(sp['s_lo'], sp['s_lo'] + 256)])
                self.s_c = sp['s_lo']
        self.k0 = len(P.ops)
        P.conv(P.sub(self.tt, sp['in_lo'], 64), P.sub(cat, 0, 64), self.wc, self.bc, relu=sp['conv_relu'], res=P.sub(cat, 64, 64), name='tail%d' % self.k0)
        P.conv(cat, out, self.wr, self.br, relu=sp['root_relu'], name='tail%d.root' % self.k0)
        if sp['pool']:
            P.maxpool(out, P.sub(self.pool, self.pool_c, 64), 2, 2, 0, name='tail%d.pool' % self.k0)

    def lowered(self, L):
        Case.lowered(self, L)
        assert L['ops'] == list(range(self.k0, self.k0 + (3 if self.sp['pool'] else 2))), L['ops']
        L['s2d_out'] = (self.st, self.s_c) if self.sp['s2d'] else None
        L['write_out'] = self.sp['norm']

    def reference(self):
        sp = self.sp
        t = dev64(self.t_img[:, 1:-1, 1:-1, sp['in_lo']:sp['in_lo'] + 64])
        x1 = dev64(self.x1)
        x2 = conv_f64(t, dev64(self.wc), dev64(self.bc)) + x1
        x2 = h16(x2.relu() if sp['conv_relu'] else x2)
        o = torch.cat([x2, x1], -1) @ dev64(self.wr[:, :, 0, 0]).T + dev64(self.br)
        return (o.relu() if sp['root_relu'] else o).cpu().numpy()

    def check(self, inner):
        sp = self.sp
        got = dict(zip([id(c[0]) for c in self.checked], inner))
        if self.ref is None:
            self.ref = self.reference()
        s2d = got[id(self.st)][..., self.s_c:self.s_c + 256] if sp['s2d'] else None
        if sp['norm']:
            y = got[id(self.ot)][..., sp['out_lo']:sp['out_lo'] + 64]
            if sp['s2d']:
                # the space-to-depth copy holds the very registers of the ordinary copy
                np.testing.assert_array_equal(s2d.view(np.uint16), to_s2d(y).view(np.uint16))
        else:
            y = from_s2d(s2d)
        close(y, self.ref, 4e-3, 'root output')
        if sp['pool']:
            p = got[id(self.pool)][..., self.pool_c:self.pool_c + 64].astype(np.float32)
            B, H, W = y.shape[:3]
            want = y.astype(np.float32).reshape(B, H // 2, 2, W // 2, 2, 64).max(axis=(2, 4))
            np.testing.assert_array_equal(p, want, err_msg='the pooled map is not the 2x2 max of the root output')


class Entry(Case):
    """conv32s2_fused.hip: proj = project1x1(max_pool2d(x, 2)) + bp (no ReLU), mid = ReLU(conv3x3 stride 2 (x) + bc)."""

    def build(self, P, rng):
        sp = self.sp
        B, Ho, Wo = sp['B'], sp['Ho'], sp['Wo']
        H, W = 2 * Ho, 2 * Wo
        xt = P.tensor(H, W, sp['in_lo'] + 32 + sp['in_hi'], 1)
        self.x_img = image(rng, B, H, W, xt.C, 1, relu=True)          # post-ReLU: exact zeros tie in the max-pool
        self.inputs.append((xt, self.x_img))
        xs = P.sub(xt, sp['in_lo'], 32)
        bottom = self.out_tensor(P, Ho, Wo, 32, 0, [])                  # the pooled map is never materialised
        self.wp, self.bp = weights(rng, 64, 32, 1), bias(rng, 64)
        self.wc, self.bc = weights(rng, 64, 32, 3), bias(rng, 64)
        c0 = sp['c_lo']
        if sp['shared']:
            self.ct = self.pt = self.out_tensor(P, Ho, Wo, c0 + 128 + sp['c_hi'], sp['c_P'], [(c0, c0 + 64), (c0 + 64, c0 + 128)])
            self.c_c, self.p_c = c0, c0 + 64
        else:
            self.ct = self.out_tensor(P, Ho, Wo, c0 + 64 + sp['c_hi'], sp['c_P'], [(c0, c0 + 64)])
            self.pt = self.out_tensor(P, Ho, Wo, sp['p_lo'] + 64 + sp['p_hi'], sp['p_P'], [(sp['p_lo'], sp['p_lo'] + 64)])
            self.c_c, self.p_c = c0, sp['p_lo']
        self.k0 = len(P.ops)
        P.maxpool(xs, bottom, 2, 2, 0, name='entry%d.downsample' % self.k0)
        P.conv(bottom, P.sub(self.pt, self.p_c, 64), self.wp, self.bp, name='entry%d.project' % self.k0)
        P.conv(xs, P.sub(self.ct, self.c_c, 64), self.wc, self.bc, stride=2, relu=True, name='entry%d.tree1.conv1' % self.k0)

    def lowered(self, L):
        Case.lowered(self, L)
        assert L['ops'] == [self.k0, self.k0 + 1, self.k0 + 2], L['ops']

    def reference(self):
        sp = self.sp
        x = dev64(self.x_img[:, 1:-1, 1:-1, sp['in_lo']:sp['in_lo'] + 32])
        B, H, W, _ = x.shape
        pooled = x.reshape(B, H // 2, 2, W // 2, 2, 32).amax(dim=(2, 4))
        proj = pooled @ dev64(self.wp[:, :, 0, 0]).T + dev64(self.bp)
        mid = conv_f64(x, dev64(self.wc), dev64(self.bc), stride=2).relu()
        return proj.cpu().numpy(), mid.cpu().numpy()

    def check(self, inner):
        if self.ref is None:
            self.ref = self.reference()
        got = dict(zip([id(c[0]) for c in self.checked], inner))
        close(got[id(self.pt)][..., self.p_c:self.p_c + 64], self.ref[0], 3e-3, 'project output')
        close(got[id(self.ct)][..., self.c_c:self.c_c + 64], self.ref[1], 3e-3, 'stride-2 conv output')


class Stem(Case):
    """conv_stem_fused.hip: base = ReLU(7x7(x) + b0), l0 = ReLU(3x3(base) + b1) [, l1 = ReLU(3x3 stride 2 (l0) + b2)], the
    16-channel maps kept in fp16; the input is the caller's fp32 NCHW batch."""

    def build(self, P, rng):
        sp = self.sp
        B, H, W = sp['B'], sp['H'], sp['W']
        self.x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
        self.w0, self.b0 = weights(rng, 16, 3, 7), bias(rng, 16)
        self.w1, self.b1 = weights(rng, 16, 16, 3), bias(rng, 16)
        self.w2, self.b2 = weights(rng, 32, 16, 3), bias(rng, 32)
        three = sp['layers'] == 3
        oc = 32 if three else 16
        Ho, Wo = (H // 2, W // 2) if three else (H, W)
        base = self.out_tensor(P, H, W, 16, 1, [])                      # the intermediate maps never leave the kernel
        self.k0 = len(P.ops) + 1                                        # (stem_mfma records the NHWC4 conversion first)
        P.stem_mfma(base, self.w0, self.b0, 1, name='stem%d.base' % self.k0)
        self.ot = self.out_tensor(P, Ho, Wo, sp['o_lo'] + oc + sp['o_hi'], sp['o_P'], [(sp['o_lo'], sp['o_lo'] + oc)])
        out = P.sub(self.ot, sp['o_lo'], oc)
        if three:
            l0 = self.out_tensor(P, H, W, 16, 1, [])
            P.conv(base, l0, self.w1, self.b1, relu=True, name='stem%d.level0' % self.k0)
            P.conv(l0, out, self.w2, self.b2, stride=2, relu=True, name='stem%d.level1' % self.k0)
        else:
            P.conv(base, out, self.w1, self.b1, relu=True, name='stem%d.level0' % self.k0)

    def lowered(self, L):
        Case.lowered(self, L)
        assert L['ops'] == list(range(self.k0, self.k0 + self.sp['layers'])), L['ops']

    def reference(self):
        x = h16(dev64(self.x.transpose(0, 2, 3, 1)))
        base = h16(conv_f64(x, dev64(self.w0), dev64(self.b0)).relu())
        l0 = conv_f64(base, dev64(self.w1), dev64(self.b1)).relu()
        if self.sp['layers'] == 2:
            return l0.cpu().numpy()
        return conv_f64(h16(l0), dev64(self.w2), dev64(self.b2), stride=2).relu().cpu().numpy()

    def check(self, inner):
        if self.ref is None:
            self.ref = self.reference()
        lo, oc = self.sp['o_lo'], 16 * (self.sp['layers'] - 1)
        close(inner[[id(c[0]) for c in self.checked].index(id(self.ot))][..., lo:lo + oc], self.ref,
              4e-3 if self.sp['layers'] == 3 else 3e-3, 'stem output')


class PoolS2D(Case):
    """rtm3d_op_maxpool_s2d: out = max over the four phase slices [ph * C, (ph + 1) * C) of the space-to-depth copy."""

    def build(self, P, rng):
        sp = self.sp
        B, Ho, Wo, C = sp['B'], sp['Ho'], sp['Wo'], sp['C']
        i0, o0 = sp['in_lo'], sp['o_lo']
        if sp['shared']:
            assert i0 + 4 * C <= o0 or o0 + C <= i0
            Ct = max(i0 + 4 * C, o0 + C) + sp['in_hi']
            img = image(rng, B, Ho, Wo, Ct, 1, fill=SENTINEL)
            img[:, 1:-1, 1:-1, i0:i0 + 4 * C] = f16(rng.standard_normal((B, Ho, Wo, 4 * C)))
            self.it = self.ot = self.out_tensor(P, Ho, Wo, Ct, 1, [(o0, o0 + C)], base=img)
        else:
            self.it = P.tensor(Ho, Wo, i0 + 4 * C + sp['in_hi'], 1)
            img = image(rng, B, Ho, Wo, self.it.C, 1)
            self.ot = self.out_tensor(P, Ho, Wo, o0 + C + sp['o_hi'], 1, [(o0, o0 + C)])
        self.inputs.append((self.it, img))
        self.s2d = img[:, 1:-1, 1:-1, i0:i0 + 4 * C].copy()
        self.k0 = len(P.ops)
        # a plan max-pool whose input exists only as its space-to-depth copy: the launch is re-pointed at the copy (lowered)
        P.maxpool(P.sub(self.it, i0, C), P.sub(self.ot, o0, C), 2, 2, 0, name='pool%d' % self.k0)

    def lowered(self, L):
        assert L['kind'] == 'maxpool' and L['ops'] == [self.k0], (L['kind'], L['ops'])
        L['kind'], L['in_s2d'] = 'maxpool_s2d', (self.it, self.sp['in_lo'])
        self.seen = True

    def check(self, inner):
        C, o0 = self.sp['C'], self.sp['o_lo']
        got = inner[[id(c[0]) for c in self.checked].index(id(self.ot))][..., o0:o0 + C].astype(np.float32)
        want = self.s2d.astype(np.float32).reshape(self.s2d.shape[:3] + (4, C)).max(axis=3)
        np.testing.assert_array_equal(got, want, err_msg='maxpool_s2d is not the max over the four phase slices')


KIND = {'conv64_root': Root, 'conv32s2_fused': Entry, 'stem_fused': Stem, 'maxpool_s2d': PoolS2D}


# ---------------------------------------------------------------------------------------------------------------- running
def realize(P, cases):
    """RealizedPlan of P with every case's launch carrying the decisions a plan cannot always express."""
    lower = plan_mod.lower
    by_op = {c.k0: c for c in cases}

    def hooked(plan):
        low = lower(plan)
        for L in low['launches']:
            c = by_op.get(L['ops'][0])
            if c is not None:
                c.lowered(L)
        return low
    plan_mod.lower = hooked
    try:
        R = plan_mod.RealizedPlan(P, 0)
    finally:
        plan_mod.lower = lower
    assert all(c.seen for c in cases), [c.sp['kind'] for c in cases if not c.seen]
    return R


def _forward(R, cases, xin):
    for c in cases:
        for s, img in c.poisoned():
            raw_write(R, s, img)
    outs = [torch.zeros(16, device='cuda') for _ in range(4)]
    R.forward(torch.cuda.current_stream().cuda_stream, xin.data_ptr(), [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    return [[raw_read(R, s) for s, *_ in c.checked] for c in cases]


def run_plan(P, cases, replays=0, graph=False):
    """Record P, assert every op's name, upload the operands, run one poisoned forward and check every output; then `replays`
    eager replays and (graph) one hipGraph replay, each re-poisoned, all bit-identical to the first."""
    R = realize(P, cases)
    try:
        names = [n for n in R.kernel_names() if n != 'nchw_f32_to_nhwc4_f16']
        assert names == [op_name(c.sp) for c in cases], names
        for c in cases:
            for s, img in c.inputs:
                raw_write(R, s, img)
        stems = [c for c in cases if c.sp['kind'] == 'stem_fused']
        assert len(stems) <= 1, 'one image batch per plan'
        xin = torch.from_numpy(stems[0].x).cuda() if stems else torch.zeros(16, device='cuda')
        first = _forward(R, cases, xin)
        for c, raws in zip(cases, first):
            c.check(c.verify(raws))
        later = [_forward(R, cases, xin) for _ in range(replays)]
        if graph:
            R.set_graph(True)
            later.append(_forward(R, cases, xin))
            captures, _, enabled = R.graph_stats()
            assert captures == 1 and enabled, R.graph_stats()
        for outs in later:
            for a, b in zip(first, outs):
                for x, y in zip(a, b):
                    np.testing.assert_array_equal(x.view(np.uint16), y.view(np.uint16))
    finally:
        R.close()


def run_one(sp, seed):
    check_regime(sp)
    H, W = (sp['H'], sp['W']) if 'H' in sp else (sp['Ho'] * 2, sp['Wo'] * 2)
    P = plan_mod.Plan(sp['B'], H, W)
    run_plan(P, [KIND[sp['kind']](P, sp, np.random.default_rng(seed))])


I110, I010, I111, I101, I011, I001 = fr.ROOT_INSTANCES

CASES = {
    # ---- conv64_root: the six instances, each `single` (total <= 256) and with tickets (total 257 / 258 / 259 / >= 768)
    'root101_total1': root(1, 8, 32, out_lo=8, out_hi=8, p_lo=8, p_hi=8, expect=dict(instance=I101, total=1, single=True)),
    'root101_b1_product': root(1, 96, 320, out_hi=256, p_lo=256, p_hi=256, expect=dict(instance=I101, total=120, single=True)),
    'root101_total768': root(4, 96, 512, out_lo=16, p_lo=8, expect=dict(instance=I101, total=768, first_draw_busy=256, mod3=0)),
    'root101_conv_relu0_single': root(2, 16, 64, conv_relu=False, out_lo=8, p_hi=8, expect=dict(instance=I101, total=8, single=True)),
    'root101_relu0_tickets': root(1, 8, 8224, conv_relu=False, root_relu=False, out_hi=8, p_lo=64,
                                  expect=dict(instance=I101, total=257, mod3=2)),
    'root110_b2_product': root(2, 96, 320, s2d=True, norm=False, s_lo=256, p_lo=256, p_hi=256,
                               expect=dict(instance=I110, total=240, single=True)),
    'root110_b8_416_tickets': root(8, 104, 320, s2d=True, norm=False, s_lo=256, p_lo=256, p_hi=256,
                                   expect=dict(instance=I110, total=1040, single=False, mod3=2, first_draw_busy=256)),
    'root110_total257_root_relu0': root(1, 8, 8224, s2d=True, norm=False, root_relu=False, shared='s2d_first', s_lo=8, s_hi=8,
                                        expect=dict(instance=I110, total=257, mod3=2, first_draw_busy=86)),
    'root110_total258_conv_relu0': root(2, 8, 4128, s2d=True, norm=False, conv_relu=False, s_hi=64, p_lo=64,
                                        expect=dict(instance=I110, total=258, mod3=0)),
    'root010_total1': root(1, 8, 32, pool=False, s2d=True, norm=False, s_lo=64, expect=dict(instance=I010, total=1, single=True)),
    'root010_total258': root(2, 8, 4128, pool=False, s2d=True, norm=False, in_lo=64, s_hi=8, expect=dict(instance=I010, total=258, mod3=0)),
    'root111_total256_shared': root(4, 64, 256, s2d=True, shared='pool_first', s_lo=8, s_hi=8, out_lo=64,
                                    expect=dict(instance=I111, total=256, single=True)),
    'root111_total259': root(7, 296, 32, s2d=True, in_lo=8, in_hi=8, s_lo=64, p_hi=8, expect=dict(instance=I111, total=259, mod3=1)),
    'root011_single': root(1, 16, 64, pool=False, s2d=True, out_hi=64, s_lo=8, s_hi=8, expect=dict(instance=I011, total=4, single=True)),
    'root011_total257': root(1, 8, 8224, pool=False, s2d=True, out_lo=8, s_lo=8, expect=dict(instance=I011, total=257, mod3=2)),
    'root001_total256': root(4, 64, 256, pool=False, out_lo=8, out_hi=8, expect=dict(instance=I001, total=256, single=True)),
    'root001_total259': root(7, 296, 32, pool=False, root_relu=False, out_hi=64, expect=dict(instance=I001, total=259, mod3=1)),
    # ---- conv32s2_fused: the same ticket boundaries; both output slices at non-zero offsets
    'entry_total1': entry(1, 8, 32, in_lo=8, c_lo=8, c_hi=8, p_lo=64, expect=dict(total=1, single=True)),
    'entry_b1_product': entry(1, 96, 320, c_lo=64, p_lo=64, expect=dict(total=120, single=True)),
    'entry_total256': entry(4, 64, 256, in_hi=8, c_lo=16, p_lo=8, p_hi=8, p_P=1, expect=dict(total=256, single=True)),
    'entry_total257': entry(1, 8, 8224, c_lo=8, p_lo=8, expect=dict(total=257, mod3=2, first_draw_busy=86)),
    'entry_total258_shared': entry(2, 8, 4128, in_lo=32, shared=True, c_lo=8, c_hi=8, expect=dict(total=258, mod3=0)),
    'entry_total259': entry(7, 296, 32, c_lo=64, c_P=0, p_lo=8, p_hi=64, expect=dict(total=259, mod3=1)),
    'entry_b2_416_product': entry(2, 104, 320, c_lo=64, p_lo=64, expect=dict(total=260, mod3=2)),
    'entry_total768': entry(4, 96, 512, c_lo=8, p_lo=8, expect=dict(total=768, first_draw_busy=256, mod3=0)),
    # ---- conv_stem_fused: both forms, output slices with spare channels on both sides, one full 384 x 1280 image
    'stem2_small': stem(2, 32, 64, 2, o_lo=8, o_hi=8, expect=dict(grid=8)),
    'stem2_b3': stem(3, 48, 96, 2, o_lo=16, o_P=0, expect=dict(grid=27)),
    'stem3_small': stem(2, 32, 64, 3, o_lo=8, o_hi=8, expect=dict(grid=8)),
    'stem3_b3': stem(3, 48, 96, 3, o_hi=8, o_P=0, expect=dict(grid=27)),
    'stem3_full_image': stem(1, 384, 1280, 3, o_lo=8, o_hi=16, expect=dict(grid=960)),
    # ---- maxpool_s2d: 8 / 128 / 256 channels, the product's channel offsets, idle lanes in the last block, one tensor
    'pool_c8_idle': pool_s2d(1, 5, 7, 8, in_lo=8, in_hi=8, o_lo=8, o_hi=8, expect=dict(threads=35, idle=221)),
    'pool_c128_product': pool_s2d(2, 24, 80, 128, in_lo=256, o_lo=512, o_hi=512, expect=dict(threads=61440, idle=0)),
    'pool_c128_idle': pool_s2d(1, 13, 39, 128, in_lo=256, o_lo=512, o_hi=512, expect=dict(threads=8112, idle=80)),
    'pool_c256_product': pool_s2d(2, 12, 40, 256, in_lo=256, o_lo=1024, o_hi=512, expect=dict(threads=30720, idle=0)),
    'pool_c256_shared_idle': pool_s2d(1, 13, 41, 256, in_lo=0, o_lo=1024, in_hi=8, shared=True, expect=dict(threads=17056, idle=96)),
    'pool_c8_shared_out_below': pool_s2d(2, 3, 5, 8, in_lo=16, o_lo=0, in_hi=8, shared=True, expect=dict(threads=30, idle=226)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_fused_route_and_regime(name):
    run_one(CASES[name], seed=sum(map(ord, name)))


# ---- ticket and single launches of the level tail (<1,1,0> and <1,0,1>) and of the level entry in ONE plan: each ticket op
# draws from its own counter, zeroed at the head of every forward; every ordered pair of regimes runs back to back
CHAIN = {
    'root110_tickets': root(1, 8, 8224, s2d=True, norm=False, s_lo=8, p_lo=8, expect=dict(instance=I110, total=257, single=False)),
    'root101_single': root(1, 16, 64, out_lo=8, p_hi=8, expect=dict(instance=I101, total=4, single=True)),
    'entry_tickets': entry(1, 8, 8224, c_lo=8, p_lo=8, expect=dict(total=257, single=False)),
    'entry_single': entry(1, 8, 64, c_hi=8, p_lo=8, expect=dict(total=2, single=True)),
}


def test_fused_counter_chain():
    keys = list(CHAIN)
    order = every_pair_order(len(keys))
    assert len({(a, b) for a, b in zip(order, order[1:])}) == len(keys) * (len(keys) - 1)
    for sp in CHAIN.values():
        check_regime(sp)
    P = plan_mod.Plan(1, 16 * 4, 16448 * 4)
    rng = np.random.default_rng(7)
    cases = [KIND[CHAIN[keys[i]]['kind']](P, CHAIN[keys[i]], rng) for i in order]
    run_plan(P, cases, replays=3, graph=True)


# ---------------------------------------------------------------------------------------------------------------- admission
class _Ctx(object):
    def __init__(self):
        self.lib = _lib.load()
        self.ctx = ctypes.c_void_p()
        _lib.check(self.lib.rtm3d_ctx_create(0, ctypes.byref(self.ctx)))

    def tensor(self, B, H, W, C, pad):
        tid = ctypes.c_int()
        _lib.check(self.lib.rtm3d_tensor_create(self.ctx, B, H, W, C, pad, ctypes.byref(tid)))
        return tid.value

    def blob(self, nbytes):
        arr = np.zeros(nbytes, np.uint8)
        bid = ctypes.c_int()
        _lib.check(self.lib.rtm3d_blob_create(self.ctx, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, ctypes.byref(bid)))
        return bid.value

    def n_ops(self):
        n = 0
        while self.lib.rtm3d_op_info(self.ctx, n, None, None, None) == 0:
            n += 1
        return n

    def last_name(self):
        got = ctypes.c_char_p()
        _lib.check(self.lib.rtm3d_op_info(self.ctx, self.n_ops() - 1, None, None, ctypes.byref(got)))
        return got.value

    def close(self):
        self.lib.rtm3d_ctx_destroy(self.ctx)


def _refusals(c, fn, what, base, bad):
    """fn(*args) for each (changes {arg index: value}, message) of `bad`: refused, reported under the op's name, nothing
    recorded.  Returns the recorded count afterwards."""
    for changes, msg in bad:
        args = list(base)
        for i, v in changes.items():
            args[i] = v
        n = c.n_ops()
        assert fn(*args) != 0, (changes, msg)
        err = c.lib.rtm3d_last_error()
        assert err.startswith(what + b':') and msg in err, (changes, msg, err)
        assert c.n_ops() == n, (changes, msg)


def test_level_tail_refusals_are_named_and_record_nothing():
    c = _Ctx()
    try:
        t_in = c.tensor(1, 16, 64, 128, 1)
        t_cat, t_out = c.tensor(1, 16, 64, 128, 1), c.tensor(1, 16, 64, 64, 1)
        t_ps, t_s2d = c.tensor(1, 8, 32, 320, 1), c.tensor(1, 8, 32, 512, 1)
        t_h20, t_nopad, t_narrow = c.tensor(1, 20, 64, 64, 1), c.tensor(1, 16, 64, 64, 0), c.tensor(1, 16, 32, 128, 1)
        wc, bc, wr, br = c.blob(9 * 64 * 64 * 2), c.blob(64 * 4), c.blob(64 * 128 * 2), c.blob(64 * 4)
        fn = lambda *a: c.lib.rtm3d_op_conv64_root(c.ctx, *a)
        # in, in_coff, res, res_coff, conv_relu, w_conv, b_conv, w_root, b_root, out, out_coff, root_relu, pool, pool_coff, s2d, s2d_coff
        base = [t_in, 0, t_cat, 64, 1, wc, bc, wr, br, t_out, 0, 1, t_ps, 0, t_ps, 64]
        _refusals(c, fn, b'op_conv64_root', base, [
            ({0: 999}, b'bad tensors'), ({2: -1}, b'bad tensors'), ({12: 999}, b'bad tensors'), ({14: 999}, b'bad tensors'),
            ({9: -1, 14: -1}, b'needs a space-to-depth copy'),
            ({14: t_out}, b'space-to-depth output slice mismatch'), ({15: 72}, b'space-to-depth output slice mismatch'),
            ({15: 68}, b'space-to-depth output slice mismatch'),
            ({9: t_s2d, 14: t_s2d, 15: 0}, b'aliases an operand'),
            ({1: 72}, b'input slice mismatch'), ({1: 4}, b'input slice mismatch'), ({0: t_nopad}, b'input slice mismatch'),
            ({0: t_h20, 14: -1}, b'needs H % 8 == 0'),          # (a copy would fail its shape check first)
            ({2: t_narrow}, b'residual / output shape mismatch'), ({9: t_narrow}, b'residual / output shape mismatch'),
            ({3: 72}, b'residual / output slice mismatch'), ({10: 8}, b'residual / output slice mismatch'),
            ({9: t_cat, 10: 64}, b'overlaps x1'), ({9: t_cat, 10: 32}, b'overlaps x1'),
            ({9: t_in, 10: 32}, b'overlaps the conv input'), ({9: t_in, 10: 0}, b'overlaps the conv input'),
            ({12: t_out}, b'pooled output slice mismatch'), ({13: 264}, b'pooled output slice mismatch'),
            ({13: 256}, b'overlaps the space-to-depth slice'), ({13: 8}, b'overlaps the space-to-depth slice'),
            ({15: 0, 13: 248}, b'overlaps the space-to-depth slice'),
            ({5: bc}, b'blob size mismatch'), ({6: wc}, b'blob size mismatch'), ({7: wc}, b'blob size mismatch'), ({8: wr}, b'blob size mismatch'),
        ])
        # accepted: the pooled slice right below / right above the copy in one tensor, the output beside the input slice
        for changes, name in (({}, b'conv3x3_c64+root1x1+pool_fused+s2d'), ({13: 256, 15: 0}, b'conv3x3_c64+root1x1+pool_fused+s2d'),
                              ({9: t_in, 10: 64, 14: -1}, b'conv3x3_c64+root1x1+pool_fused'),
                              ({9: -1, 12: -1}, b'conv3x3_c64+root1x1_fused+s2d')):
            args = list(base)
            for i, v in changes.items():
                args[i] = v
            n = c.n_ops()
            assert fn(*args) == 0, (changes, c.lib.rtm3d_last_error())
            assert c.n_ops() == n + 1 and c.last_name() == name, (changes, c.last_name())
    finally:
        c.close()


def test_level_entry_refusals_are_named_and_record_nothing():
    c = _Ctx()
    try:
        t_x, t_oc, t_op = c.tensor(1, 16, 64, 40, 1), c.tensor(1, 8, 32, 128, 1), c.tensor(1, 8, 32, 64, 0)
        t_nopad, t_h24, t_w96, t_full = c.tensor(1, 16, 64, 32, 0), c.tensor(1, 24, 64, 32, 1), c.tensor(1, 16, 96, 32, 1), c.tensor(1, 16, 64, 64, 1)
        wc, bc, wp, bp = c.blob(9 * 4 * 64 * 8 * 2), c.blob(64 * 4), c.blob(4 * 64 * 8 * 2), c.blob(64 * 4)
        fn = lambda *a: c.lib.rtm3d_op_conv32s2_fused(c.ctx, *a)
        # in, in_coff, conv, conv_coff, proj, proj_coff, w_conv, b_conv, w_proj, b_proj
        base = [t_x, 8, t_oc, 0, t_op, 0, wc, bc, wp, bp]
        _refusals(c, fn, b'op_conv32s2_fused', base, [
            ({0: 999}, b'bad tensors'), ({2: 999}, b'bad tensors'), ({4: -1}, b'bad tensors'),
            ({1: 16}, b'input slice mismatch'), ({1: 4}, b'input slice mismatch'), ({0: t_nopad, 1: 0}, b'input slice mismatch'),
            ({0: t_h24, 1: 0}, b'needs H % 16 == 0 and W % 64 == 0'), ({0: t_w96, 1: 0}, b'needs H % 16 == 0 and W % 64 == 0'),
            ({2: t_full}, b'half the input resolution'), ({4: t_full}, b'half the input resolution'),
            ({3: 72}, b'output slice mismatch'), ({3: 4}, b'output slice mismatch'), ({5: 8}, b'output slice mismatch'),
            ({4: t_oc, 5: 0}, b'overlaps the project slice'), ({4: t_oc, 3: 64, 5: 8}, b'overlaps the project slice'),
            ({4: t_oc, 3: 8, 5: 64}, b'overlaps the project slice'), ({4: t_oc, 3: 56, 5: 0}, b'overlaps the project slice'),
            ({6: wp}, b'blob size mismatch'), ({7: wc}, b'blob size mismatch'), ({8: wc}, b'blob size mismatch'), ({9: wp}, b'blob size mismatch'),
        ])
        for changes in ({}, {4: t_oc, 3: 0, 5: 64}, {4: t_oc, 3: 64, 5: 0}):      # adjacent slices of one tensor are accepted
            args = list(base)
            for i, v in changes.items():
                args[i] = v
            n = c.n_ops()
            assert fn(*args) == 0, (changes, c.lib.rtm3d_last_error())
            assert c.n_ops() == n + 1 and c.last_name() == b'pool+proj1x1+conv3x3s2_fused'
    finally:
        c.close()
