"""CPU yardsticks of the neck FPN backward (include/rtm3d_hip.h, "neck FPN backward"), at any channel count.

R64: torch's fp64 CPU autograd.  Two forms of it:
     ``autograd_uncomposed`` over the function as models/nets/keypoint_fpn_fusion.py:35-46 writes it (head, up, cat, proj per
     level, every conv with its own weight and bias) - what tests/golden/neck_fpn_grad_cases.npz holds; and
     ``chain(case, False)`` over the function as the plan computes it (proj followed by head composed into one 1x1 conv A = Wh Wp,
     b = Wh bp + bh) on the saved activations a forward left, plus ``factor_rule``, which gives the reference's own parameters from
     the composed gradients.  There is no non-linearity between proj and head, so the two agree to rounding.
Q16: the rule restated - the same chain with the fp16 roundings at the stated points (every D_k, E_k, g_k, d feat3) and fp64 sums
     - plus, per tensor, the any-order fp32 summation bound n * 2^-24 * max sum |term| of its last reduction ("floor").

A case (tests/fpn_backward_cases.py) holds NHWC arrays; everything here is NCHW fp64.  C: the FPN's width (256 on the device).
    B, H, W (the MAP of z0), C, S, T, U, want_slices
    dz            (B, H, W, C): the gradient of z0 as it ARRIVES, times S
    ncat[k]       (B, H >> k, W >> k, C + f_k), k = 0, 1, 2: the saved concat tensor [up | feat_k]
    h[k]          (B, H >> (k + 1), W >> (k + 1), C): kfpn_h{k + 3} as the forward saved it
    feat3         (B, H >> 3, W >> 3, f_3)
    F[k]          (B, H >> (k + 1), W >> (k + 1), C): the fusion-path term of d kfpn_h{k + 3} as it ARRIVES, times S T
    A[k]          (C, C + f_k) for k = 0, 1, 2 and (C, f_3) for k = 3 (kfpn_head5): the 1x1 weights as the forward used them
    wup[k]        (C, C, 4, 4): kfpn_up{k + 3}'s weight as the forward used it
"""
import numpy as np
import torch
import torch.nn.functional as F_

from tests import neck_backward_ref as nref

_nchw, _r16, deconv = nref._nchw, nref._r16, nref.deconv
LEVELS = 3


# ------------------------------------------------------------------------------------------------- the function, un-composed
def param_names(levels=(2, 3, 4, 5)):
    """The reference's parameter keys (without the 'kfpn_fusion.' prefix), in the order the fixture stores them."""
    out = []
    for L in levels[::-1]:
        out += ['kfpn_head%d.weight' % L, 'kfpn_head%d.bias' % L]
        if L > levels[0]:
            out += ['kfpn_up%d.conv_tran.weight' % L, 'kfpn_proj%d.weight' % L, 'kfpn_proj%d.bias' % L]
    return out


def fpn_uncomposed(feats, p):
    """keypoint_fpn_fusion.py:35-46 on NCHW tensors feats[0 .. 3] and a dict of parameters -> [z0, h3, h4, h5]."""
    x = list(feats)
    n = len(x)
    for i in range(n - 1, 0, -1):
        L = i + 2
        x[i] = F_.conv2d(x[i], p['kfpn_head%d.weight' % L], p['kfpn_head%d.bias' % L])
        up = deconv(x[i], p['kfpn_up%d.conv_tran.weight' % L])
        x[i - 1] = F_.conv2d(torch.cat([up, x[i - 1]], 1), p['kfpn_proj%d.weight' % L], p['kfpn_proj%d.bias' % L])
    x[0] = F_.conv2d(x[0], p['kfpn_head2.weight'], p['kfpn_head2.bias'])
    return x


def autograd_uncomposed(feats, params, G):
    """fp64 autograd of (sum_i out_i * G_i).sum() w.r.t. the features and every parameter -> ({'feat<i>': ...}, {name: ...})."""
    feats = [torch.as_tensor(np.asarray(f, np.float64)).clone().requires_grad_(True) for f in feats]
    p = {k: torch.as_tensor(np.asarray(v, np.float64)).clone().requires_grad_(True) for k, v in params.items()}
    out = fpn_uncomposed(feats, p)
    loss = sum((o * torch.as_tensor(np.asarray(g, np.float64))).sum() for o, g in zip(out, G))
    names = sorted(p)
    gr = torch.autograd.grad(loss, feats + [p[k] for k in names])
    return ({'feat%d' % i: gr[i].numpy() for i in range(len(feats))}, {k: gr[len(feats) + i].numpy() for i, k in enumerate(names)},
            [o.detach() for o in out])


def compose(params, L):
    """A = Wh Wp, b = Wh bp + bh of proj_L followed by head_{L-1}, in fp64 (plan.py, _compose)."""
    wh = np.asarray(params['kfpn_head%d.weight' % (L - 1)], np.float64)[:, :, 0, 0]
    wp = np.asarray(params['kfpn_proj%d.weight' % L], np.float64)[:, :, 0, 0]
    b = wh @ np.asarray(params['kfpn_proj%d.bias' % L], np.float64) + np.asarray(params['kfpn_head%d.bias' % (L - 1)], np.float64)
    return wh @ wp, b


def factor_rule(dA, db, wh, wp, bp):
    """The reference's own gradients from the composed conv's: (dWh, dWp, dbh, dbp), 2-D weights, fp64.  head's input is
    x = Wp ncat + bp, so dWh = sum_p g x^T = dA Wp^T + db bp^T: the bias of proj reaches head's weight."""
    dA, db, wh, wp, bp = (np.asarray(a, np.float64) for a in (dA, db, wh, wp, bp))
    return dA @ wp.T + np.outer(db, bp), wh.T @ dA, db, wh.T @ db


def forward_composed(feats, params):
    """The forward as the plan runs it, fp64 and unrounded: -> (ncat[0 .. 2], h[0 .. 2], z0), NCHW tensors."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    conv = lambda x, A, b: F_.conv2d(x, t(A)[:, :, None, None], t(b))
    hk = conv(t(feats[3]), np.asarray(params['kfpn_head5.weight'])[:, :, 0, 0], params['kfpn_head5.bias'])
    ncat, h = [None] * 3, [None] * 3
    for k in (2, 1, 0):
        h[k] = hk
        ncat[k] = torch.cat([deconv(hk, t(params['kfpn_up%d.conv_tran.weight' % (k + 3)])), t(feats[k])], 1)
        hk = conv(ncat[k], *compose(params, k + 3))
    return ncat, h, hk


# ------------------------------------------------------------------------------------------------- the chain, composed
def _deconv_grads(x, w, dy):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    return torch.autograd.grad(deconv(x, w), [x, w], dy)


def chain(case, rounded):
    """The backward chain of a case.  rounded=False: R64 (no scale plays a part: every result is unscaled); True: Q16, the
    activation gradients in the S U domain as the device stores them.  -> dict: 'D' [k] (k = 0 .. 2: Cin channels), 'E' [k], 'g' [k]
    (k = 1 .. 3 at index k - 1), 'dfeat3', 'dA' [k], 'db' [k] (k = 0 .. 3), 'dwup' [k]; the parameter gradients unscaled always.
    With rounded=True also 'floor:<name>'."""
    S, T, U = (float(case[k]) for k in 'STU')
    rnd = _r16 if rounded else (lambda t: t)
    u24 = 2.0 ** -24
    C = int(case['C'])
    g = _nchw(case['dz']) if rounded else _nchw(case['dz']) / S
    fac = S if rounded else 1.0                                               # the factor g carries
    out = {k: [] for k in ('D', 'E', 'g', 'dA', 'db', 'dwup', 'floor:D', 'floor:E', 'floor:g', 'floor:dA', 'floor:db', 'floor:dwup')}

    def conv1x1(x, A, g, mul):
        dA = torch.einsum('bohw,bihw->oi', g, x) / fac
        db = g.sum((0, 2, 3)) / fac
        D = rnd(mul * torch.einsum('bohw,oi->bihw', g, A))
        npix = x.shape[0] * x.shape[2] * x.shape[3]
        fl = (float(npix * u24 * torch.einsum('bohw,bihw->oi', g.abs(), x.abs()).max() / fac), float(npix * u24 * g.abs().sum((0, 2, 3)).max() / fac),
              float(g.shape[1] * u24 * mul * torch.einsum('bohw,oi->bihw', g.abs(), A.abs()).max()))
        return dA, db, D, fl

    for k in range(LEVELS):
        x, A = _nchw(case['ncat'][k]), torch.as_tensor(np.asarray(case['A'][k], np.float64))
        mul = U if (rounded and k == 0) else 1.0
        dA, db, D, fl = conv1x1(x, A, g, mul)
        fac = S * U if rounded else 1.0
        h, w = _nchw(case['h'][k]), torch.as_tensor(np.asarray(case['wup'][k], np.float64))
        dy = D[:, :C].contiguous()
        E, dw = _deconv_grads(h, w, dy)
        ae, aw = _deconv_grads(h.abs(), w.abs(), dy.abs())
        E = rnd(E)
        Fk = _nchw(case['F'][k]) * (U / T if rounded else 1.0 / (S * T))
        g = rnd(E + Fk)
        npix = h.shape[0] * h.shape[2] * h.shape[3]
        fE = float(16 * C * u24 * ae.max())
        for name, v in (('D', D), ('E', E), ('g', g), ('dA', dA), ('db', db), ('dwup', dw / fac),
                        ('floor:dA', fl[0]), ('floor:db', fl[1]), ('floor:D', fl[2]), ('floor:E', fE), ('floor:g', fE),
                        ('floor:dwup', float(npix * u24 * aw.max() / fac))):
            out[name].append(v)
    dA, db, D, fl = conv1x1(_nchw(case['feat3']), torch.as_tensor(np.asarray(case['A'][3], np.float64)), g, 1.0)
    out['dA'].append(dA); out['db'].append(db); out['dfeat3'] = D
    out['floor:dA'].append(fl[0]); out['floor:db'].append(fl[1]); out['floor:dfeat3'] = fl[2]
    return out


def flat(res, scale=1.0):
    """{tensor name: fp64 numpy array} of a chain() result.  The activation gradients of an R64 result are multiplied by ``scale``
    (S U) so that they compare with the device's scaled fp16 maps."""
    out = {'dfeat3': res['dfeat3'].numpy() * scale}
    for key in ('D', 'E', 'g'):
        for k, t in enumerate(res[key]):
            out['%s[%d]' % (key, k)] = t.numpy() * scale
    for key in ('dA', 'db', 'dwup'):
        for k, t in enumerate(res[key]):
            out['%s[%d]' % (key, k)] = t.numpy()
    return out


def floors(res):
    out = {'dfeat3': res['floor:dfeat3']}
    for key in ('D', 'E', 'g', 'dA', 'db', 'dwup'):
        for k, v in enumerate(res['floor:' + key]):
            out['%s[%d]' % (key, k)] = v
    return out


# ------------------------------------------------------------------------------------------------- one 1x1 conv, written out
def layer_exact(x, A, dy, inv, mul):
    """One 1x1 conv on integer-valued NHWC x (Cin), (256, Cin) A and NHWC dy (256): (dX NHWC, dA, db) in fp64, the sums written out as
    the rule has them (no autograd)."""
    x, A, dy = (np.asarray(a, np.float64) for a in (x, A, dy))
    return mul * np.einsum('byxo,oi->byxi', dy, A), inv * np.einsum('byxo,byxi->oi', dy, x), inv * dy.sum((0, 1, 2))


def add_exact(e, f, r):
    """g = fp16(fp32(E) + fp32(F) r) with numpy's fp32 and fp16 roundings (IEEE, round to nearest even: the device's)."""
    with np.errstate(invalid='ignore', over='ignore'):                        # (the special values are the point)
        return (np.asarray(e, np.float16).astype(np.float32) + np.asarray(f, np.float16).astype(np.float32) * np.float32(r)).astype(np.float16)
