"""CPU yardsticks of the head backward (include/rtm3d_hip.h, "head backward").

R64: torch's fp64 CPU autograd over torch.nn.functional.conv2d, structured as models/nets/header.py (conv + frozen BN folded
     into Wf + ReLU per layer, a final conv with bias), evaluated on the fp16 weights and the saved fp16 activations a forward
     left: the exact gradient of the function that forward computed.
Q16: the rule restated - the same chain with the fp16 roundings at the stated points (go, every dh, dz) and fp64 sums - plus, per
     tensor, the any-order fp32 summation bound gamma_n * sum |term| of its last reduction ("floor").

A case (tests/head_backward_cases.py) holds NHWC activations and torch-order weights; everything here is NCHW fp64 inside.
"""
import numpy as np
import torch
import torch.nn.functional as F


def _nchw(a):
    return torch.as_tensor(np.asarray(a, np.float64)).permute(0, 3, 1, 2).contiguous()


def _layer_grads(x, w, dy, dil, need_dx=True):
    """fp64 autograd of y = conv2d(x, w, dilation=dil, padding=dil) for the upstream dy: (dx or None, dw, db)."""
    x = x.clone().requires_grad_(need_dx)
    w = w.clone().requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, dilation=dil, padding=dil)
    got = torch.autograd.grad(y, ([x] if need_dx else []) + [w, b], dy)
    return (got[0] if need_dx else None,) + tuple(got[-2:])


def _r16(t):
    return t.to(torch.float16).to(torch.float64)


def chain(case, rounded):
    """The backward chain of a case.  rounded=False: R64 (S plays no part); True: Q16.  -> dict of fp64 tensors:
    'go' (B, G*16 .. as NCHW per head list), 'dh%d' (NCHW, G*256 channels, in the scaled domain for Q16), 'dz', and the parameter
    gradients 'dw%d' / 'db%d' (lists over g, k = 1 .. num_conv), 'dwo' / 'dbo'; with rounded=True also 'floor:<name>'."""
    G, n, S = len(case['K']), case['num_conv'], float(case['S']) if rounded else 1.0
    rnd = _r16 if rounded else (lambda t: t)
    u = 2.0 ** -24
    out = {}
    acts = [_nchw(a) for a in case['acts']]
    go = [rnd(S * torch.as_tensor(d, dtype=torch.float64)) for d in case['dlogits']]
    out['go'] = go
    hl = acts[n]
    dh = []
    out['dwo'], out['dbo'], out['floor:dwo'], out['floor:dbo'] = [], [], [], []
    npix = hl.shape[0] * hl.shape[2] * hl.shape[3]
    for g in range(G):
        x = hl[:, g * 256:(g + 1) * 256]
        wo = torch.as_tensor(np.asarray(case['wo'][g], np.float64))
        dx, dw, db = _layer_grads(x, wo, go[g], 1)
        out['dwo'].append(dw / S); out['dbo'].append(db / S)
        if rounded:
            _, aw, ab = _layer_grads(x.abs(), wo.abs(), go[g].abs(), 1, need_dx=False)
            out['floor:dwo'].append(float(npix * u * aw.max() / S)); out['floor:dbo'].append(float(npix * u * ab.max() / S))
        dh.append(rnd(dx * (x > 0)))
    dy = torch.cat(dh, 1)
    out['dh%d' % n] = dy
    for k in range(n, 0, -1):
        dil = 6 if k == 1 else 1
        xin = acts[k - 1]
        out['dw%d' % k], out['db%d' % k], out['floor:dw%d' % k], out['floor:db%d' % k] = [], [], [], []
        dxs = []
        for g in range(G):
            x = xin if k == 1 else xin[:, g * 256:(g + 1) * 256]
            wf = torch.as_tensor(np.asarray(case['wf'][k][g], np.float64))
            s = torch.as_tensor(np.asarray(case['scale'][k][g], np.float64))
            need_dx = k > 1 or case['input_grad']
            dx, dw, db = _layer_grads(x, wf, dy[:, g * 256:(g + 1) * 256], dil, need_dx)
            out['dw%d' % k].append(dw / S * s[:, None, None, None]); out['db%d' % k].append(db / S * s)
            if rounded:
                _, aw, ab = _layer_grads(x.abs(), wf.abs(), dy[:, g * 256:(g + 1) * 256].abs(), dil, need_dx=False)
                out['floor:dw%d' % k].append(float(npix * u * (aw * s.abs()[:, None, None, None]).max() / S))
                out['floor:db%d' % k].append(float(npix * u * (ab * s.abs()).max() / S))
            dxs.append(dx)
        if k > 1:
            dy = torch.cat([rnd(dx * (xin[:, g * 256:(g + 1) * 256] > 0)) for g, dx in enumerate(dxs)], 1)
            out['dh%d' % (k - 1)] = dy
        elif case['input_grad']:
            out['dz'] = rnd(sum(dxs))
    return out


def flat(res, scaled_S=1.0):
    """{tensor name: fp64 numpy array} of a chain() result; lists become 'name[g]'.  Activation gradients of an R64 result are
    multiplied by scaled_S so that they compare with the device's scaled fp16 maps."""
    out = {}
    for k, v in res.items():
        if k.startswith('floor:'):
            continue
        act = k == 'go' or k.startswith('dh') or k == 'dz'
        for i, t in enumerate(v if isinstance(v, list) else [v]):
            name = '%s[%d]' % (k, i) if isinstance(v, list) else k
            out[name] = t.numpy() * (scaled_S if act else 1.0)
    return out


def unfolded_param_grads(x, w, b, gamma, beta, mean, var, eps, dy, dil):
    """fp64 torch autograd through the UNFOLDED layer conv2d(x, w, b) -> eval-mode batch_norm: (dw, db)."""
    x, dy = torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(dy, dtype=torch.float64)
    w = torch.as_tensor(w, dtype=torch.float64).requires_grad_(True)
    b = torch.as_tensor(b, dtype=torch.float64).requires_grad_(True)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    y = F.batch_norm(F.conv2d(x, w, b, dilation=dil, padding=dil), t(mean), t(var), t(gamma), t(beta), False, 0.0, eps)
    return torch.autograd.grad(y, [w, b], dy)
