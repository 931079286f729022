"""CPU yardsticks of the neck fusion backward (include/rtm3d_hip.h, "neck fusion backward"), at any channel count.

R64: torch's fp64 CPU autograd over torch.nn.functional.conv_transpose2d(stride 2, padding 1) and the detached softmax product
     u * softmax(u.detach()), structured as models/nets/keypoint_fpn_fusion.py:62-69 and evaluated on the fp16-valued weights and
     the saved activations a forward left: the exact gradient of the function that forward computed.
Q16: the rule restated - the same chain with the fp16 roundings at the stated points (every du, every dX) and fp64 sums - plus,
     per tensor, the any-order fp32 summation bound n * 2^-24 * max sum |term| of its last reduction ("floor").

A case (tests/neck_backward_cases.py) holds NHWC arrays and torch-order (ci, co, 4, 4) weights; everything here is NCHW fp64.
    B, H, W (the MAP of z), levels, C, S, T, want_slices
    dz            (B, H, W, C): the gradient of z as it ARRIVES, times S
    us[l]         (B, H, W, C): u_l as the forward saved it
    xs[l][j]      the saved input of deconv j of operand l, (B, H >> (l + 1 - j), W >> (l + 1 - j), C); xs[l][0]: kfpn_h
    w[l][j]       (C, C, 4, 4) the weight as the forward used it
"""
import numpy as np
import torch
import torch.nn.functional as F


def _nchw(a):
    return torch.as_tensor(np.asarray(a, np.float64)).permute(0, 3, 1, 2).contiguous()


def _r16(t):
    return t.to(torch.float16).to(torch.float64)


def deconv(x, w):
    return F.conv_transpose2d(x, w, stride=2, padding=1)


def forward(h, w, round16):
    """The fusion's forward from the leaves h[l] (NCHW tensors, operand l's kfpn_h) and weights w[l][j] -> (xs, us): the saved
    input of every deconv and every u.  round16: each map is rounded to fp16 as a device forward stores it."""
    rnd = _r16 if round16 else (lambda t: t)
    xs, us = [], []
    for l, x in enumerate(h):
        chain = []
        for j in range(l + 1):
            chain.append(x)
            x = rnd(deconv(x, w[l][j]))
        xs.append(chain)
        us.append(x)
    return xs, us


def softmax_grad(u, g):
    """fp64 autograd of sum(g * u * softmax_{HW}(u.detach())) w.r.t. u."""
    u = u.clone().requires_grad_(True)
    b, c, h, w = u.shape
    zi = u * torch.softmax(u.detach().view(b, c, -1), dim=-1).view(b, c, h, w)
    return torch.autograd.grad(zi, [u], g)[0]


def _layer_grads(x, w, dy):
    """fp64 autograd of y = conv_transpose2d(x, w, stride 2, padding 1) for the upstream dy: (dx, dw)."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    return torch.autograd.grad(deconv(x, w), [x, w], dy)


def chain(case, rounded):
    """The backward chain of a case.  rounded=False: R64 (neither scale plays a part: every result is unscaled); True: Q16, the
    activation gradients in the S T domain as the device stores them.  -> dict: 'du' [l], 'dx' [l][j], 'dw' [l][j] (unscaled
    always); with rounded=True also 'floor:dw' and 'floor:dx'."""
    n = case['levels']
    S, T = (float(case['S']), float(case['T'])) if rounded else (1.0, 1.0)
    rnd = _r16 if rounded else (lambda t: t)
    u24 = 2.0 ** -24
    g = _nchw(case['dz']) / float(case['S']) * S                              # the device's dz (times S), or the unscaled gradient
    out = {'du': [], 'dx': [], 'dw': [], 'floor:dx': [], 'floor:dw': []}
    for l in range(n):
        dy = rnd(softmax_grad(_nchw(case['us'][l]), T * g))
        out['du'].append(dy)
        dxs, dws, fx, fw = [None] * (l + 1), [None] * (l + 1), [None] * (l + 1), [None] * (l + 1)
        for j in range(l, -1, -1):
            x = _nchw(case['xs'][l][j])
            w = torch.as_tensor(np.asarray(case['w'][l][j], np.float64))
            dx, dw = _layer_grads(x, w, dy)
            dws[j] = dw / (S * T)
            if rounded:
                ax, aw = _layer_grads(x.abs(), w.abs(), dy.abs())
                npix = x.shape[0] * x.shape[2] * x.shape[3]
                fw[j] = float(npix * u24 * aw.max() / (S * T))
                fx[j] = float(16 * x.shape[1] * u24 * ax.max())
            dy = rnd(dx)
            dxs[j] = dy
        out['dx'].append(dxs); out['dw'].append(dws); out['floor:dx'].append(fx); out['floor:dw'].append(fw)
    return out


def flat(res, scale=1.0):
    """{tensor name: fp64 numpy array} of a chain() result: 'du[l]', 'dx[l][j]', 'dw[l][j]'.  The activation gradients of an R64
    result are multiplied by ``scale`` (S T) so that they compare with the device's scaled fp16 maps."""
    out = {}
    for l, t in enumerate(res['du']):
        out['du[%d]' % l] = t.numpy() * scale
    for l, row in enumerate(res['dx']):
        for j, t in enumerate(row):
            out['dx[%d][%d]' % (l, j)] = t.numpy() * scale
    for l, row in enumerate(res['dw']):
        for j, t in enumerate(row):
            out['dw[%d][%d]' % (l, j)] = t.numpy()
    return out


def floors(res):
    out = {}
    for key in ('dx', 'dw'):
        for l, row in enumerate(res['floor:' + key]):
            for j, v in enumerate(row):
                out['%s[%d][%d]' % (key, l, j)] = v
    return out


def layer_exact(x, w, dy, st):
    """One transposed conv on integer-valued NHWC x, (ci, co, 4, 4) w and NHWC dy (2 Hi x 2 Wi): (dX NHWC, dW) in fp64, dW divided
    by st = S T.  The sums written out as the rule has them (no autograd): dW[ci][co][ky][kx] = sum X[y][x][ci] dY[2y+ky-1][2x+kx-1][co]."""
    x, w, dy = (np.asarray(a, np.float64) for a in (x, w, dy))
    B, Hi, Wi, C = x.shape
    pad = np.zeros((B, 2 * Hi + 2, 2 * Wi + 2, dy.shape[3]))
    pad[:, 1:-1, 1:-1] = dy
    dw = np.zeros(w.shape)
    dx = np.zeros(x.shape)
    for ky in range(4):
        for kx in range(4):
            win = pad[:, ky:ky + 2 * Hi:2, kx:kx + 2 * Wi:2]                  # dY[2y + ky - 1][2x + kx - 1]
            dw[:, :, ky, kx] = np.einsum('byxi,byxo->io', x, win)
            dx += np.einsum('byxo,io->byxi', win, w[:, :, ky, kx])
    return dx, dw / st
