"""Time the neck FPN backward (csrc/neck_fpn_backward.hip plus the kfpn_up launches of csrc/neck_backward.hip) launch by launch and as
a whole, at the bench shape: B = 32, the 96 x 320 map of z0, DLA-34's feature widths 64 / 128 / 256 / 512 - next to torch's own fp16
autograd over the same four 1x1 convs, three ConvTranspose2d and concats on the same card.  hipEvents around each call after a
warm-up call, median / min / max of --iters repeats; the whole chain and torch's forward + backward ALTERNATE inside one loop, so
both see the same clocks.  FLOPs are 2 x B H W x 256 x Cin per 1x1 wgrad and per dgrad and 2 x B Hi Wi x 16 x 256 x 256 per
transposed-conv wgrad and dgrad, with their shares of the 2.5 PFLOP/s dense fp16 rate DESIGN.md measures everything against; the
bytes are what a launch must move (operands once, results once; 8 TB/s peak).

    python tools/gpu_fpn_backward_time.py [--batch 32] [--map 96 320] [--iters 5] [--no-torch] >> profiles/neck_fpn_backward.txt
"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rtm3d_amd import _lib  # noqa: E402
from rtm3d_amd import head_train as ht  # noqa: E402
from rtm3d_amd import neck_train as nt  # noqa: E402
from rtm3d_amd import fpn_train as ft  # noqa: E402

PEAK, PEAK_BW = 2.5e15, 8.0e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--map', type=int, nargs=2, default=(96, 320))
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--fpn-scale', type=float, default=None)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    B, (H, W) = a.batch, a.map
    dev = torch.device('cuda')
    lib = _lib.load()
    fp = ft.FpnBackward(B, H, W, dev, grad_scale=ht.DEFAULT_GRAD_SCALE, fusion_scale=nt.DEFAULT_FUSION_SCALE, fpn_scale=a.fpn_scale)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd16 = lambda *s: torch.randn(*s, generator=gen, device=dev, dtype=torch.float16)

    def padded(h, w, c, P):
        t = torch.zeros(B, h + 2 * P, w + 2 * P, c, dtype=torch.float16, device=dev)
        t[:, P:P + h, P:P + w] = rnd16(B, h, w, c)
        return t
    dz_t = padded(H, W, 256, 0)
    ncat_t = [padded(*fp.hw(k), fp.cin[k], 1) for k in range(3)]
    h_t = [padded(*fp.hw(k + 1), 256, 1) for k in range(3)]
    F_t = [padded(*fp.hw(k + 1), 256, 1) for k in range(3)]
    feat3_t = padded(*fp.hw(3), fp.cin[3], 0)
    A16 = [rnd16(256, c) / 32 for c in fp.cin]
    wu16 = [rnd16(256, 256, 4, 4) / 32 for _ in range(3)]
    wr, wur = [ft.transpose_weights(w) for w in A16], [nt.rotate_deconv_weights(w) for w in wu16]
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    dA, db, dwu = [f32(256, c, 1, 1) for c in fp.cin], [f32(256) for _ in fp.cin], [f32(256, 256, 4, 4) for _ in range(3)]
    m = lambda t, c, P: ht.hb_map(t.data_ptr(), c, P)
    dz, feat3 = m(dz_t, 256, 0), m(feat3_t, fp.cin[3], 0)
    ncat, hm, F = [m(t, fp.cin[k], 1) for k, t in enumerate(ncat_t)], [m(t, 256, 1) for t in h_t], [m(t, 256, 1) for t in F_t]
    whole = lambda: fp.run(dz, ncat, hm, feat3, F, wr, wur, dA, db, dwu)
    whole()                                                                   # (fills every gradient map: the single launches below read them)
    torch.cuda.synchronize()

    st = _lib.stream_ptr(dev)
    ws, nws, ctr = fp.ws.data_ptr(), fp.ws.numel() * 4, fp.nonfinite.data_ptr()
    rows = []
    for k in range(4):
        Hk, Wk = fp.hw(k)
        npix, cin = B * Hk * Wk, fp.cin[k]
        g = dz if k == 0 else m(fp.g[k - 1], 256, 0)
        x = ncat[k] if k < 3 else feat3
        out = m(fp.D[k], cin, 1) if k < 3 else m(fp.dfeat3, cin, 0)
        inv = 1.0 / fp.S if k == 0 else 1.0 / (fp.S * fp.U)
        flops = 2.0 * npix * 256 * cin
        tag = '%s (%d x %d, Cin %d)' % (ft.conv_launch_names()[k], Hk, Wk, cin)
        rows.append((tag + ' wgrad + bias + reduce', flops, npix * (256 + cin) * 2.0, lambda k=k, Hk=Hk, Wk=Wk, cin=cin, x=x, g=g, inv=inv: _lib.check(
            lib.rtm3d_fpn_conv1x1_wgrad(st, B, Hk, Wk, cin, ctypes.byref(x), ctypes.byref(g), inv, dA[k].data_ptr(), db[k].data_ptr(), fp.want[k], ws, nws, ctr), 'wgrad')))
        rows.append((tag + ' dgrad', flops, npix * (256 + cin) * 2.0, lambda k=k, Hk=Hk, Wk=Wk, cin=cin, g=g, out=out: _lib.check(
            lib.rtm3d_fpn_conv1x1_dgrad(st, B, Hk, Wk, cin, ctypes.byref(g), wr[k].data_ptr(), fp.U if k == 0 else 1.0, ctypes.byref(out)), 'dgrad')))
        if k == 3:
            break
        Hi, Wi = fp.hw(k + 1)
        dflops = 2.0 * B * Hi * Wi * 16 * 256 * 256
        e, gk = m(fp.E[k], 256, 0), m(fp.g[k], 256, 0)
        rows.append(('kfpn_up%d (%d x %d in) wgrad + reduce' % (k + 3, Hi, Wi), dflops, 0.0, lambda k=k, Hi=Hi, Wi=Wi, out=out: _lib.check(
            lib.rtm3d_neck_deconv_wgrad(st, B, Hi, Wi, ctypes.byref(hm[k]), ctypes.byref(out), fp.S, fp.U, dwu[k].data_ptr(), fp.want_up, ws, nws, ctr), 'up wgrad')))
        rows.append(('kfpn_up%d (%d x %d in) dgrad' % (k + 3, Hi, Wi), dflops, 0.0, lambda k=k, Hi=Hi, Wi=Wi, out=out, e=e: _lib.check(
            lib.rtm3d_neck_deconv_dgrad(st, B, Hi, Wi, ctypes.byref(out), wur[k].data_ptr(), ctypes.byref(e)), 'up dgrad')))
        rows.append(('grad add at kfpn_h%d (%d x %d)' % (k + 3, Hi, Wi), 0.0, B * Hi * Wi * 256 * 2.0 * 3, lambda k=k, Hi=Hi, Wi=Wi, e=e, gk=gk: _lib.check(
            lib.rtm3d_fpn_grad_add(st, B, Hi, Wi, ctypes.byref(e), ctypes.byref(F[k]), fp.U / fp.T, ctypes.byref(gk)), 'add')))
    total = sum(r[1] for r in rows)
    print('neck FPN backward, B = %d, map %d x %d, Cin %s, K-slices wanted %s (1x1) / %d (kfpn_up); S = 2 ** %d, T = 2 ** %d, U = 2 ** %d; MI355X (gfx950)'
          % (B, H, W, fp.cin, fp.want, fp.want_up, int(torch.tensor(fp.S).log2()), int(torch.tensor(fp.T).log2()), int(torch.tensor(fp.U).log2())))
    print('%-58s %9s %9s %9s %9s %8s %8s' % ('launch', 'median ms', 'min', 'max', 'TFLOP/s', 'of 2.5PF', 'GB/s'))
    for name, flops, nbytes, fn in rows:
        fn()
        torch.cuda.synchronize()
        med, lo, hi_ = stats([event_ms(fn) for _ in range(a.iters)])
        print('%-58s %9.3f %9.3f %9.3f %9.1f %8.3f %8.0f' % (name, med, lo, hi_, flops / med / 1e9, flops / med / 1e-3 / PEAK, nbytes / med / 1e6))
    print('non-finite parameter gradients counted: %d' % int(fp.nonfinite.item()))
    if a.no_torch:
        med, lo, hi_ = stats([event_ms(whole) for _ in range(a.iters)])
        print('%-58s %9.3f %9.3f %9.3f %9.1f %8.3f' % ('whole FPN backward', med, lo, hi_, total / med / 1e9, total / med / 1e-3 / PEAK))
        return
    # torch: the same function through its own fp16 autograd (NCHW leaves, conv2d, conv_transpose2d, cat)
    import torch.nn.functional as Fn
    nchw = lambda t, P: (t[:, P:t.shape[1] - P, P:t.shape[2] - P] if P else t).permute(0, 3, 1, 2).contiguous()
    feats = [nchw(ncat_t[k], 1)[:, 256:].contiguous().requires_grad_(True) for k in range(3)] + [nchw(feat3_t, 0).requires_grad_(True)]
    At = [w.clone().view(256, -1, 1, 1).requires_grad_(True) for w in A16]
    bt = [torch.zeros(256, dtype=torch.float16, device=dev, requires_grad=True) for _ in A16]
    wt = [w.clone().requires_grad_(True) for w in wu16]
    gz = nchw(dz_t, 0)
    gF = [nchw(t, 1) for t in F_t]

    def fwd():
        hk = Fn.conv2d(feats[3], At[3], bt[3])
        outs = []
        for k in (2, 1, 0):
            outs.append(hk)
            hk = Fn.conv2d(torch.cat([Fn.conv_transpose2d(hk, wt[k], stride=2, padding=1), feats[k]], 1), At[k], bt[k])
        return [hk] + outs[::-1]

    def fwd_only():
        with torch.no_grad():
            fwd()

    def fwd_bwd():
        for t in feats + At + bt + wt:
            t.grad = None
        torch.autograd.backward(fwd(), [gz] + gF)
    fwd_only(); fwd_bwd(); whole()
    torch.cuda.synchronize()
    ours, tf, tfb = [], [], []
    for _ in range(a.iters):                                                  # alternating: one of each per round
        ours.append(event_ms(whole)); tf.append(event_ms(fwd_only)); tfb.append(event_ms(fwd_bwd))
    med, lo, hi_ = stats(ours)
    print('%-58s %9.3f %9.3f %9.3f %9.1f %8.3f' % ('whole FPN backward', med, lo, hi_, total / med / 1e9, total / med / 1e-3 / PEAK))
    f_med, fb_med = stats(tf)[0], stats(tfb)
    print('torch fp16 autograd, the same four 1x1 convs + three ConvTranspose2d + cat: forward %.3f ms, forward + backward %.3f ms (min %.3f, max %.3f) '
          '-> backward %.3f ms' % (f_med, fb_med[0], fb_med[1], fb_med[2], fb_med[0] - f_med))
    print('ratio: this backward / torch backward = %.2f' % (med / (fb_med[0] - f_med)))


if __name__ == '__main__':
    main()
