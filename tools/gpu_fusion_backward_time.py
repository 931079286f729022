"""Time the neck fusion backward (csrc/neck_backward.hip) launch by launch and as a whole, at the bench shape: B = 32, the
96 x 320 map of z, DLA-34's 256 channels, three operands with chains of 1 / 2 / 3 transposed convs - next to torch's own fp16
autograd over the same six ConvTranspose2d plus the detached softmax product on the same card.  hipEvents around each call after
a warm-up call, median / min / max of --iters repeats; FLOPs are 2 x B Hi Wi x 16 taps x 256 x 256 per wgrad and per dgrad, their
shares of the 2.5 PFLOP/s dense fp16 rate DESIGN.md measures everything against; the softmax pass is memory-bound and reported in
GB/s of the bytes it must move (u twice, dz once, du once; 8 TB/s peak).

    python tools/gpu_fusion_backward_time.py [--batch 32] [--map 96 320] [--iters 5] [--no-torch] >> profiles/neck_backward.txt
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

PEAK, PEAK_BW = 2.5e15, 8.0e12


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(iters):
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b))
    best.sort()
    return best[len(best) // 2], best[0], best[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--map', type=int, nargs=2, default=(96, 320))
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    B, (H, W), n = a.batch, a.map, 3
    dev = torch.device('cuda')
    lib = _lib.load()
    fb = nt.FusionBackward(B, H, W, dev, n, ht.DEFAULT_GRAD_SCALE, nt.DEFAULT_FUSION_SCALE)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd16 = lambda *s: torch.randn(*s, generator=gen, device=dev, dtype=torch.float16)

    def padded(h, w, P):
        t = torch.zeros(B, h + 2 * P, w + 2 * P, 256, dtype=torch.float16, device=dev)
        t[:, P:P + h, P:P + w] = rnd16(B, h, w, 256)
        return t
    dz_t = padded(H, W, 0)
    u_t = [padded(H, W, 0) for _ in range(n)]
    x_t = [[padded(*fb.in_hw(l, j), 1) for j in range(l + 1)] for l in range(n)]
    w16 = [[rnd16(256, 256, 4, 4) / 32 for _ in range(l + 1)] for l in range(n)]
    wr = [[nt.rotate_deconv_weights(w) for w in row] for row in w16]
    dw = [[torch.empty(256, 256, 4, 4, dtype=torch.float32, device=dev) for _ in range(l + 1)] for l in range(n)]
    dz = ht.hb_map(dz_t.data_ptr(), 256, 0)
    us = [ht.hb_map(t.data_ptr(), 256, 0) for t in u_t]
    xs = [[ht.hb_map(t.data_ptr(), 256, 1) for t in row] for row in x_t]
    whole = lambda: fb.run(dz, us, xs, wr, dw)
    whole()                                                                   # (fills du and every dX: the single launches below read them)

    st = _lib.stream_ptr(dev)
    ws, nws = fb.ws.data_ptr(), fb.ws.numel() * 4
    arr = lambda maps: (_lib.HbMapC * n)(*maps)
    npix = B * H * W
    rows = [('softmax stats + combine + grad, 3 operands', 0.0, 3 * npix * 256 * 2 * 4.0,
             lambda: _lib.check(lib.rtm3d_neck_softmax_grad(st, B, H, W, n, ctypes.byref(dz), arr(us), arr([fb.du_map(l) for l in range(n)]), fb.T, ws, nws), 'softmax'))]
    for l in range(n):
        for j in range(l, -1, -1):
            hi, wi = fb.in_hw(l, j)
            dy = fb.du_map(l) if j == l else fb.dx_map(l, j + 1)
            flops = 2.0 * B * hi * wi * 16 * 256 * 256
            tag = 'fusion_up%d.%d (%d x %d in)' % (l + 3, j, hi, wi)
            rows.append((tag + ' wgrad + reduce', flops, 0.0, lambda l=l, j=j, hi=hi, wi=wi, dy=dy: _lib.check(lib.rtm3d_neck_deconv_wgrad(
                st, B, hi, wi, ctypes.byref(xs[l][j]), ctypes.byref(dy), fb.S, fb.T, dw[l][j].data_ptr(), fb.want, ws, nws, fb.nonfinite.data_ptr()), 'wgrad')))
            dx = fb.dx_map(l, j)
            rows.append((tag + ' dgrad', flops, 0.0, lambda l=l, j=j, hi=hi, wi=wi, dy=dy, dx=dx: _lib.check(lib.rtm3d_neck_deconv_dgrad(
                st, B, hi, wi, ctypes.byref(dy), wr[l][j].data_ptr(), ctypes.byref(dx)), 'dgrad')))
    total = sum(r[1] for r in rows)
    rows.append(('whole fusion backward', total, 0.0, whole))
    print('neck fusion backward, B = %d, map %d x %d, 3 operands, %d K-slices wanted; S = 2 ** %d, T = 2 ** %d; MI355X (gfx950)'
          % (B, H, W, fb.want, int(torch.tensor(fb.S).log2()), int(torch.tensor(fb.T).log2())))
    print('%-52s %9s %9s %9s %9s %8s %8s' % ('launch', 'median ms', 'min', 'max', 'TFLOP/s', 'of 2.5PF', 'GB/s'))
    ours = None
    for name, flops, nbytes, fn in rows:
        med, lo, hi_ = timed(fn, a.iters)
        print('%-52s %9.3f %9.3f %9.3f %9.1f %8.3f %8.0f' % (name, med, lo, hi_, flops / med / 1e9, flops / med / 1e-3 / PEAK, nbytes / med / 1e6))
        ours = med
    print('non-finite weight gradients counted: %d' % int(fb.nonfinite.item()))
    if a.no_torch:
        return
    # torch: the same function through its own fp16 autograd (NCHW leaves, conv_transpose2d, detached softmax product)
    import torch.nn.functional as F
    h = [x_t[l][0][:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous().requires_grad_(True) for l in range(n)]
    wt = [[w.clone().requires_grad_(True) for w in row] for row in w16]
    g = dz_t.permute(0, 3, 1, 2).contiguous()

    def fwd():
        z = None
        for l in range(n):
            u = h[l]
            for j in range(l + 1):
                u = F.conv_transpose2d(u, wt[l][j], stride=2, padding=1)
            zi = u * torch.softmax(u.detach().float().view(B, 256, -1), dim=-1).view(B, 256, H, W).half()
            z = zi if z is None else z + zi
        return z

    def fwd_only():
        with torch.no_grad():
            fwd()

    def fwd_bwd():
        for t in h + [w for row in wt for w in row]:
            t.grad = None
        fwd().backward(g)
    f_med, _, _ = timed(fwd_only, a.iters)
    fb_med, fb_lo, fb_hi = timed(fwd_bwd, a.iters)
    print('torch fp16 autograd, the same six ConvTranspose2d + softmax product: forward %.3f ms, forward + backward %.3f ms (min %.3f, max %.3f) '
          '-> backward %.3f ms' % (f_med, fb_med, fb_lo, fb_hi, fb_med - f_med))
    print('ratio: this backward / torch backward = %.2f' % (ours / (fb_med - f_med)))


if __name__ == '__main__':
    main()
