"""Time the head backward (csrc/head_backward.hip) launch by launch and as a whole, at the bench shape: B = 32, a 96 x 320 map, the
four DLA-34 heads (K = 3, 16, 2, 2; HEADER_NUM_CONV = 2), next to the same heads' backward through torch's own fp16 conv
autograd on the device.  FLOP shares are of the 2.5 PFLOP/s dense fp16 rate DESIGN.md measures everything against.

    python tools/gpu_head_backward_time.py [--batch 32] [--map 96 320] [--iters 5] [--no-torch] > profiles/head_backward.txt
"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rtm3d_amd import _lib  # noqa: E402
from rtm3d_amd import head_train as ht  # noqa: E402

PEAK = 2.5e15
K = (3, 16, 2, 2)


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
    B, (H, W), G, n = a.batch, a.map, len(K), 2
    dev = torch.device('cuda')
    lib = _lib.load()
    hb = ht.HeadBackward(B, H, W, K, n, dev, 1024.0, True)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd16 = lambda *s: torch.randn(*s, generator=gen, device=dev, dtype=torch.float16)

    def padded(C, P, relu):
        t = torch.zeros(B, H + 2 * P, W + 2 * P, C, dtype=torch.float16, device=dev)
        v = rnd16(B, H, W, C)
        t[:, P:P + H, P:P + W] = torch.relu(v) if relu else v
        return t
    keep = [padded(256, 6, False), padded(G * 256, 1, True), padded(G * 256, 1, True)]
    acts = [ht.hb_map(keep[0].data_ptr(), 256, 6, 0, 0)] + [ht.hb_map(keep[k].data_ptr(), G * 256, 1, 0, 256) for k in (1, 2)]
    wf = [None] + [(rnd16(G, 256, 256, 3, 3) * 0.02) for _ in range(n)]
    wr = [None] + [ht.rotate_weights(w) for w in wf[1:]]
    wo = torch.zeros(G, 16, 256, 3, 3, dtype=torch.float16, device=dev)
    for g in range(G):
        wo[g, :K[g]] = rnd16(K[g], 256, 3, 3) * 0.02
    wr_out = ht.rotate_weights(wo)
    scales = [None] + [[torch.ones(256, device=dev) for _ in range(G)] for _ in range(n)]
    dl = [torch.randn(B, k, H, W, generator=gen, device=dev) * 1e-3 for k in K]
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    dw = [None] + [[f32(256, 256, 3, 3) for _ in range(G)] for _ in range(n)]
    db = [None] + [[f32(256) for _ in range(G)] for _ in range(n)]
    dwo, dbo = [f32(k, 256, 3, 3) for k in K], [f32(k) for k in K]
    whole = lambda: hb.run(dl, acts, wr, wr_out, scales, dw, db, dwo, dbo)

    st = _lib.stream_ptr(dev)
    go = hb.go_map()
    npix = B * H * W
    big = 2.0 * npix * 9 * 256 * 256 * G
    small = 2.0 * npix * 9 * 16 * 256 * G
    none4 = [None] * G
    steps = [
        ('go', 0.0, lambda: _lib.check(lib.rtm3d_head_go(st, B, H, W, G, (ctypes.c_int * 4)(*K), (ctypes.c_void_p * 4)(*[t.data_ptr() for t in dl]),
                                                            hb.S, ctypes.byref(go)), 'go')),
        ('final wgrad (+ colsum, reduce)', small, lambda: hb._wgrad(lib, st, 1, 16, K, go, acts[2], None, dwo, dbo)),
        ('final dgrad', small, lambda: _lib.check(lib.rtm3d_head_dgrad(st, B, H, W, G, 1, 1, 16, ctypes.byref(go), wr_out.data_ptr(), ctypes.byref(acts[2]),
                                                                       ctypes.byref(hb.dh_map(2))), 'dgrad')),
        ('d1 wgrad (+ colsum, reduce)', big, lambda: hb._wgrad(lib, st, 1, 256, [256] * G, hb.dh_map(2), acts[1], scales[2], dw[2], db[2])),
        ('d1 wgrad, weights only', big, lambda: hb._wgrad(lib, st, 1, 256, [256] * G, hb.dh_map(2), acts[1], scales[2], dw[2], none4)),
        ('d1 dgrad', big, lambda: _lib.check(lib.rtm3d_head_dgrad(st, B, H, W, G, 1, 1, 256, ctypes.byref(hb.dh_map(2)), wr[2].data_ptr(), ctypes.byref(acts[1]),
                                                                  ctypes.byref(hb.dh_map(1))), 'dgrad')),
        ('d6 wgrad (+ colsum, reduce)', big, lambda: hb._wgrad(lib, st, 6, 256, [256] * G, hb.dh_map(1), acts[0], scales[1], dw[1], db[1])),
        ('d6 dgrad (dz)', big, lambda: _lib.check(lib.rtm3d_head_dgrad(st, B, H, W, 1, G, 6, 256, ctypes.byref(hb.dh_map(1)), wr[1].data_ptr(), None,
                                                                       ctypes.byref(ht.hb_map(hb.dz.data_ptr(), 256, 0, 0, 0))), 'dgrad')),
    ]
    print('head backward, B = %d, map %d x %d, G = %d, K = %s, HEADER_NUM_CONV = %d, %d K-slices of %d tiles; %s'
          % (B, H, W, G, K, n, hb.n_slices, hb.tiles_per_slice, torch.cuda.get_device_name(0)))
    print('%-34s %10s %10s %10s %12s %8s' % ('launch', 'median ms', 'min', 'max', 'TFLOP/s', 'of 2.5PF'))
    whole()
    for name, flops, fn in steps:
        med, lo, hi = timed(fn, a.iters)
        print('%-34s %10.3f %10.3f %10.3f %12.1f %8.3f' % (name, med, lo, hi, flops / med / 1e9, flops / med / 1e-3 / PEAK))
    med, lo, hi = timed(whole, a.iters)
    total = 4 * big + 2 * small
    print('%-34s %10.3f %10.3f %10.3f %12.1f %8.3f' % ('whole backward', med, lo, hi, total / med / 1e9, total / med / 1e-3 / PEAK))
    print('non-finite parameter gradients counted: %d' % int(hb.nonfinite.item()))
    ours = med
    if a.no_torch:
        return
    del hb
    # the same heads through torch's fp16 conv autograd (NCHW, what torch picks for these shapes)
    import torch.nn.functional as F
    x = keep[0][:, 6:-6, 6:-6].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    params = []
    for g in range(G):
        params.append([wf[1][g].clone().requires_grad_(True), wf[2][g].clone().requires_grad_(True), wo[g, :K[g]].clone().requires_grad_(True),
                       torch.zeros(256, dtype=torch.float16, device=dev, requires_grad=True), torch.zeros(256, dtype=torch.float16, device=dev, requires_grad=True),
                       torch.zeros(K[g], dtype=torch.float16, device=dev, requires_grad=True)])
    del keep, acts
    up = [d.half() for d in dl]

    def fwd():
        outs = []
        for g in range(G):
            w1, w2, w3, b1, b2, b3 = params[g]
            h = torch.relu(F.conv2d(x, w1, b1, dilation=6, padding=6))
            h = torch.relu(F.conv2d(h, w2, b2, padding=1))
            outs.append(F.conv2d(h, w3, b3, padding=1))
        return outs
    leaves = [x] + [p for ps in params for p in ps]

    def fb():
        torch.autograd.grad(fwd(), leaves, up)
    f_med, _, _ = timed(lambda: [o for o in fwd()], a.iters)
    fb_med, fb_lo, fb_hi = timed(fb, a.iters)
    print('torch fp16 conv autograd, the same heads: forward %.3f ms, forward + backward %.3f ms (min %.3f, max %.3f) -> backward %.3f ms'
          % (f_med, fb_med, fb_lo, fb_hi, fb_med - f_med))
    print('ratio: this backward / torch backward = %.2f' % (ours / (fb_med - f_med)))


if __name__ == '__main__':
    main()
