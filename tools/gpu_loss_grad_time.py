"""hipEvent times of the loss gradient on one MI355X at B = 32, 3 x 96 x 320 maps (the 384 x 1280 input of the benchmark), 10
objects per image: rtm3d_loss_grad alone (the C entry point, preallocated outputs, the forward's counts on the device), the
forward-only RTM3DLoss(pred, batch) call, forward + backward through the wrapper (``loss, _ = RTM3DLoss(cfg)(leaves, batch);
loss.backward()``), and what a user would otherwise run: torch autograd over ``torch_loss`` of tools/gpu_loss_time.py on a
materialised target, forward + backward.  The two gradients are checked against each other before timing.
Median (min) of 20 timed groups of 10 calls after a warm-up.  Prints the table; with an argument, also appends it to that file
(profiles/loss_grad.txt holds its output)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_loss_time import B, C, H, W, PER_IMAGE, GROUPS, PER, torch_loss  # noqa: E402


def main():
    import numpy as np
    import torch
    from rtm3d_amd import _lib, loss as L
    from tests import loss_cases as lc
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    rng = np.random.default_rng(11)
    objs = sum([lc._scene(rng, b, PER_IMAGE, H, W) for b in range(B)], [])
    batch = lc.batch(lc._case(B, H, W, objs)).to(dev)
    pred = [(torch.randn(B, ch, H, W, device=dev) * 2).contiguous() for ch in (C, 16, 2, 2)]
    pred[0] -= 3.0
    fn = L.RTM3DLoss()
    tg = L.build_targets(batch, H, W)
    tab, start = batch.table(H, W), batch._dev[2]

    # agreement: the fused gradient against torch autograd on the materialised target
    leaves = [p.clone().requires_grad_(True) for p in pred]
    loss, items = fn(leaves, batch)
    loss.backward()
    fused = [leaf.grad for leaf in leaves]
    tleaves = [p.clone().requires_grad_(True) for p in pred]
    torch_loss(tleaves, tg)[4].backward()
    torch.cuda.synchronize()
    agree = []
    for a, t in zip(fused, tleaves):
        assert torch.equal(a == 0, t.grad == 0), 'zero patterns differ'
        agree.append(((a - t.grad).abs().max() / t.grad.abs().max()).item())
    assert max(agree) < 1e-5, agree
    explicit = fn.grad(pred, batch)
    assert all(torch.equal(a, b) for a, b in zip(fused, explicit))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            f()
        t = []
        for _ in range(GROUPS):
            e0.record()
            for _ in range(PER):
                f()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / PER)
        return float(np.median(t)), float(min(t))

    stream = _lib.stream_ptr(dev)
    with torch.no_grad():
        fn(pred, batch)
    counts = fn.counts
    outs = [torch.empty_like(p) for p in pred]

    def f_grad_c():
        _lib.check(lib.rtm3d_loss_grad(stream, B, C, H, W, pred[0].data_ptr(), pred[1].data_ptr(), pred[2].data_ptr(), pred[3].data_ptr(),
                                       start.data_ptr(), tab.data_ptr(), batch.N, ctypes.byref(fn._params), counts.data_ptr(), None,
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr()))

    def f_grad_hm():
        _lib.check(lib.rtm3d_loss_grad(stream, B, C, H, W, pred[0].data_ptr(), pred[1].data_ptr(), pred[2].data_ptr(), pred[3].data_ptr(),
                                       start.data_ptr(), tab.data_ptr(), batch.N, ctypes.byref(fn._params), counts.data_ptr(), None,
                                       outs[0].data_ptr(), None, None, None))

    def f_forward():
        with torch.no_grad():
            fn(pred, batch)

    def f_both():
        for leaf in leaves:
            leaf.grad = None
        fn(leaves, batch)[0].backward()

    def f_torch():
        for leaf in tleaves:
            leaf.grad = None
        torch_loss(tleaves, tg)[4].backward()

    res = [('rtm3d_loss_grad through the C entry point, all four maps (2 launches)', timed(f_grad_c)),
           ('rtm3d_loss_grad, the heat-map gradient only (1 launch, no zeros)', timed(f_grad_hm)),
           ('RTM3DLoss(pred, batch), forward only, no grad (2 launches)', timed(f_forward)),
           ('forward + backward through the wrapper: loss.backward() into four leaves', timed(f_both)),
           ('torch autograd over torch_loss on the materialised target, forward + backward', timed(f_torch))]
    moved = 4.0 * B * H * W * (C + C + 20)
    lines = ['loss gradient, us per call: median (min) of %d groups of %d back-to-back calls, hipEvent' % (GROUPS, PER),
             'B=%d, %d x %d x %d maps, %d objects (%.1f per image), counts %s; fused vs torch autograd, max abs difference over the '
             'largest magnitude per map: %s' % (B, C, H, W, batch.N, batch.N / B, counts.tolist(), ', '.join('%.1e' % a for a in agree))]
    lines += ['  %-84s %9.1f (%.1f)' % (n + ':', m, lo) for n, (m, lo) in res]
    lines.append('  rtm3d_loss_grad moves at least %.1f MB (%.1f in, %.1f out, %.1f of zeros): %.2f TB/s over the whole call'
                 % (moved / 1e6, 4.0 * B * H * W * C / 1e6, 4.0 * B * H * W * C / 1e6, 4.0 * B * H * W * 20 / 1e6, moved / res[0][1][0] / 1e6))
    lines.append('  fused forward + backward %.1f us against torch autograd %.1f us: %s'
                 % (res[3][1][0], res[4][1][0], 'the fused path is %.1fx faster' % (res[4][1][0] / res[3][1][0])
                    if res[4][1][0] > res[3][1][0] else 'the fused path is NOT faster'))
    print('\n'.join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
