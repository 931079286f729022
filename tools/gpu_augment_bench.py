"""Device time of rtm3d_frames_augment (the numbers of profiles/augment.txt): bs 32 of 375 x 1242 frames onto a 384 x 1280
canvas, out_mode 1 (fp16 NHWC4 with the plan's border of 4), no Resize - with identity parameters, with each step alone and with
everything on (brightness / contrast, noise, zoom 1.1 with the reference's offset, mirror) - next to rtm3d_preprocess_batch on
the same frames into the same buffer (the validation path: the floor) and to a composition of the same steps in torch device ops
(affine_grid / grid_sample, randn, flip, pad, normalise).  hipEvents around CALLS back-to-back calls on the current stream,
enqueued behind a matrix product of about a millisecond so that the calls wait in the queue and the time between the events is
the device's; the variants are interleaved over ROUNDS rounds after one warm-up call each.  The kernels are called through the C
entry points with prebuilt descriptors.  Bytes moved, from the shapes: every source byte read once (3 B per source pixel) and 8 B
written per canvas pixel.  Before anything is timed the identity call is compared with preprocess_batch's output bit for bit.

    python tools/gpu_augment_bench.py [OUT.txt]
"""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import _lib, augment, preprocess    # noqa: E402

B, ROUNDS, CALLS = 32, 5, 10
H_SRC, W_SRC, H, W, BORDER = 375, 1242, 384, 1280, 4
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def params_for(photo=False, noise=False, zoom=False, mirror=False):
    P = augment.AugmentParams.identity(B)
    rng = np.random.Generator(np.random.PCG64(2))
    if photo:
        P.alpha[:], P.beta[:] = 1 + rng.uniform(-0.2, 0.2, B), rng.uniform(-0.2, 0.2, B)
    if noise:
        P.sigma[:] = np.sqrt(rng.uniform(10, 50, B))
        P.seed[:] = rng.integers(0, 2 ** 63, B).astype(np.uint64)
    if zoom:
        P.scale[:] = 1.1
        P.offset[:] = augment.affine_offset_of(W_SRC, H_SRC, 1.1)
    if mirror:
        P.flip[:] = True
    return P


def torch_composition(frames_u8, P, mean, std, out):
    """The same steps in torch device ops, one batch: (B, h, w, 3) uint8 -> fp16 NHWC4 canvas with a border."""
    x = frames_u8.permute(0, 3, 1, 2).float()
    a = torch.as_tensor(P.alpha, dtype=torch.float32, device=x.device).view(-1, 1, 1, 1)
    b = torch.as_tensor(P.beta * 255, dtype=torch.float32, device=x.device).view(-1, 1, 1, 1)
    s = torch.as_tensor(P.sigma, dtype=torch.float32, device=x.device).view(-1, 1, 1, 1)
    x = (x * a + b).clamp_(0, 255)
    x = (x + torch.randn_like(x) * s).clamp_(0, 255)
    # dst = scale * src + offset  ->  src = (dst - offset) / scale, in normalised coordinates
    sc = torch.as_tensor(P.scale, dtype=torch.float32, device=x.device)
    off = torch.as_tensor(P.offset, dtype=torch.float32, device=x.device)
    theta = torch.zeros(B, 2, 3, device=x.device)
    theta[:, 0, 0], theta[:, 1, 1] = 1 / sc, 1 / sc
    theta[:, 0, 2] = (1 / sc - 1) - (1 + 2 * off[:, 0]) / (sc * W_SRC) + 1 / W_SRC
    theta[:, 1, 2] = (1 / sc - 1) - (1 + 2 * off[:, 1]) / (sc * H_SRC) + 1 / H_SRC
    x = F.grid_sample(x, F.affine_grid(theta, list(x.shape), align_corners=False), mode='bilinear', padding_mode='zeros', align_corners=False)
    flip = torch.as_tensor(P.flip, device=x.device).view(-1, 1, 1, 1)
    x = torch.where(flip, x.flip(3), x)
    x = x.round_()
    pad_w, pad_h = (W - W_SRC) // 2, (H - H_SRC) // 2
    colour = x.mean(dim=(2, 3), keepdim=True).floor_()
    canvas = colour.expand(B, 3, H, W).clone()
    canvas[:, :, pad_h:pad_h + H_SRC, pad_w:pad_w + W_SRC] = x
    canvas = (canvas / 255 - mean) / std
    out[:, BORDER:BORDER + H, BORDER:BORDER + W, :3] = canvas.permute(0, 2, 3, 1).half()
    return out


def timed(variants, rounds, calls):
    times = [[] for _ in variants]
    for _, fn in variants:
        fn()
    a16 = torch.ones(8192, 8192, dtype=torch.float16, device='cuda')
    torch.mm(a16, a16)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for i, (_, fn) in enumerate(variants):
            torch.mm(a16, a16)                   # keeps the queue busy, so the host side of the timed calls hides behind the device
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) * 1e3 / calls)
    return times


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.Generator(np.random.PCG64(1))
    batch = torch.from_numpy(rng.integers(0, 256, (B, H_SRC, W_SRC, 3), dtype=np.uint8)).to(dev)
    frames = [batch[b] for b in range(B)]
    src = _lib.ptr_array(frames)
    hw = np.array([[H_SRC, W_SRC]] * B, np.int32)
    d_lut, d_lut16 = preprocess.device_luts(MEAN, STD, dev)
    table = augment.device_noise_table(dev)
    sums = torch.zeros(B, 3, dtype=torch.int64, device=dev)
    out = torch.zeros(B, H + 2 * BORDER, W + 2 * BORDER, 4, dtype=torch.float16, device=dev)
    out_ref = torch.zeros_like(out)
    out_t = torch.zeros_like(out)
    mean_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device=dev).view(1, 3, 1, 1)

    def aug_call(desc, dst=out):
        rc = lib.rtm3d_frames_augment(stream, B, src, desc, ctypes.c_void_p(dst.data_ptr()), 1, H, W, BORDER, table.data_ptr(), d_lut.data_ptr(),
                                      d_lut16.data_ptr(), sums.data_ptr())
        assert rc == 0, lib.rtm3d_last_error().decode()

    def pre_call(dst=out_ref):
        rc = lib.rtm3d_preprocess_batch(stream, B, src, hw.ctypes.data_as(ctypes.c_void_p), None, ctypes.c_void_p(dst.data_ptr()), 1, H, W, BORDER,
                                        d_lut.data_ptr(), d_lut16.data_ptr(), sums.data_ptr())
        assert rc == 0, lib.rtm3d_last_error().decode()

    sets = [('identity', params_for()), ('brightness / contrast alone', params_for(photo=True)), ('noise alone', params_for(noise=True)),
            ('zoom 1.1 + mirror alone', params_for(zoom=True, mirror=True)), ('everything on', params_for(True, True, True, True))]
    descs = [(name, augment.descriptors(hw, P, (H, W))[0], P) for name, P in sets]
    aug_call(descs[0][1])
    pre_call()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out_ref.view(torch.int16)), 'identity augmentation differs from preprocess_batch'
    variants = [('frames_augment   %-28s' % name, lambda d=d: aug_call(d)) for name, d, _ in descs]
    variants.append(('preprocess_batch %-28s' % '(validation path, the floor)', pre_call))
    variants.append(('torch device ops %-28s' % 'everything on', lambda: torch_composition(batch, sets[-1][1], mean_t, std_t, out_t)))
    times = timed(variants, ROUNDS, CALLS)
    moved = B * H_SRC * W_SRC * 3 + B * H * W * 8
    lines = ['bs %d of %d x %d uint8 frames -> %d x %d canvas, fp16 NHWC4 (border %d), no Resize; per call; %d interleaved rounds x %d calls'
             % (B, H_SRC, W_SRC, H, W, BORDER, ROUNDS, CALLS),
             'bytes from the shapes: %.1f MB read once + %.1f MB written = %.1f MB per batch' % (B * H_SRC * W_SRC * 3 / 1e6, B * H * W * 8 / 1e6, moved / 1e6),
             'identity output == preprocess_batch output, bit for bit: checked before timing']
    med = [float(np.median(t)) for t in times]
    for (name, _), t, m in zip(variants, times, med):
        lines.append('%s median %8.1f us  min %8.1f  max %8.1f   %5.2f TB/s of the %.1f MB' % (name, m, np.min(t), np.max(t), moved / (m * 1e-6) / 1e12, moved / 1e6))
    lines.append('ratios of medians: everything on / identity %.2f;  identity / preprocess_batch %.2f;  everything on / preprocess_batch %.2f;  '
                 'torch device ops / everything on %.2f' % (med[4] / med[0], med[0] / med[5], med[4] / med[5], med[6] / med[4]))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args:
        with open(args[0], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
