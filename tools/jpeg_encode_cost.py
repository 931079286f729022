"""Cost of the JPEG encoding (the numbers of profiles/jpeg_encode.txt) on one batch of 32 synthetic frames of 384 x 1280 at
quality 90: the device stage rtm3d_frames_jpeg_fdct per chunk in 4:2:0 and 4:4:4 with the bytes it moves (two events around ONE
call with prebuilt descriptors, enqueued behind a matrix product of about a millisecond so that the call waits in the queue),
the copy of the coefficients to pinned memory, the host's Huffman coding of the batch at 1 and at 8 threads
(rtm3d_frames_jpeg_encode_finish), and the whole chain jpeg.encode (wall clock, frames on the device -> bytes on the host) at 1
and at 8 threads.  Each figure is taken once, after one warm-up call.  The frames are a gradient with saturated rectangles
and a patch of noise over a ninth of the picture: the Huffman coding's time depends on the content, camera frames code faster.

    python tools/jpeg_encode_cost.py [OUT.txt]
"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import _lib, jpeg          # noqa: E402

B, H, W, QUALITY = 32, 384, 1280, 90
COPY_TBS = 5.0                            # profiles/r04_hbm_rates.txt: copy (1 read + 1 write), 4.9-5.0 TB/s


def picture(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = rng.uniform(0, 255, (2, 3))
    img = a[0] + (a[1] - a[0]) * ((xx / (W - 1) + yy / (H - 1)) / 2)[:, :, None]
    for _ in range(40):
        y0, x0 = rng.integers(0, H), rng.integers(0, W)
        img[y0:y0 + rng.integers(1, H // 2), x0:x0 + rng.integers(1, W // 2)] = rng.choice([0.0, 255.0], 3)
    ny, nx = rng.integers(0, H), rng.integers(0, W)
    patch = img[ny:ny + H // 3, nx:nx + W // 3]
    patch[...] = rng.uniform(0, 255, patch.shape)
    return np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8)


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    frames = [torch.from_numpy(picture(b)).to(dev) for b in range(B)]
    luma, chroma = jpeg.quality_tables(QUALITY)
    stream = _lib.stream_ptr(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    busy = torch.randn(8192, 8192, device=dev, dtype=torch.float16)

    def device_time(fn):
        torch.cuda.synchronize()
        torch.mm(busy, busy)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    device_time(lambda: None)                            # the product's own warm-up
    px = B * H * W
    lines = ['workload: %d frames of %d x %d (h x w), quality %d, %.1f MB of packed pixels' % (B, H, W, QUALITY, 3 * px / 1e6)]
    for mode in ('420', '444'):
        count = jpeg.frame_layout(H, W, mode)['coef_count']
        coef = [torch.empty(count, dtype=torch.int16, device=dev) for _ in range(B)]
        arr = jpeg.c_enc_frames([(f, c, H, W, mode) for f, c in zip(frames, coef)])
        call = lambda: _lib.check(lib.rtm3d_frames_jpeg_fdct(stream, B, arr, luma.ctypes.data, chroma.ctypes.data, 0), 'frames_jpeg_fdct')
        call()                                           # warm-up
        t = device_time(call)
        moved = 3 * px + 2 * count * B
        lines.append('device stage, one chunk of %d frames in %s (rtm3d_frames_jpeg_fdct): %8.1f us  %.1f MB read + %.1f MB written = %.2f TB/s, %.0f %% of the '
                     '%.1f TB/s of a streaming copy' % (B, mode, t * 1e6, 3 * px / 1e6, 2 * count * B / 1e6, moved / t / 1e12, 100 * moved / t / 1e12 / COPY_TBS,
                                                       COPY_TBS))
        if mode != '420':
            continue
        d_all = torch.cat(coef)
        host = torch.empty(d_all.numel(), dtype=torch.int16).pin_memory()
        host.copy_(d_all, non_blocking=True)
        t = device_time(lambda: host.copy_(d_all, non_blocking=True))
        lines.append('copy of the coefficients (4:2:0), device -> pinned host: %8.1f us  %.1f GB/s' % (t * 1e6, 2 * d_all.numel() / t / 1e9))
        torch.cuda.synchronize()
        hw = (ctypes.c_int * (2 * B))(*([H, W] * B))
        bounds = [jpeg.encode_bound(H, W, mode)] * B
        outs = [np.empty(n, np.uint8) for n in bounds]
        ptrs = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs])
        caps, lens = (ctypes.c_size_t * B)(*bounds), (ctypes.c_size_t * B)()
        for threads in (1, 8):
            finish = lambda: _lib.check(lib.rtm3d_frames_jpeg_encode_finish(B, hw, 3, 0, host.data_ptr(), ptrs, caps, lens, threads), 'frames_jpeg_encode')
            finish()                                     # warm-up
            t0 = time.perf_counter()
            finish()
            t = time.perf_counter() - t0
            total = sum(lens)
            lines.append('host Huffman coding (4:2:0), %d thread%s: %8.2f ms  %7.0f frames/s  %7.1f MB/s of stream (%.2f MB, %.2f bits per pixel)'
                         % (threads, ' ' if threads == 1 else 's', t * 1e3, B / t, total / t / 1e6, total / 1e6, 8.0 * total / px))
    for threads in (1, 8):
        for _ in range(2):                               # both staging sets warm
            jpeg.encode(frames, quality=QUALITY, threads=threads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jpeg.encode(frames, quality=QUALITY, threads=threads)
        t = time.perf_counter() - t0
        lines.append('chain jpeg.encode (4:2:0), %d thread%s (frames on the device -> bytes on the host, wall clock): %8.2f ms  %7.0f frames/s'
                     % (threads, ' ' if threads == 1 else 's', t * 1e3, B / t))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args:
        with open(args[0], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
