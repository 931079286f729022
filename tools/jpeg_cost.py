"""Cost of the JPEG frame stage (the numbers of profiles/jpeg.txt) on one batch of 32 JPEG files: the host's entropy decode at 1
and at 8 threads (MB/s of stream and frames/s), the device stage per chunk with the bytes it moves and the copy of the
coefficients from pinned memory (two events around ONE call with prebuilt descriptors, enqueued behind a matrix product of about
a millisecond so that the call waits in the queue), and the whole chain jpeg.decode (wall clock to the end of the last kernel)
at 1 and at 8 threads.  Each figure is taken once, after one warm-up call.  The library makes no JPEG
files: pass a directory of .jpg files (the first 32 in name order are used, repeated if there are fewer) or one file.

    python tools/jpeg_cost.py FRAMES_DIR_OR_FILE [OUT.txt]
"""
import ctypes
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import _lib, jpeg          # noqa: E402

B = 32


def load(path):
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(('.jpg', '.jpeg')))
    else:
        files = [path]
    if not files:
        raise SystemExit('no .jpg files in %s' % path)
    return jpeg.read_files([files[i % len(files)] for i in range(B)])


def host_decode(datas, infos, threads):
    """Seconds of one entropy decode of the batch on `threads` threads (the foreign call releases the interpreter lock)."""
    lib = _lib.load()
    arrs = [np.frombuffer(d, np.uint8) for d in datas]
    bufs = [np.empty(i['coef_count'], np.int16) for i in infos]

    def one(b):
        assert lib.rtm3d_jpeg_entropy_decode(arrs[b].ctypes.data, arrs[b].size, bufs[b].ctypes.data, bufs[b].size) == 0

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(B)))                    # warm-up
        t0 = time.perf_counter()
        list(pool.map(one, range(B)))
        return time.perf_counter() - t0, bufs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if not args:
        raise SystemExit(__doc__)
    import torch
    datas = load(args[0])
    infos = [jpeg.info(d) for d in datas]
    stream_bytes = sum(len(d) for d in datas)
    coef_bytes = sum(i['coef_count'] for i in infos) * 2
    pixel_bytes = sum(i['h'] * i['w'] * 3 for i in infos)
    i0 = infos[0]
    lines = ['workload: %d frames, the first %d x %d %s (h x w), %.2f MB of streams, %.1f MB of coefficients, %.1f MB of packed pixels'
             % (B, i0['h'], i0['w'], i0['mode'], stream_bytes / 1e6, coef_bytes / 1e6, pixel_bytes / 1e6)]
    for threads in (1, 8):
        t, bufs = host_decode(datas, infos, threads)
        lines.append('host entropy decode, %d thread%s: %8.2f ms  %7.1f MB/s of stream  %7.0f frames/s'
                     % (threads, ' ' if threads == 1 else 's', t * 1e3, stream_bytes / t / 1e6, B / t))
    dev = torch.device('cuda', 0)
    # the device stage alone: coefficient buffers already on the device
    up = [(torch.from_numpy(b).to(dev), i['h'], i['w'], i['mode']) for b, i in zip(bufs, infos)]
    out = jpeg.idct(up)                                  # warm-up
    torch.cuda.synchronize()
    lib = _lib.load()
    frames, dst, stream = jpeg.c_frames(up), _lib.ptr_array(out), _lib.stream_ptr(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    busy = torch.randn(8192, 8192, device=dev, dtype=torch.float16)

    def device_time(fn):
        """Seconds between two events around fn(), enqueued behind a matrix product of about a millisecond so that the call waits
        in the queue and the time is the device's, not the host's."""
        torch.cuda.synchronize()
        torch.mm(busy, busy)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    device_time(lambda: None)                            # the product's own warm-up
    t = device_time(lambda: lib.rtm3d_frames_jpeg_idct(stream, B, frames, dst, 0))
    moved = coef_bytes + pixel_bytes
    lines.append('device stage, one chunk of %d frames (rtm3d_frames_jpeg_idct): %8.1f us  %.1f MB read + %.1f MB written = %.2f TB/s'
                 % (B, t * 1e6, coef_bytes / 1e6, pixel_bytes / 1e6, moved / t / 1e12))
    # the copy of the coefficients
    host = torch.empty(coef_bytes // 2, dtype=torch.int16).pin_memory()
    d_coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=dev)
    d_coef.copy_(host, non_blocking=True)
    t = device_time(lambda: d_coef.copy_(host, non_blocking=True))
    lines.append('copy of the coefficients, pinned host -> device: %8.1f us  %.1f GB/s' % (t * 1e6, coef_bytes / t / 1e9))
    # the whole chain
    for threads in (1, 8):
        for _ in range(2):                               # both staging sets warm
            jpeg.decode(datas, out=out, threads=threads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jpeg.decode(datas, out=out, threads=threads)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        lines.append('chain jpeg.decode, %d thread%s (streams -> packed frames, wall clock): %8.2f ms  %7.0f frames/s'
                     % (threads, ' ' if threads == 1 else 's', t * 1e3, B / t))
    try:
        import io
        from PIL import Image
        t0 = time.perf_counter()
        for d in datas:
            np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
        t = time.perf_counter() - t0
        lines.append('Pillow on one core, the same frames: %8.2f ms  %7.0f frames/s' % (t * 1e3, B / t))
    except ImportError:
        lines.append('Pillow on one core: unmeasured here (Pillow is not installed on this machine)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if len(args) > 1:
        with open(args[1], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
