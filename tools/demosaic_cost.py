"""Device time of rtm3d_frames_demosaic (the numbers of profiles/demosaic.txt): bs 32, 1080 x 1920 frames, every sample layout
at its least pitch rounded up to 256 bytes, both methods, to packed RGB; with and without a tone table and a colour matrix for
one layout; next to rtm3d_frames_convert of NV12 at the same size - the neighbouring stage - in the same session.  Two events
around CALLS back-to-back calls on the current stream, enqueued behind a matrix product of about a millisecond so that the calls
wait in the queue and the time between the events is the device's; the variants are interleaved over ROUNDS rounds after one
warm-up call each (the method of tools/frames_convert_cost.py).  The kernels are called through the C entry points with
prebuilt descriptors.

    python tools/demosaic_cost.py [OUT.txt]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import _lib, pixfmt, raw          # noqa: E402
from tools.frames_convert_cost import timed      # noqa: E402

B, H, W, ROUNDS, CALLS = 32, 1080, 1920, 5, 10
LAYOUTS = [('u8', 8), ('u16', 12), ('u16_msb', 16), ('mipi10', 10), ('mipi12', 12)]
CCM = [[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [-0.1, -0.7, 1.8]]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    dev = torch.device('cuda', 0)
    rng = np.random.Generator(np.random.PCG64(1))
    lib = _lib.load()
    packed = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(B)]
    dst = (ctypes.c_void_p * B)(*[p.data_ptr() for p in packed])
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    written = B * H * W * 3
    lines = ['workload: bs %d, %d x %d frames, planes at a pitch rounded up to 256 bytes, GRBG, black 64, gains (1.9, 1.0, 1.4), to packed '
             'R G B (%.1f MB written per batch)' % (B, H, W, written / 1e6)]
    tone = raw.tone_table('srgb').to(dev)
    variants, moved, keep = [], [], []
    for layout, bits in LAYOUTS:
        row, _ = raw.layout(layout, bits, H, W)
        pitch = (row + 255) // 256 * 256
        planes = [torch.from_numpy(rng.integers(0, 256, (H, pitch), dtype=np.uint8)).to(dev) for _ in range(B)]
        keep.append(planes)
        black = min(64, (1 << bits) - 1)
        for label, kw in (('', {}),) + ((('+ ccm + tone', {'ccm': CCM, 'tone': tone}),) if layout == 'mipi10' else ()):
            srcs = [raw.RawSource(p.reshape(-1), layout, 'grbg', bits=bits, size=(H, W), pitch=pitch, black=black, gains=(1.9, 1.0, 1.4), **kw)
                    for p in planes]
            arr = raw.c_sources(srcs)
            keep.append((srcs, arr))
            for method in ('mhc', 'bilinear'):
                mid = raw.METHODS[method]
                variants.append(('rtm3d_frames_demosaic %-7s %2d bit %-8s %s' % (layout, bits, method, label),
                                 lambda arr=arr, mid=mid: lib.rtm3d_frames_demosaic(stream, B, arr, dst, mid, 0)))
                moved.append(B * H * row + written)
    # the neighbouring stage at the same size
    cw, ch = (W + 1) // 2, (H + 1) // 2
    pitch = (max(W, 2 * cw) + 255) // 256 * 256
    surf = [torch.from_numpy(rng.integers(0, 256, (H + ch, pitch), dtype=np.uint8)).to(dev) for _ in range(B)]
    nv12 = [pixfmt.FrameSource.nv12(s[:H, :W], s[H:, :2 * cw]) for s in surf]
    narr = pixfmt.c_sources(nv12)
    variants.append(('rtm3d_frames_convert  NV12 -> RGB', lambda: lib.rtm3d_frames_convert(stream, B, narr, dst, 0)))
    moved.append(B * (H * W + ch * 2 * cw) + written)
    for _, fn in variants:
        assert fn() == 0, lib.rtm3d_last_error()
    torch.cuda.synchronize()
    times = timed(variants, ROUNDS, CALLS)
    for (name, _), t, nbytes in zip(variants, times, moved):
        lines.append('%-58s median %8.1f us  min %8.1f  max %8.1f  (per call; %d interleaved rounds x %d)  %6.1f MB moved, %5.2f TB/s'
                     % (name, np.median(t), np.min(t), np.max(t), ROUNDS, CALLS, nbytes / 1e6, nbytes / (np.median(t) * 1e-6) / 1e12))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args:
        with open(args[0], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
