"""Device time of rtm3d_frames_convert (the numbers of profiles/frames_convert.txt): bs 32, 375 x 1242 frames as NV12, P010,
YUYV and BGRA surfaces at a pitch rounded up to 256 bytes, each to packed RGB, next to the same conversion composed from
torch ops (what a Python caller had to write before), and the detect_frames step of a DLA-34 engine (384 x 1280 canvas,
synthetic weights) with and without the conversion in front.  Two events around CALLS back-to-back calls on the current
stream, enqueued behind a matrix product of about a millisecond so that the calls wait in the queue and the time between the
events is the device's; the variants are interleaved over ROUNDS rounds after one warm-up call each.  The kernel is called
through the C entry point with prebuilt descriptors (what a C caller pays); the torch compositions are some 500 small launches
per batch and stay bound by their enqueue whatever stands in front.  They are checked against the kernel (BGRA: equal; the
float composition of the YUV formats: within 1).

    python tools/frames_convert_cost.py [OUT.txt] [--no-step]
"""
import ctypes
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtm3d_amd                                 # noqa: E402
from rtm3d_amd import _lib, engine, pixfmt, weights    # noqa: E402

B, H, W, ROUNDS, CALLS = 32, 375, 1242, 5, 10
CW, CH = (W + 1) // 2, (H + 1) // 2


def pitched(rows, row_bytes, dev, rng):
    pitch = (row_bytes + 255) // 256 * 256
    return torch.from_numpy(rng.integers(0, 256, (rows, pitch), dtype=np.uint8)).to(dev), pitch


def sources(dev):
    """name -> (list of FrameSource, bytes read per batch, torch composition)"""
    rng = np.random.Generator(np.random.PCG64(1))
    out = {}
    cy, crv, cgu, cgv, cbu = [c / 65536.0 for c in pixfmt.yuv_coefficients('nv12')[0]]

    def yuv_float(Y, U, V, yo, co, scale):
        Y, U, V = (Y.float() - yo) * (cy * scale), U.float() - co, V.float() - co
        rgb = torch.stack([Y + crv * scale * V, Y + cgu * scale * U + cgv * scale * V, Y + cbu * scale * U], -1)
        return (rgb + 0.5).floor().clamp(0, 255).to(torch.uint8)

    surf = [pitched(H + CH, max(W, 2 * CW), dev, rng) for _ in range(B)]
    out['NV12'] = ([pixfmt.FrameSource.nv12(s[:H, :W], s[H:, :2 * CW]) for s, _ in surf], B * (H * W + CH * 2 * CW),
                   lambda: [yuv_float(s[:H, :W], s[H:, :2 * CW:2].repeat_interleave(2, 0).repeat_interleave(2, 1)[:H, :W],
                                      s[H:, 1:2 * CW:2].repeat_interleave(2, 0).repeat_interleave(2, 1)[:H, :W], 16, 128, 1.0) for s, _ in surf])
    surf16 = [pitched(H + CH, 2 * max(W, 2 * CW), dev, rng) for _ in range(B)]
    v16 = [s.view(torch.int16) for s, _ in surf16]                          # little-endian samples; >> 6 of the unsigned value below
    u10 = lambda t: (t.int() & 0xffff) >> 6
    out['P010'] = ([pixfmt.FrameSource.p010(s[:H, :2 * W], s[H:, :4 * CW]) for s, _ in surf16], B * 2 * (H * W + CH * 2 * CW),
                   lambda: [yuv_float(u10(v[:H, :W]), u10(v[H:, :2 * CW:2]).repeat_interleave(2, 0).repeat_interleave(2, 1)[:H, :W],
                                      u10(v[H:, 1:2 * CW:2]).repeat_interleave(2, 0).repeat_interleave(2, 1)[:H, :W], 64, 512, 0.25) for v in v16])
    surfy = [pitched(H, 4 * CW, dev, rng) for _ in range(B)]
    out['YUYV'] = ([pixfmt.FrameSource.yuyv(s[:, :4 * CW], size=(H, W)) for s, _ in surfy], B * H * 4 * CW,
                   lambda: [yuv_float(s[:, 0:4 * CW:2][:, :W], s[:, 1:4 * CW:4].repeat_interleave(2, 1)[:, :W],
                                      s[:, 3:4 * CW:4].repeat_interleave(2, 1)[:, :W], 16, 128, 1.0) for s, _ in surfy])
    surfb = [pitched(H, 4 * W, dev, rng) for _ in range(B)]
    out['BGRA'] = ([pixfmt.FrameSource.packed(s[:, :4 * W].view(H, W, 4), 'bgra') for s, _ in surfb], B * H * W * 4,
                   lambda: [s[:, :4 * W].view(H, W, 4)[:, :, [2, 1, 0]].contiguous() for s, _ in surfb])
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
    dev = torch.device('cuda', 0)
    src = sources(dev)
    packed = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(B)]
    lines = ['workload: bs %d, %d x %d frames, surfaces at a pitch rounded up to 256 bytes, to packed R G B (%.1f MB written per batch)'
             % (B, H, W, B * H * W * 3 / 1e6)]
    variants = []
    lib = _lib.load()
    dst = (ctypes.c_void_p * B)(*[p.data_ptr() for p in packed])
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for name, (s, nread, compose) in src.items():
        got = [t.clone() for t in pixfmt.convert(s, 'rgb', out=packed)]
        d = max(int((a.int() - b.int()).abs().max()) for a, b in zip(got, compose()))
        assert d <= (0 if name == 'BGRA' else 1), (name, d)
        lines.append('check %s: the torch composition differs from the kernel by at most %d' % (name, d))
        arr = pixfmt.c_sources(s)
        variants.append(('rtm3d_frames_convert %s -> RGB' % name, lambda arr=arr: lib.rtm3d_frames_convert(stream, B, arr, dst, 0)))
        variants.append(('torch ops            %s -> RGB' % name, compose))
    times = timed(variants, ROUNDS, CALLS)
    for (name, _), t, nbytes in zip(variants, times, [n for _, (_, n, _) in src.items() for _ in range(2)]):
        moved = nbytes + B * H * W * 3
        extra = '  %6.1f MB moved, %5.2f TB/s' % (moved / 1e6, moved / (np.median(t) * 1e-6) / 1e12) if name.startswith('rtm3d') else ''
        lines.append('%-36s median %8.1f us  min %8.1f  max %8.1f  (per call; %d interleaved rounds x %d)%s'
                     % (name, np.median(t), np.min(t), np.max(t), ROUNDS, CALLS, extra))
    if '--no-step' not in sys.argv:
        cfg = rtm3d_amd.kitti_config('DLA-34')
        m = rtm3d_amd.create_model(cfg).to(dev).eval()
        m.load_state_dict(weights.synth_state_dict('DLA-34', 1, 'trained', heat_bias=-3.0))
        path = os.path.join(tempfile.mkdtemp(), 'dla34_bs32.rtm3d')
        m.save_engine(path, B, 384, 1280)
        eng = engine.Engine(path, dev)
        eng.set_frame_params(cfg.DATASET.MEAN, cfg.DATASET.STD, None)
        K = torch.as_tensor(np.tile(weights.synth_intrinsics(), (B, 1)), device=dev)
        nv12 = src['NV12'][0]
        pixfmt.convert(nv12, 'rgb', out=packed)
        rec = torch.empty(B, eng.info['topk'], 32, dtype=torch.float32, device=dev)
        step = [('detect_frames on packed frames', lambda: eng.detect_frames(packed, K, out=rec)),
                ('detect_frames_src on NV12 surfaces', lambda: eng.detect_frames_src(nv12, K, packed=packed, out=rec))]
        t = timed(step, ROUNDS, 5)
        for (name, _), v in zip(step, t):
            lines.append('%-36s median %8.3f ms  min %8.3f  max %8.3f  (DLA-34 engine, bs %d, 384 x 1280 canvas, synthetic weights; %d '
                         'interleaved rounds x 5)' % (name, np.median(v) / 1e3, np.min(v) / 1e3, np.max(v) / 1e3, B, ROUNDS))
        lines.append('difference of the medians: %.1f us' % (np.median(t[1]) - np.median(t[0])))
        eng.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args:
        with open(args[0], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
