"""Device time of rtm3d_frames_remap and rtm3d_lens_map_build (the numbers of profiles/lens.txt): bs 32 of 375 x 1242 and of
1080 x 1920 frames, each through a Brown map of its own size (one map shared by the batch, and one map per frame), plus the
identity map as the coherent limit and the build of the 32 maps.  hipEvents around CALLS back-to-back calls on the current
stream, enqueued behind a matrix product of about a millisecond so that the calls wait in the queue and the time between the
events is the device's; the variants are interleaved over ROUNDS rounds after one warm-up call each (ROUNDS x CALLS >= 20
timed repeats).  The kernels are called through the C entry points with prebuilt descriptors.  Bytes moved: 8 B of map read
and 3 B written per destination pixel, 3 B per pixel the four samples of a destination pixel bring in when neighbours share
them (14 B per destination pixel), and beside it the source bytes actually touched: the union of the 2 x 2 neighbourhoods,
counted from the map.  The remap is checked against torch's own gather arithmetic on the first frame before it is timed.

    python tools/gpu_lens_bench.py [OUT.txt]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import _lib, lens    # noqa: E402

B, ROUNDS, CALLS = 32, 5, 10
SIZES = [(375, 1242), (1080, 1920)]
DIST = [-0.28, 0.07, 1.5e-3, -2.5e-3, -0.011]


def model_for(h, w):
    f = 0.58 * w                                                  # a horizontal field of view of about 80 degrees
    return lens.LensModel.brown([f, 0, (w - 1) / 2 + 3.25, 0, f, (h - 1) / 2 - 2.5, 0, 0, 1], DIST, (h, w))


def remap_torch(src, m, fill=0):
    """The header's rule in torch int64 ops (one frame): the check of what is timed."""
    h, w = src.shape[:2]
    m = m.long()
    sx, sy = m[..., 0], m[..., 1]
    ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31
    flat = src.reshape(-1, 3).long()

    def S(i, j):
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        v = flat[(j.clamp(0, h - 1) * w + i.clamp(0, w - 1)).reshape(-1)].reshape(i.shape + (3,))
        return torch.where(inside[..., None], v, torch.full_like(v, fill))

    a, b = ax[..., None], ay[..., None]
    out = ((32 - a) * (32 - b) * S(ix, iy) + a * (32 - b) * S(ix + 1, iy) + (32 - a) * b * S(ix, iy + 1) + a * b * S(ix + 1, iy + 1) + 512) >> 10
    return torch.where((sx == lens.OUTSIDE)[..., None], torch.full_like(out, fill), out).to(torch.uint8)


def touched_bytes(m, h, w):
    """Bytes of an h x w source inside the union of the 2 x 2 neighbourhoods of a map."""
    m = m.long().reshape(-1, 2)
    m = m[m[:, 0] != lens.OUTSIDE]
    hit = torch.zeros(h * w, dtype=torch.bool, device=m.device)
    ix, iy = m[:, 0] >> 5, m[:, 1] >> 5
    for dx in (0, 1):
        for dy in (0, 1):
            i, j = ix + dx, iy + dy
            ok = (i >= 0) & (i < w) & (j >= 0) & (j < h)
            hit[(j[ok] * w + i[ok])] = True
    return 3 * int(hit.sum())


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
    fill = lens.c_fill((0, 0, 0))
    rng = np.random.Generator(np.random.PCG64(1))
    lines, variants, moved, keep = [], [], [], []
    for h, w in SIZES:
        frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
        out = [torch.empty(h, w, 3, dtype=torch.uint8, device=dev) for _ in range(B)]
        models = [model_for(h, w)] * B
        own = lens.build_maps(models, device=dev)                              # 32 maps of 8 B per pixel: a map per frame
        v, u = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
        ident = lens.LensMap(torch.stack([32 * u, 32 * v], -1).int().contiguous())
        got = lens.remap(frames[:1], own[:1], out=out[:1])[0]
        assert torch.equal(got, remap_torch(frames[0], own[0].tensor)), 'the kernel disagrees with the rule in torch ops'
        n_out = int((own[0].tensor[..., 0] == lens.OUTSIDE).sum())
        touch = touched_bytes(own[0].tensor, h, w)
        lines.append('%d x %d: Brown map k1 k2 p1 p2 k3 = %s, f = %.1f; %d of %d entries outside, the map touches %.2f of the %.2f MB of a '
                     'source frame' % (h, w, DIST, models[0].K[0], n_out, h * w, touch / 1e6, h * w * 3 / 1e6))
        src = (ctypes.c_void_p * B)(*[f.data_ptr() for f in frames])
        dst = (ctypes.c_void_p * B)(*[o.data_ptr() for o in out])
        hw = (ctypes.c_int * (2 * B))(*([h, w] * B))
        for name, maps, map_bytes, src_bytes in (('Brown, one map shared', [own[0]] * B, h * w * 8, B * touch),
                                                 ('Brown, a map per frame', own, B * h * w * 8, B * touch),
                                                 ('identity, one map shared', [ident] * B, h * w * 8, B * h * w * 3)):
            cm = lens.c_maps(maps)
            keep.append((cm, maps))
            variants.append(('remap %4d x %4d  %-24s' % (h, w, name),
                             lambda cm=cm, src=src, dst=dst, hw=hw: lib.rtm3d_frames_remap(stream, B, src, hw, cm, dst, fill)))
            # nominal: 14 B per destination pixel; distinct: what has to come from memory at least once
            moved.append((B * h * w * 14, map_bytes + src_bytes + B * h * w * 3))
        cmod, crect = (_lib.LensModelC * B)(), (_lib.LensRectC * B)()
        for i, mod in enumerate(models):
            cmod[i] = mod.c_struct()
            crect[i] = _lib.LensRectC(h, w, (ctypes.c_double * 9)(*mod.K), (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1))
        ptrs = (ctypes.c_void_p * B)(*[m.tensor.data_ptr() for m in own])
        keep.append((frames, out, own, cmod, crect, ptrs, src, dst, hw))
        variants.append(('build %4d x %4d  32 Brown maps            ' % (h, w),
                         lambda cmod=cmod, crect=crect, ptrs=ptrs: lib.rtm3d_lens_map_build(stream, B, cmod, crect, ptrs)))
        moved.append((B * h * w * 8, B * h * w * 8))
    times = timed(variants, ROUNDS, CALLS)
    lines.append('per call of bs %d; %d interleaved rounds x %d calls; nominal = 14 B per destination pixel (build: the 8 B written), '
                 'distinct = map + touched source + output bytes once each' % (B, ROUNDS, CALLS))
    for (name, _), t, (nominal, distinct) in zip(variants, times, moved):
        med = np.median(t)
        lines.append('%s median %8.1f us  min %8.1f  max %8.1f   nominal %7.1f MB %5.2f TB/s   distinct %7.1f MB %5.2f TB/s'
                     % (name, med, np.min(t), np.max(t), nominal / 1e6, nominal / (med * 1e-6) / 1e12, distinct / 1e6,
                        distinct / (med * 1e-6) / 1e12))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args:
        with open(args[0], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
