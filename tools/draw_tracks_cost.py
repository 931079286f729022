"""Device time of rtm3d_records_draw_tracks next to rtm3d_records_draw on the workload of profiles/draw.txt (the numbers of
profiles/draw_tracks.txt): bs 32, 375 x 1242 frames, 100 slots per frame - the twelve planted kept cuboids of tests/draw_cases.py
and 88 random flag-1 cuboids - 400 x 400 panels.  Two events around CALLS back-to-back calls on the current stream, behind one
untimed call (the queue never drains, so the time is the device's); the variants are interleaved over ROUNDS rounds after one
warm-up call each.

    python tools/draw_tracks_cost.py [OUT.txt]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import draw as rdraw, track     # noqa: E402
from tests import draw_cases as dc             # noqa: E402

B, TOPK, T, ROUNDS, CALLS = 32, 100, 128, 5, 10


def workload(dev):
    k = [c for c in dc.cases() if c['name'] == 'kitti_source0'][0]
    rng = np.random.Generator(np.random.PCG64(5))
    rec = np.zeros((TOPK, 32), np.float32)
    rec[:12] = k['rec'][0, :12]
    for s in range(12, TOPK):
        x, y = rng.uniform(40, 1200), rng.uniform(40, 340)
        sx, sy = rng.uniform(15, 60), rng.uniform(10, 40)
        rec[s] = dc.record(s % 3, (x, y), dc.cuboid(x, y, sx, sy, rng.uniform(-20, 20), rng.uniform(-12, 12)), (x - sx - 5, y - sy - 5, x + sx + 5, y + sy + 5), 1,
                           score=rng.uniform(0.3, 0.9))
    rec = np.tile(rec[None], (B, 1, 1))
    ids = np.zeros((B, TOPK), np.int32)
    ids[:, :12] = np.arange(1, 13)
    ids[:, 5] = -6
    frames = [torch.from_numpy(rng.integers(0, 256, (375, 1242, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
    trk = track.Tracker(B, T, None, dev)
    state = np.zeros((B, 8 + 24 * T))
    for t in range(12):                          # the kept boxes as live tracks, every fourth coasting
        s = state[:, 8 + 24 * t:8 + 24 * (t + 1)]
        s[:, 0], s[:, 2], s[:, 3], s[:, 4], s[:, 6] = t + 1, 4, 0 if t % 4 == 3 else 3, 1 if t % 4 == 3 else 0, -1 if t % 4 == 3 else t
        s[:, 7:14] = rec[0, t, 24:31]
        s[:, 14], s[:, 16] = 0.5, -1.0
    trk.state.copy_(torch.from_numpy(state))
    return frames, torch.from_numpy(rec).to(dev), torch.from_numpy(ids).to(dev), torch.as_tensor(np.tile(k['K'], (B, 1)), device=dev), trk


def main():
    dev = torch.device('cuda', 0)
    frames, rec, ids, K, trk = workload(dev)
    panels = torch.zeros(B, 400, 400, 3, dtype=torch.uint8, device=dev)
    base = dict(layers=rdraw.FRAME_LAYERS | rdraw.BEV, bev_hw=(400, 400), bev_m_per_px=0.2)
    tb = dict(base, layers=rdraw.FRAME_LAYERS | rdraw.LABEL | rdraw.TRACK_BEV)
    variants = [
        ('rtm3d_records_draw, all layers + panel', lambda: rdraw.draw_records(frames, rec, K, rdraw.DrawParams(**base), panels, check_classes=False)),
        ('draw_tracks, id colours, no label layer', lambda: rdraw.draw_tracks(frames, rec, ids, K, rdraw.TrackDrawParams(**base), None, panels, check_classes=False)),
        ('draw_tracks, id colours + labels (id class)', lambda: rdraw.draw_tracks(
            frames, rec, ids, K, rdraw.TrackDrawParams(**dict(base, layers=base['layers'] | rdraw.LABEL)), None, panels, check_classes=False)),
        ('draw_tracks, labels, all four fields', lambda: rdraw.draw_tracks(
            frames, rec, ids, K, rdraw.TrackDrawParams(label_fields=15, **dict(base, layers=base['layers'] | rdraw.LABEL)), None, panels, check_classes=False)),
        ('draw_tracks, labels + track panel, bev_fade 256', lambda: rdraw.draw_tracks(frames, rec, ids, K, rdraw.TrackDrawParams(**tb), trk, panels,
                                                                                      check_classes=False)),
        ('draw_tracks, labels + track panel, bev_fade 200', lambda: rdraw.draw_tracks(frames, rec, ids, K, rdraw.TrackDrawParams(bev_fade=200, **tb), trk,
                                                                                      panels, check_classes=False)),
    ]
    times = [[] for _ in variants]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for i, (_, fn) in enumerate(variants):
            fn()                                 # keeps the queue busy, so the host side of the timed calls hides behind the device
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) * 1e3 / CALLS)
    lines = ['workload: bs %d, 375 x 1242 frames, %d slots per frame, 12 kept (ids 1..12, one tentative), thickness 1, radius 5, 400 x 400 panels at '
             '0.2 m/px, %d track slots (12 live, 3 coasting)' % (B, TOPK, T)]
    ref_t = float(np.median(times[0]))
    for (name, _), t in zip(variants, times):
        lines.append('%-52s median %7.1f us  min %7.1f  max %7.1f  x %.2f  (per call; %d interleaved rounds of %d calls)'
                     % (name, np.median(t), np.min(t), np.max(t), np.median(t) / ref_t, ROUNDS, CALLS))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
