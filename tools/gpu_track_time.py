"""hipEvent times of rtm3d_tracks_update on one MI355X at B = 32, topk = 100, T = 128 with 10 and with 100 detections per frame,
for each metric, in the steady state (the same frame fed again and again: every track is matched in every call), through the C
entry point with preallocated buffers; the 3D NMS of the same records (rtm3d_records_nms3d on its own survivors) next to it for
scale.  Median of 20 timed groups of 10 calls after a warm-up.
Every configuration is timed under both association rules in the same run: the greedy match through rtm3d_tracks_update, then
the optimal assignment through rtm3d_tracks_update_assign on the same records, with the ratio of the two.  One adversarial row
follows: the 40-chain of tests/track_assign_ref.py (every detection between two tracks, the record slots in reversed x order,
T = 64, topk = 48) on 32 streams, the frame after the births, where the augmenting paths are long; its table is put back before
every call (outside the timed span), so each call is timed alone between two events.
Prints the table; with an argument, also appends it to that file (profiles/track.txt holds its output)."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import _lib, box_overlap, track
from tests import track_assign_ref as ar

B, TOPK, T, GROUPS, PER = 32, 100, 128, 20, 10
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def boxes(rng, n):
    """n boxes in clusters of about five around car-sized sites 9 m apart (tools/gpu_box_overlap_time.py)."""
    site = rng.integers(max(1, n // 5), size=n)
    b = np.empty((n, 7))
    b[:, 0:3] = rng.uniform(0.9, 1.1, (n, 3)) * np.array([1.6, 1.8, 4.0])
    b[:, 3] = (site % 6) * 9.0 - 22.0 + rng.uniform(-0.8, 0.8, n)
    b[:, 4] = rng.uniform(0.8, 1.2, n)
    b[:, 5] = (site // 6) * 9.0 + 8.0 + rng.uniform(-0.8, 0.8, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    out = []
    for _ in range(GROUPS):
        e0.record()
        for _ in range(PER):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / PER)
    return float(np.median(out)), float(np.min(out))


dev = torch.device('cuda', 0)
lib = _lib.load()
rng = np.random.Generator(np.random.PCG64(1))
log('tracking kernels on %s' % torch.cuda.get_device_name(0))
log('us per call (two launches): median (min) of %d groups of %d back-to-back calls, hipEvent' % (GROUPS, PER))
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
def update_call(assign, b, topk, t, d_rec, p, state, ids, ws):
    """assign None: rtm3d_tracks_update; 0 / 1: rtm3d_tracks_update_assign."""
    if assign is None:
        return lambda: _lib.check(lib.rtm3d_tracks_update(stream, b, topk, t, d_rec.data_ptr(), 1.0, None, ctypes.byref(p), state.data_ptr(),
                                                          ids.data_ptr(), ws.data_ptr()), 'tracks_update')
    return lambda: _lib.check(lib.rtm3d_tracks_update_assign(stream, b, topk, t, d_rec.data_ptr(), 1.0, None, ctypes.byref(p), assign,
                                                             state.data_ptr(), ids.data_ptr(), ws.data_ptr()), 'tracks_update')


def timed_alone(fn, before):
    """Each call between its own two events, `before` run ahead of it outside the timed span."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for n in range(5 + GROUPS):
        acc = 0.0
        for _ in range(PER):
            before()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc += e0.elapsed_time(e1) * 1e3
        if n >= 5:
            out.append(acc / PER)
    return float(np.median(out)), float(np.min(out))


for kept in (10, TOPK):
    rec = np.zeros((B, TOPK, 32), np.float32)
    for b in range(B):
        rec[b, :, 24:31] = boxes(rng, TOPK)
        rec[b, :, 0] = rng.integers(3, size=TOPK)
        rec[b, :, 1] = np.sort(rng.uniform(0.3, 0.99, TOPK))[::-1]
        rec[b, :, 31] = 1.0
        rec[b, rng.permutation(TOPK)[:kept], 31] = 2.0
    d_rec = torch.from_numpy(rec).to(dev)
    for metric, thresh in (('bev', 0.01), ('3d', 0.01), ('dist', -2.0)):
        greedy_us = None
        for rule, assign in (('greedy', None), ('optimal', 1)):
            trk = track.Tracker(B, T, track.TrackParams(metric=metric, thresh=thresh), dev)
            p = trk.params.to_c()
            ids = torch.empty(B, TOPK, dtype=torch.int32, device=dev)
            ws = torch.empty(int(lib.rtm3d_tracks_workspace_bytes(B, TOPK, T)), dtype=torch.uint8, device=dev)
            t = timed(update_call(assign, B, TOPK, T, d_rec, p, trk.state, ids, ws))
            tab = trk.tracks()
            tail = '%d live tracks, %d ids issued, %d slots tracked' % (int(tab['live'].sum()), int(tab['issued'].sum()), int((ids != 0).sum()))
            if assign is None:
                greedy_us = t[0]
                log('tracks_update B=%d topk=%d T=%d, %3d detections per frame, %-4s: %7.1f (%.1f); %s' % (B, TOPK, T, kept, metric, t[0], t[1], tail))
            else:
                log('  assign=optimal, the same records             %-4s: %7.1f (%.1f); %.2f x greedy; %s' % (metric, t[0], t[1], t[0] / greedy_us, tail))
    work = d_rec.clone()
    box_overlap.nms3d_records(work, 0.5, metric='3d')
    n = timed(lambda: box_overlap.nms3d_records(work, 0.5, metric='3d'))
    log('records_nms3d B=%d topk=%d, %3d kept per image, 3d IoU 0.5, on its own survivors (for scale): %7.1f (%.1f)' % (B, TOPK, kept, n[0], n[1]))

# the adversarial row: the chain, reversed slot order, on every stream; the frame after the births
chain = ar.chain_dist()
CT, CK = chain['T'], chain['topk']
frames = [torch.from_numpy(np.ascontiguousarray(np.repeat(f[1:2], B, axis=0))).to(dev) for f in chain['frames']]
greedy_us = None
for rule, assign in (('greedy', None), ('optimal', 1)):
    trk = track.Tracker(B, CT, track.TrackParams(**chain['params']), dev, assignment=rule)
    trk.update(frames[0])
    saved = trk.state.clone()
    p = trk.params.to_c()
    ids = torch.empty(B, CK, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.rtm3d_tracks_workspace_bytes(B, CK, CT)), dtype=torch.uint8, device=dev)
    t = timed_alone(update_call(assign, B, CK, CT, frames[1], p, trk.state, ids, ws), lambda: trk.state.copy_(saved))
    tab = trk.tracks()
    tail = '%d live tracks, %d ids issued' % (int(tab['live'].sum()), int(tab['issued'].sum()))
    if assign is None:
        greedy_us = t[0]
        log('40-chain, reversed slots, B=%d topk=%d T=%d, dist, each call alone between two events, greedy : %7.1f (%.1f); %s' % (B, CK, CT, t[0], t[1], tail))
    else:
        log('40-chain, reversed slots, B=%d topk=%d T=%d, dist, each call alone between two events, optimal: %7.1f (%.1f); %.2f x greedy; %s'
            % (B, CK, CT, t[0], t[1], t[0] / greedy_us, tail))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'a') as f:
        f.write('\n'.join(lines) + '\n')
