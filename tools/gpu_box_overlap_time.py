"""hipEvent times of the box-overlap kernels on one MI355X: rtm3d_records_nms3d at B = 32, topk = 100 with 10 and with all 100
kept (flag 2) slots per image, rtm3d_box_overlaps at B = 32, 100 x 100.  Median of 20 timed groups of 10 launches after a
warm-up; the NMS input is restored between groups outside the timed region (the call works in place).
Prints the table; with an argument, also writes it to that file (profiles/box_overlap.txt holds its output)."""
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import box_overlap

B, TOPK, GROUPS, PER = 32, 100, 20, 10
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def boxes(rng, n):
    """n boxes in clusters of about five around car-sized sites 9 m apart."""
    site = rng.integers(max(1, n // 5), size=n)
    b = np.empty((n, 7))
    b[:, 0:3] = rng.uniform(0.9, 1.1, (n, 3)) * np.array([1.6, 1.8, 4.0])
    b[:, 3] = (site % 6) * 9.0 - 22.0 + rng.uniform(-0.8, 0.8, n)
    b[:, 4] = rng.uniform(0.8, 1.2, n)
    b[:, 5] = (site // 6) * 9.0 + 8.0 + rng.uniform(-0.8, 0.8, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def timed(fn, reset=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    out = []
    for _ in range(GROUPS):
        if reset is not None:
            reset()
        e0.record()
        for _ in range(PER):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / PER)
    return float(np.median(out)), float(np.min(out))


dev = torch.device('cuda', 0)
rng = np.random.Generator(np.random.PCG64(1))
try:
    commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=os.path.dirname(os.path.abspath(__file__)),
                                     stderr=subprocess.DEVNULL).decode().strip()
except Exception:
    commit = 'unknown'
log('box overlap kernels on %s (tree on top of commit %s)' % (torch.cuda.get_device_name(0), commit))
log('us per launch: median (min) of %d groups of %d back-to-back launches, hipEvent' % (GROUPS, PER))
for kept in (10, TOPK):
    rec = np.zeros((B, TOPK, 32), np.float32)
    for b in range(B):
        rec[b, :, 24:31] = boxes(rng, TOPK)
        rec[b, :, 0] = rng.integers(3, size=TOPK)
        rec[b, :, 31] = 1.0
        rec[b, rng.permutation(TOPK)[:kept], 31] = 2.0
    src = torch.from_numpy(rec).to(dev)
    work = src.clone()
    for metric in ('bev', '3d'):
        # the first launch of a group does the suppression, the other nine see its survivors: time both kinds
        first = timed(lambda: (work.copy_(src), box_overlap.nms3d_records(work, 0.5, metric=metric)))
        copy = timed(lambda: work.copy_(src))
        again = timed(lambda: box_overlap.nms3d_records(work, 0.5, metric=metric), reset=lambda: work.copy_(src))
        left = int((work[..., 31] == 2).sum())
        log('records_nms3d B=%d topk=%d, %3d kept per image, %s IoU 0.5: %7.1f (%.1f) with the restoring copy, copy alone %5.1f (%.1f), '
            'mostly on survivors %7.1f (%.1f); %d of %d survive' % (B, TOPK, kept, metric, first[0], first[1], copy[0], copy[1], again[0], again[1],
                                                                   left, B * kept))
a = torch.from_numpy(np.stack([boxes(rng, 100) for _ in range(B)])).to(dev)
b = torch.from_numpy(np.stack([boxes(rng, 100) for _ in range(B)])).to(dev)
t = timed(lambda: box_overlap.overlaps(a, b))
bev, _ = box_overlap.overlaps(a, b)
log('box_overlaps  B=%d 100 x 100 (iou, both outputs; includes the two torch.empty and the counts fill of the Python wrapper): %7.1f (%.1f); '
    '%d of %d pairs overlap' % (B, t[0], t[1], int((bev > 0).sum()), bev.numel()))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
