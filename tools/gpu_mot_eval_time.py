"""Times of the tracking evaluation on one MI355X: a seeded synthetic split of KITTI-tracking size (tests/mot_eval_cases.scene,
seed 1: 21 sequences of 381 frames = 8001 frames, 15 objects per sequence), class Car, 3D IoU.
  * wall time of ``mot_eval.evaluate`` over the whole split, synchronised: median (min, max) of 5 after one warm-up run, and of
    its parts - ``prepare`` (host packing + the similarity launch) and ``run_device`` with HOTA only / CLEAR only;
  * hipEvent times of the device launches alone (rtm3d_mot_hota's four, rtm3d_mot_clear's one) on prepared device arrays;
  * wall time of the yardstick (tests/mot_eval_ref.py, margins off) on the same host's CPU, fed the device's similarities, and
    whether its counts equal the device's.
Prints the table; with an argument, also writes it to that file (profiles/mot_eval.txt holds its output, followed by the figures
tests/test_gpu_mot_eval.py prints)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import mot_eval
from tests import mot_eval_cases as mc
from tests import mot_eval_ref as ref

SEED, N_SEQ, N_FRAMES, N_OBJ, RUNS = 1, 21, 381, 15, 5
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def wall(fn, runs=RUNS):
    fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return r, float(np.median(out)), min(out), max(out)


dev = torch.device('cuda', 0)
gt, trk = mc.scene(SEED, n_seq=N_SEQ, n_frames=N_FRAMES, n_obj=N_OBJ)
log('tracking evaluation on %s' % torch.cuda.get_device_name(0))
res, med, lo, hi = wall(lambda: mot_eval.evaluate(gt, trk, classes=('Car',), metric='iou3d', device=dev))
p = mot_eval.prepare(gt, trk, 'Car', 'iou3d', True, dev)
log('synthetic split (scene seed %d): %d sequences, %d frames, %d ground truths (<= %d per frame), %d tracker boxes (<= %d per frame), '
    '%d / %d ids in the largest sequence' % (SEED, N_SEQ, len(p['ng']), int(p['ng'].sum()), int(p['ng'].max()), int(p['nt'].sum()),
                                             int(p['nt'].max()), int(p['gid'].max()) + 1, int(p['tid'].max()) + 1))
log('evaluate (Car, iou3d, KITTI preprocessing on), wall: median %.3f s (min %.3f, max %.3f) of %d after one warm-up run' % (med, lo, hi, RUNS))
log('  HOTA %.4f DetA %.4f AssA %.4f LocA %.4f | MOTA %.4f MOTP %.4f IDSW %d Frag %d' % tuple(
    [res.hota_mean['Car'][k] for k in ('HOTA', 'DetA', 'AssA', 'LocA')] + [res.clear['Car'][k] for k in ('MOTA', 'MOTP', 'IDSW', 'Frag')]))
_, med, lo, hi = wall(lambda: mot_eval.prepare(gt, trk, 'Car', 'iou3d', True, dev))
log('  of which prepare (host packing of the label rows, similarity, preprocessing ASSIGN): median %.3f s (min %.3f, max %.3f)' % (med, lo, hi))
args = (p['sim'], p['ng'], p['nt'], p['gid'], p['tid'], p['seq_start'])
_, med, lo, hi = wall(lambda: mot_eval.run_device(*args, clear=False))
log('  of which run_device, HOTA only (slot tables, uploads, 4 launches, fetch): median %.3f s (min %.3f, max %.3f)' % (med, lo, hi))
got, med, lo, hi = wall(lambda: mot_eval.run_device(*args, hota=False))
log('  of which run_device, CLEAR only (uploads, 1 launch, fetch): median %.3f s (min %.3f, max %.3f)' % (med, lo, hi))

# ---- the launches alone: hipEvent round the C call, every array already on the device
from rtm3d_amd import _lib, kitti_eval   # noqa: E402
lib = _lib.load()
F, cap_g, cap_t = p['sim'].shape
S = len(p['seq_start']) - 1
n_gid, n_tid = int(p['gid'].max()) + 1, int(p['tid'].max()) + 1
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                  # noqa: E731
d = {k: up(v) for k, v in dict(seq=p['seq_start'], ng=p['ng'], nt=p['nt'], gid=p['gid'], tid=p['tid'], gslot=mot_eval.slot_tables(p['gid'], p['ng'], n_gid),
                               tslot=mot_eval.slot_tables(p['tid'], p['nt'], n_tid)).items()}
z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)             # noqa: E731
ws = torch.empty(int(lib.rtm3d_mot_workspace_bytes(S, F, cap_g, cap_t, n_gid, n_tid)), dtype=torch.uint8, device=dev)
h = dict(potential=z(S, n_gid, n_tid, dt=torch.float64), gcount=z(S, n_gid), tcount=z(S, n_tid), match=z(F, cap_g), tp=z(S, 19), fn=z(S, 19),
         fp=z(S, 19), loc=z(S, 19, dt=torch.float64), mc=z(S, 19, n_gid, n_tid))
c = dict(match=z(F, cap_g), counts=z(S, 4), simsum=z(S, dt=torch.float64), idcount=z(S, n_gid), matched=z(S, n_gid), frag=z(S, n_gid))
stream = kitti_eval._stream(dev)


def hota():
    _lib.check(lib.rtm3d_mot_hota(stream, S, F, cap_g, cap_t, n_gid, n_tid, d['seq'].data_ptr(), d['ng'].data_ptr(), d['nt'].data_ptr(),
                                  d['gid'].data_ptr(), d['tid'].data_ptr(), d['gslot'].data_ptr(), d['tslot'].data_ptr(), p['sim'].data_ptr(),
                                  h['potential'].data_ptr(), h['gcount'].data_ptr(), h['tcount'].data_ptr(), h['match'].data_ptr(), h['tp'].data_ptr(),
                                  h['fn'].data_ptr(), h['fp'].data_ptr(), h['loc'].data_ptr(), h['mc'].data_ptr(), ws.data_ptr()), 'mot_hota')


def clear():
    _lib.check(lib.rtm3d_mot_clear(stream, S, F, cap_g, cap_t, n_gid, n_tid, d['seq'].data_ptr(), d['ng'].data_ptr(), d['nt'].data_ptr(),
                                   d['gid'].data_ptr(), d['tid'].data_ptr(), p['sim'].data_ptr(), 0.5, c['match'].data_ptr(), c['counts'].data_ptr(),
                                   c['simsum'].data_ptr(), c['idcount'].data_ptr(), c['matched'].data_ptr(), c['frag'].data_ptr(), ws.data_ptr()),
               'mot_clear')


def events(fn, groups=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    out = []
    for _ in range(groups):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out)), float(np.min(out))


log('the launches alone, us per call: median (min) of 10 calls after 3, hipEvent (ctypes call included)')
t = events(hota)
log('  rtm3d_mot_hota  (sums, alignment walk over %d x %d pairs x %d sequences, %d match waves, loc): %9.1f (%.1f)' % (n_gid, n_tid, S, F, t[0], t[1]))
t = events(clear)
log('  rtm3d_mot_clear (%d waves, each walking ~%d frames in order): %9.1f (%.1f)' % (S, N_FRAMES, t[0], t[1]))

# ---- the yardstick on the same host's CPU, the device's similarities
a = dict(p, sim=p['sim'].cpu().numpy())
t0 = time.perf_counter()
hr = ref.hota(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], with_margin=False)
t1 = time.perf_counter()
cr = ref.clear(a['sim'], a['ng'], a['nt'], a['gid'], a['tid'], a['seq_start'], 0.5, with_margin=False)
t2 = time.perf_counter()
full = mot_eval.run_device(*args)
same = all(np.array_equal(full[k], dict(hr, **cr)[k]) for k in ('match', 'tp', 'fn', 'fp', 'mc', 'gcount', 'tcount', 'clear_match', 'counts', 'idcount',
                                                                'matched', 'frag'))
worst = max(float(np.abs(full[k] - dict(hr, **cr)[k]).max()) for k in ('potential', 'loc', 'simsum'))
log('yardstick (tests/mot_eval_ref.py, numpy loops + scipy, margins off) on this host, similarities given: HOTA %.1f s, CLEAR %.1f s; integer '
    'outputs equal to the device: %s; largest disagreement of potential / loc / simsum: %.3g' % (t1 - t0, t2 - t1, same, worst))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
