"""Engine files against the Python path, DLA-34 bs=32 384x1280 on one MI355X: cold start (create_model + load_state_dict + first
plan build against rtm3d_engine_load) and per-step time of rtm3d_engine_detect against the same non-pipelined Python step.
Prints the table; with an argument, also writes it to that file (profiles/r08_engine.txt holds its output)."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtm3d_amd
from rtm3d_amd import engine, weights, distributed as rdist
from rtm3d_amd.model import Detections
from rtm3d_amd.model_utils import Boxes3D, decode3d_slots

B, H, W, bb = 32, 384, 1280, 'DLA-34'
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


dev = torch.device('cuda', 0)
torch.zeros(1, device=dev)
torch.cuda.synchronize()
sd = weights.synth_state_dict(bb, 1, 'trained', heat_bias=-3.0)
cfg = rtm3d_amd.kitti_config(bb)
workdir = tempfile.mkdtemp()
path = os.path.join(workdir, 'dla34_b32.rtm3d')
t = time.perf_counter()
m0 = rtm3d_amd.create_model(cfg)
m0.load_state_dict(sd)
m0.save_engine(path, B, H, W)
log('export (create_model + load_state_dict + save_engine, no GPU work): %.2f s, %.1f MB' % (time.perf_counter() - t, os.path.getsize(path) / 1e6))
del m0

for rep in range(2):
    torch.cuda.synchronize()
    t = time.perf_counter()
    m = rtm3d_amd.create_model(cfg).to(dev).eval()
    m.load_state_dict(sd)
    m._plan_for(B, H, W, dev)
    torch.cuda.synchronize()
    tp = time.perf_counter() - t
    m._drop_plans()
    del m
    torch.cuda.synchronize()
    t = time.perf_counter()
    eng = engine.Engine(path, dev)
    torch.cuda.synchronize()
    te = time.perf_counter() - t
    eng.close()
    del eng
    log('cold start %d: python create_model + load_state_dict + first plan build %.3f s | rtm3d_engine_load (+ workspace) %.3f s' % (rep, tp, te))

x = weights.synth_images(B, H, W, seed=7).to(dev)
K = torch.as_tensor(np.tile(weights.synth_intrinsics(), (B, 1)), device=dev)
m = rtm3d_amd.create_model(cfg).to(dev).eval()
m.load_state_dict(sd)
det, boxes = Detections(B, 100, dev), Boxes3D(B * 100, dev)
rec_py = torch.empty(B, 100, 32, device=dev)


def py_step():
    lg = m.forward_logits(x, out='reuse')
    m.decode2d(lg, out=det)
    decode3d_slots(det, K, cfg.DETECTOR.dim_ref, (0.0, -0.5, 20.0), out=boxes)
    rdist.pack_records(det.n, det.cls, det.score, det.mproj, det.verts, det.bbox, 100, boxes, out=rec_py)


eng = engine.Engine(path, dev)
rec_e = torch.empty(B, 100, 32, device=dev)


def eng_step():
    eng.detect(x, K, out=rec_e)


def timed(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for rep in range(3):
    tp, te = timed(py_step), timed(eng_step)
    log('per step %d (20 steps after 5 warm-up, events on the stream): python step %.3f ms | rtm3d_engine_detect %.3f ms' % (rep, tp, te))
torch.cuda.synchronize()
log('records equal: %s (kept 3D boxes %d)' % (torch.equal(rec_py, rec_e), int((rec_e[..., 31] == 2).sum())))
eng.close()
os.remove(path)
os.rmdir(workdir)
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
