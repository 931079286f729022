"""Heads stage in fp16 and in the opt-in MXFP8 mode (head_precision='mxfp8', csrc/conv_mx8.hip) at the flagship shape.

Per precision: per-op device ms of the head ops (rtm3d_forward_timed, median of --reps replays), the heads stage wall ms
(rtm3d_forward_marks), the pipelined step (Detect3DPipeline) ms and images/s; and the parity of the MXFP8 logits /
detections against the fp16 path on the same batch.  Prints one JSON line (also written to --out when given).

    python tools/gpu_heads_mx8.py [--batch 32] [--height 384] [--width 1280] [--steps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtm3d_amd                     # noqa: E402
from rtm3d_amd import weights        # noqa: E402

PEAK_FP8 = 5.0e15        # dense MXFP8 MFMA peak (MI355X)
PEAK_FP16 = 2.5e15       # dense fp16 MFMA peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    B, H, W = a.batch, a.height, a.width
    dev = torch.device('cuda', 0)
    bb = 'DLA-34'
    cfg = rtm3d_amd.kitti_config(bb)
    sd = weights.synth_state_dict(bb, 1, 'trained', heat_bias=-3.0)
    model = rtm3d_amd.create_model(cfg).to(dev).eval()
    model.load_state_dict(sd)
    x = weights.synth_images(B, H, W, seed=1234).to(dev)
    K = torch.as_tensor(np.tile(weights.synth_intrinsics(), (B, 1)), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {'shape': [B, H, W], 'backbone': bb}
    logits = {}
    for prec in ('fp16', 'mxfp8'):
        lg = model.forward_logits(x, head_precision=prec)
        torch.cuda.synchronize()
        logits[prec] = [t.clone() for t in lg]
        plan = model._plan_for(B, H, W, dev, 'dense', prec)
        optrs = [t.data_ptr() for t in lg]
        plan.forward_timed(stream, x.data_ptr(), optrs)
        runs = [plan.forward_timed(stream, x.data_ptr(), optrs) for _ in range(a.reps)]
        ops = []
        for k, op in enumerate(runs[0]):
            if not op['name'].startswith('heads'):
                continue
            ms = float(np.median([r[k]['ms'] for r in runs]))
            d = {'name': op['name'], 'kernel': op['kernel'], 'ms': round(ms, 4)}
            if op['flops']:
                tf = op['flops'] / (ms * 1e-3)
                d.update(tflops=round(tf / 1e12, 1), frac_fp8_peak=round(tf / PEAK_FP8, 3), frac_fp16_peak=round(tf / PEAK_FP16, 3))
            ops.append(d)
        names = [i['name'] for i in runs[0]]
        mark = next(k for k, n in enumerate(names) if n.startswith('heads'))
        stage = [plan.forward_marks(stream, x.data_ptr(), optrs, [mark])[0] for _ in range(a.reps + 1)][1:]
        # the pipelined step (forward + decode2d + decode3d + records), as bench.py runs it
        from rtm3d_amd.pipeline import Detect3DPipeline
        pipe = Detect3DPipeline(model, B, dev, gather=True, head_precision=prec)
        for _ in range(3):
            pipe.submit(x, K)
        pipe.drain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            pipe.submit(x, K)
        pipe.drain()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        res[prec] = {'head_ops': ops, 'heads_op_sum_ms': round(sum(o['ms'] for o in ops), 3),
                     'heads_stage_wall_ms': round(float(np.median(stage)), 3), 'step_ms': round(dt * 1e3, 3),
                     'images_per_s': round(B / dt, 1)}
        del pipe
    res['heads_stage_ratio_mxfp8_over_fp16'] = round(res['mxfp8']['heads_stage_wall_ms'] / res['fp16']['heads_stage_wall_ms'], 3)
    # parity on this batch: logits and detections of the MXFP8 path against the fp16 path
    rel = [float((a_ - b_).abs().max()) / max(1.0, float(b_.abs().max())) for a_, b_ in zip(logits['mxfp8'], logits['fp16'])]
    d16 = model.inference(tuple(logits['fp16']))
    d8 = model.inference(tuple(logits['mxfp8']))
    tot = hit = 0
    vmax = 0.0
    for b in range(B):
        if d16[0][b] is None:
            continue
        ref = {(int(c), int(m[0] // 4), int(m[1] // 4)): v for c, m, v in zip(d16[0][b].cpu().numpy(), d16[2][b].cpu().numpy(), d16[3][b].cpu().numpy())}
        got = {} if d8[0][b] is None else {(int(c), int(m[0] // 4), int(m[1] // 4)): v for c, m, v in
                                             zip(d8[0][b].cpu().numpy(), d8[2][b].cpu().numpy(), d8[3][b].cpu().numpy())}
        for k, v in ref.items():
            tot += 1
            if k in got:
                hit += 1
                vmax = max(vmax, float(np.abs(got[k] - v).max()))
    res['parity_vs_fp16'] = {'logit_rel_err': [round(r, 5) for r in rel], 'fp16_detections': tot,
                             'matched_share': round(hit / max(1, tot), 4), 'vertex_linf_px': round(vmax, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
