#!/usr/bin/env python3
"""Throughput of the RTM3D inference hot path on MI355X.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the whole hot path over one batch already resident in HBM:
backbone + neck + heads (HIP MFMA/direct convs) -> 2D decode (sigmoid/NMS/top-k/gather) ->
3D decode (fp64 L-BFGS-B per object) [-> at N>1: one RCCL all-gather of the detection records].
Workload = BASELINE.json configs[2]: rtm3d_dla34_kitti, bs=32 per GPU, 384x1280, fp16 storage /
fp32 accumulate, seeded synthetic weights ("trained"-style) and images.  Weak scaling: every rank
processes its own 32-image shard (configs[3] = 8 x 32).

Prints ONE JSON line (rank 0) with the driver's keys plus `roofline` (dominant kernel, timed live
with hipEvents on the launch stream during the timed steps).  A plain run does only that: set up, warm up,
time the steps, print the line.  `--full` adds what takes runs of its own outside the timed steps:
`cpu_baseline` (the CPU oracle = PyTorch-CPU fp32 restatement of the reference + SciPy L-BFGS-B, timed
on this host on a bounded sample), `parity` (3D-box L-inf against that oracle), the peaks-only probe
`detect_surface_sparse_heads` and the per-stage wall times `roofline.per_stage[*].wall_ms`.
`--dump-outputs DIR` also writes the last timed step's detection records to DIR/records.npy, to compare two builds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_FP16_MFMA_TFLOPS = 2500.0     # dense, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0

# (backbone) -> (weight seed, heat-map bias) giving a sparse, realistic number of detections/image
SYNTH = {'DLA-34': (1, -6.0), 'RESNET-18': (1, -5.0)}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--backbone', default='DLA-34')
    ap.add_argument('--batch', type=int, default=32, help='images per GPU')
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--full', action='store_true',
                    help='also measure and check, outside the timed steps, what the headline does not need: the CPU baseline, the parity block '
                         'against the CPU oracle, the peaks-only probe and the per-stage wall times (without it: cpu_baseline and parity are null)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--cpu-full', action='store_true', help='with --full: whole BASELINE.md section-4 CPU protocol (adds minutes: one-thread bs=8)')
    ap.add_argument('--cpu-threads', type=int, default=0, help='threads of the all-thread CPU legs (0: min(scheduler affinity, cgroup CPU quota))')
    ap.add_argument('--no-parity', action='store_true', help='with --full: skip the 3D-box L-inf check against the CPU oracle')
    ap.add_argument('--parity-images', type=int, default=8, help='benchmark images the oracle runs for the parity block (16 planted cuboids each)')
    ap.add_argument('--side-cus', type=int, default=0, help='CUs the decode3d side stream may use (0 = unrestricted)')
    ap.add_argument('--depth', type=int, default=0, help='pipeline slots (0: automatic)')
    ap.add_argument('--side-streams', type=int, default=0, help='decode3d side streams (0: automatic)')
    ap.add_argument('--no-conv128', action='store_true', help='DIAGNOSTIC (A/B): 128->128 3x3 layers on the generic kernel instead of conv128_halo')
    ap.add_argument('--serial', action='store_true', help='single stream, no decode3d/forward overlap')
    ap.add_argument('--diag-no-decode3d', action='store_true', help='DIAGNOSTIC ONLY: skip the 3D decode (result is not a valid benchmark)')
    ap.add_argument('--heat-bias', type=float, default=None, help='override the synthetic heat-map bias (e.g. +2: top-k saturates, 100 objects/image; marks the line DIAGNOSTIC)')
    ap.add_argument('--v2-min-tiles', type=int, default=None, help='DIAGNOSTIC: fewest 256x256 tiles a layer needs to go to the persistent conv256 kernel (plan.V2_MIN_TILES)')
    ap.add_argument('--from-uint8', choices=['step', 'once'], default=None,
                    help='row n1 measured on B uint8 360x1240 camera-style images resident in HBM.  step: every step runs Resize to 1280 + letterbox + '
                         'normalise on the device (two launches, straight into the fp16 input tensor) in front of the plan; once: the same images are '
                         'preprocessed once, outside the timed region, into the fp32 NCHW batch that is then fed like the BASELINE line (the A/B partner)')
    ap.add_argument('--graph', action='store_true', help='DIAGNOSTIC (A/B): replay the plan as one hipGraph (the live roofline probe needs the eager replay, so launch_ms then comes from the per-op pass)')
    ap.add_argument('--bn-tile', action='append', default=[], metavar='OP=N', help='DIAGNOSTIC (A/B): output-channel tile (16/32/64/128) of the 128-pixel conv kernel for the op named OP (plan.BN_TILE_OVERRIDE)')
    ap.add_argument('--no-sparse-probe', action='store_true', help='with --full: skip the informational detect_surface_sparse_heads block (a few pipelined steps of the peaks-only mode after the timed region)')
    ap.add_argument('--sparse-heads', action='store_true', help='DIAGNOSTIC (not the BASELINE line): the detect3d call surface with the regression head branches evaluated at the detected peaks only (Model.decode2d_sparse); Model.forward() and the headline keep all four dense maps')
    ap.add_argument('--zero-weights', action='store_true', help='DIAGNOSTIC: all weights and biases zero (every activation is 0): what the same kernels do when the MFMA operands carry no energy (profiles/r03_heads_clock.txt)')
    ap.add_argument('--solver-form', choices=['direct', 'published'], default=None,
                    help="search direction of the 3D decode inside the timed step (rtm3d_decode3d_slots form): 'direct' = two-loop recursion, "
                         "'published' = L-BFGS-B 3.0's subspace step, the arithmetic SciPy runs for the reference; default: rtm3d_amd.model_utils.DEFAULT_SOLVER_FORM")
    ap.add_argument('--shared-weight-cache', action='store_true', help='N > 1: rank 0 folds and packs the weights and writes the on-disk weight cache, the other ranks build their plans from that file behind a barrier (off by default: measured SLOWER at 4 ranks on a 16-core host share, 3.3 s against 2.8 s from spawn to the first timed step - packing is 0.5 s per rank and the barrier serialises it; for hosts with few cores per rank)')
    ap.add_argument('--per-op', action='store_true', help='also print a per-kernel table to stderr')
    ap.add_argument('--force-launch', action='store_true', help='go through the rank launcher even for --gpus 1 (rehearses the N > 1 path: process group, RCCL all-gather)')
    ap.add_argument('--rehearse-one-gpu', action='store_true', help='DIAGNOSTIC: the N ranks of --gpus N all run on GPU 0 and exchange their records over gloo through host memory (RCCL refuses duplicate devices): the whole N > 1 code path - shards, pipelined gather, ordering, diagnostics - on a one-GPU box; the line is marked INVALID')
    ap.add_argument('--dry-launch', action='store_true', help='launcher rehearsal over gloo on CPU tensors, no GPU and no hot path (line marked INVALID)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step handed its caller (the (world*B, topk, 32) detection '
                         'records) as DIR/records.npy (float32, at most 64 MB: a fixed seeded sample of images beyond that); '
                         'inputs are seeded, so two builds run with the same arguments can be compared output for output')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    return args


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """Writes each tensor of `arrays` (name -> tensor) as d/<name>.npy in float32 (float64 stays float64).  If they exceed
    DUMP_BUDGET_BYTES together, each keeps a fixed seeded sample of its rows (first axis), and d/<name>_rows.npy says which."""
    os.makedirs(d, exist_ok=True)
    arrs = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        arrs[name] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float32)
    total = sum(a.nbytes for a in arrs.values())
    for name, a in arrs.items():
        if total > DUMP_BUDGET_BYTES and a.ndim > 0 and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * (DUMP_BUDGET_BYTES - 2 ** 20) // total))
            rows = np.sort(np.random.Generator(np.random.PCG64(0)).choice(a.shape[0], keep, replace=False))
            np.save(os.path.join(d, name + '_rows.npy'), rows.astype(np.float64))
            a = a[rows]
        np.save(os.path.join(d, name + '.npy'), np.ascontiguousarray(a))


def _best_median(ts):
    ts = sorted(ts)
    return ts[0], ts[len(ts) // 2]


def host_cpu_info():
    """What this process may really use: scheduler affinity, the cgroup CPU quota (v2 cpu.max, v1 cfs_quota_us), the CPU
    model.  `usable` = min(affinity, ceil(quota)) is the thread count of the all-thread legs: more OpenMP threads than the
    quota admits only time-slice against each other (r02: 128 threads inside a smaller quota ran 1.46x one thread)."""
    import math
    info = {'os_cpu_count': os.cpu_count()}
    try:
        info['affinity'] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        info['affinity'] = os.cpu_count() or 1
    quota = None
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:                      # cgroup v2: "max 100000" or "<quota> <period>"
            q, per = f.read().split()[:2]
            quota = None if q == 'max' else float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us') as f:     # cgroup v1
                q = float(f.read())
            with open('/sys/fs/cgroup/cpu/cpu.cfs_period_us') as f:
                per = float(f.read())
            quota = None if q <= 0 else q / per
        except (OSError, ValueError):
            pass
    info['cgroup_cpu_quota'] = quota
    model = None
    try:
        with open('/proc/cpuinfo') as f:
            for ln in f:
                if ln.lower().startswith('model name'):
                    model = ln.split(':', 1)[1].strip()
                    break
    except OSError:
        pass
    info['cpu_model'] = model
    info['usable'] = max(1, min(info['affinity'], int(math.ceil(quota)) if quota else info['affinity']))
    return info


def cpu_baseline(backbone, sd, H, W, cfg, full=False, threads=None):
    """The oracle timed on this host, BASELINE.md section 4: all usable host threads and one thread, bs=1 and bs=8,
    1 warm-up + 3 timed runs (best / median), forward + 2D decode (images/s) and the SciPy 3D decode (objects/s)
    separately.  Bounded by default (about 30-40 s): the one-thread leg runs bs=1 once warm + 2 timed and skips bs=8
    unless --cpu-full.  `value` = whole path (forward + 2D + 3D decode of the detections found) at the best
    all-thread configuration.  `cores` = the threads the all-thread legs really ran on (host_cpu_info()['usable'], or
    --cpu-threads); every leg also reports process-CPU-seconds / wall-seconds (`cpus_busy`), so a leg that was not what its
    name says (one thread that is not one, a pool throttled by a quota) shows in the line itself."""
    from oracle import rtm3d_ref, decode3d_ref
    from rtm3d_amd import weights
    host = host_cpu_info()
    torch_default = torch.get_num_threads()
    nthreads = int(threads) if threads else host['usable']
    torch.set_num_threads(nthreads)
    th, tk = cfg.DETECTOR.SCORE_THRESH, cfg.DETECTOR.TOPK_CANDIDATES
    x8 = weights.synth_images(8, H, W, seed=1234)
    K = weights.synth_intrinsics()
    detail = {}
    gflop_img = {'DLA-34': 436.28, 'RESNET-18': 411.62}.get(backbone)

    def time_forward(bs, runs, warm=1):
        for _ in range(warm):
            rtm3d_ref.model_forward(x8[:bs], sd, backbone, th, tk)
        ts, busy = [], []
        for _ in range(runs):
            c0, t0 = time.process_time(), time.perf_counter()
            dets, _ = rtm3d_ref.model_forward(x8[:bs], sd, backbone, th, tk)
            t1, c1 = time.perf_counter(), time.process_time()
            ts.append(t1 - t0); busy.append((c1 - c0) / (t1 - t0))
        return ts, dets, busy

    def leg(bs, nt, ts, busy):
        best, med = _best_median(ts)
        d = {'best_s': best, 'median_s': med, 'images_per_s_best': bs / best, 'torch_threads': torch.get_num_threads(),
             'cpus_busy': round(sorted(busy)[len(busy) // 2], 2)}
        if gflop_img:
            d['gflops_best'] = round(gflop_img * bs / best, 1)
        detail['forward+decode2d bs=%d threads=%d' % (bs, nt)] = d

    dets8 = None
    try:
        for bs in (1, 8):
            ts, dets, busy = time_forward(bs, 3)
            assert torch.get_num_threads() == nthreads
            leg(bs, nthreads, ts, busy)
            if bs == 8:
                dets8 = dets
        torch.set_num_threads(1)
        assert torch.get_num_threads() == 1
        ts, _, busy = time_forward(1, 3 if full else 2)
        leg(1, 1, ts, busy)
        if full:
            ts, _, busy = time_forward(8, 3)
            leg(8, 1, ts, busy)
    finally:
        torch.set_num_threads(torch_default)
    # 3D decode: SciPy L-BFGS-B with Python-level objective/gradient, one thread by construction
    objs = [(dets8[0][i].numpy(), dets8[3][i].numpy()) for i in range(8) if dets8[0][i] is not None]
    nobj = sum(len(c) for c, _ in objs)
    ts = []
    for _ in range(3 if nobj else 0):
        t0 = time.perf_counter()
        cnt = 0
        for c, v in objs:
            decode3d_ref.optim_decode_bbox3d(c[:5], v[:5], K, cfg.DETECTOR.dim_ref, [0, -0.5, 20])
            cnt += len(c[:5])
        ts.append(time.perf_counter() - t0)
    per_obj = None
    if ts:
        best, med = _best_median(ts)
        per_obj = best / cnt
        detail['decode3d scipy threads=1'] = {'objects': cnt, 'best_s': best, 'median_s': med, 'objects_per_s_best': cnt / best}
    fw = max(detail['forward+decode2d bs=%d threads=%d' % (bs, nthreads)]['images_per_s_best'] for bs in (1, 8))
    per_img = 1.0 / fw + (per_obj or 0.0) * nobj / 8.0
    return {'value': 1.0 / per_img, 'unit': 'images/s', 'cores': nthreads, 'kind': 'port', 'host': host,
            'sample': '%s %dx%d fp32 PyTorch-CPU oracle: forward+2D decode bs=1 and bs=8 (1 warm-up + 3 timed, best) on %d threads '
                      '(= min(affinity %d, cgroup quota %s) of a %s), '
                      '+ SciPy L-BFGS-B 3D decode at %.1f objects/image (measured on %d objects, 3 runs, 1 thread); '
                      'one-thread forward timed beside it' % (backbone, H, W, nthreads, host['affinity'], host['cgroup_cpu_quota'],
                                                              host['cpu_model'], nobj / 8.0, cnt if ts else 0),
            'detail': detail}


def _dist(values, bar=1e-4):
    """p50 / p90 / p99 / max and the share at or below the bar of a 1-D sample."""
    v = np.asarray(values, np.float64)
    if v.size == 0:
        return None
    q = np.percentile(v, [50, 90, 99])
    return {'n': int(v.size), 'p50': float(q[0]), 'p90': float(q[1]), 'p99': float(q[2]), 'max': float(v.max()),
            'frac_le_%g' % bar: float((v <= bar).mean())}


BOX_PARAMS = ['Ry', 'h', 'w', 'l', 'X', 'Y', 'Z']


def _box_stats(boxd):
    """boxd: list of (7,) |device - reference| per box over [Ry, h, w, l, X, Y, Z].  Per-box L-inf distribution + the same
    per parameter."""
    if not boxd:
        return None
    bd = np.stack(boxd)
    out = {'box_linf': _dist(bd.max(1))}
    out['per_param'] = {n: {k: v for k, v in _dist(bd[:, i]).items() if k != 'n'} for i, n in enumerate(BOX_PARAMS)}
    return out


def csrc_sha1():
    """sha1 over the kernel sources (rtm3d_amd/csrc/*.hip, *.h, Makefile): what a committed PMC profile is 'of'."""
    import hashlib
    h = hashlib.sha1()
    d = os.path.join(ROOT, 'rtm3d_amd', 'csrc')
    for f in sorted(os.listdir(d)):
        if f.endswith(('.hip', '.h')) or f == 'Makefile':
            h.update(f.encode()); h.update(open(os.path.join(d, f), 'rb').read())
    return h.hexdigest()


def _default_solver_form():
    from rtm3d_amd.model_utils import DEFAULT_SOLVER_FORM
    return DEFAULT_SOLVER_FORM


def parity_check(model, cfg, sd, backbone, x_dev, k, dev, planted=16, draws=2, solver_form=None):
    """BASELINE metric, second half: 3D-box L-inf of the device pipeline vs the CPU reference path (the oracle), on
    the first k images of the benchmark workload (`x_dev` = the benchmark batch: the device runs the SAME plan / kernels
    as the timed steps on the whole batch, the oracle the first k images of it).  Regimes:
      stage : the device decode kernels fed the ORACLE's fp32 logits, with `planted` exact cuboid projections per image
              written over them (tests/golden/cases.plant_cuboids) so that real boxes are kept (fun < 0.1) next to the
              workload's natural detections: indices must be identical, boxes are compared on the kept objects;
      e2e   : images -> fp16 network -> device decode, against the fp32 oracle end to end: detections matched by
              (class, y, x) cell, vertex / score L-inf on the matches, box |d| on the objects BOTH sides keep: per-box L-inf
              and per-parameter p50 / p90 / p99 / max and the share within 1e-4 (north_star's bar);
      e2e_fp32_mode : the same with the network in the fp32 verification mode;
      reference_sensitivity : the REFERENCE's own decode (SciPy, through the oracle) re-run on its own kept objects with
              the vertices moved by uniform noise of the vertex error each mode was measured at: how far the reference
              itself moves for an input error of that size (the yardstick for the two e2e distributions)."""
    from oracle import rtm3d_ref, decode3d_ref
    from rtm3d_amd import weights
    from rtm3d_amd.model_utils import decode3d_slots as _decode3d_slots, DEFAULT_SOLVER_FORM
    from tests.golden.cases import plant_cuboids
    solver_form = DEFAULT_SOLVER_FORM if solver_form is None else solver_form

    def decode3d_slots(det_, K_, dim_, loc_):          # every decode of this block runs the form the timed step ran
        return _decode3d_slots(det_, K_, dim_, loc_, form=solver_form)
    t_start = time.perf_counter()
    th, tk = float(cfg.DETECTOR.SCORE_THRESH), int(cfg.DETECTOR.TOPK_CANDIDATES)
    dim_ref = cfg.DETECTOR.dim_ref
    k = min(k, x_dev.shape[0])
    x = x_dev[:k].cpu()
    K = weights.synth_intrinsics()
    Kd = torch.as_tensor(np.tile(K, (k, 1)), dtype=torch.float64, device=dev)
    Kd_all = torch.as_tensor(np.tile(K, (x_dev.shape[0], 1)), dtype=torch.float64, device=dev)
    host = host_cpu_info()
    torch_default = torch.get_num_threads()
    torch.set_num_threads(host['usable'])
    try:
        dets_ref, logits_ref = rtm3d_ref.model_forward(x, sd, backbone, th, tk)
    finally:
        torch.set_num_threads(torch_default)

    def box_params(xs):            # (n, 8) solver state -> (n, 7) [Ry, h, w, l, X, Y, Z]  (utils/model_utils.py:300-303)
        return np.concatenate([np.arctan2(xs[:, 0:1], xs[:, 1:2]), xs[:, 3:5], xs[:, 2:3], xs[:, 5:8]], 1)

    def angle_diff(a, b):
        d = np.abs(a - b)
        d[:, 0] = np.minimum(d[:, 0], 2 * np.pi - d[:, 0])
        return d

    def solve_ref(dets, b, verts=None):
        v = dets[3][b].numpy() if verts is None else verts
        _, raw = decode3d_ref.optim_decode_bbox3d(dets[0][b].numpy(), v, K, dim_ref, [0, -0.5, 20], return_raw=True)
        return raw

    out = {'images': k, 'planted_per_image': planted,
           'reference': 'oracle: PyTorch-CPU fp32 forward + Model.inference restatement + SciPy L-BFGS-B'}
    # ---------------------------------------------------------------- stage regime (planted cuboids on oracle logits)
    lg = [l.numpy().copy() for l in logits_ref]
    truth = plant_cuboids(lg[0], lg[1:], K, planted, np.random.Generator(np.random.PCG64(2)))
    raws_p = [None] * k
    dets_p = rtm3d_ref.inference([torch.from_numpy(a) for a in lg], th, tk, 4.0)
    det = model.decode2d([torch.from_numpy(a).to(dev) for a in lg])
    boxes = decode3d_slots(det, Kd, dim_ref, [0, -0.5, 20])
    torch.cuda.synchronize(dev)
    n_dev = det.n.cpu().numpy()
    xs, fs = boxes.x.cpu().numpy(), boxes.fun.cpu().numpy()
    st = {'objects': 0, 'index_mismatches': 0, 'kept_ref': 0, 'kept_dev': 0, 'keep_decision_mismatches': 0, 'box_linf': 0.0,
          'vert_linf_px': 0.0}
    st_boxd = []
    for b in range(k):
        nr = 0 if dets_p[0][b] is None else len(dets_p[0][b])
        if nr:
            raws_p[b] = solve_ref(dets_p, b)
        if nr != int(n_dev[b]):
            st['index_mismatches'] += abs(nr - int(n_dev[b]))
            continue
        if nr == 0:
            continue
        sl = slice(b * tk, b * tk + nr)
        st['objects'] += nr
        st['index_mismatches'] += int((det.cls[sl].cpu().numpy() != dets_p[0][b].numpy()).sum())
        st['vert_linf_px'] = max(st['vert_linf_px'], float(np.abs(det.verts[sl].cpu().numpy() - dets_p[3][b].numpy()).max()))
        raw = raws_p[b]
        kr, kd = raw['kept'], fs[sl] < 0.1
        st['kept_ref'] += int(kr.sum()); st['kept_dev'] += int(kd.sum())
        st['keep_decision_mismatches'] += int((kr != kd).sum())
        both = kr & kd
        if both.any():
            dv = angle_diff(box_params(xs[sl][both]), box_params(raw['x'][both]))
            st_boxd.extend(list(dv))
            st['box_linf'] = max(st['box_linf'], float(dv.max()))
    st['boxes'] = _box_stats(st_boxd)
    st['solver_form'] = solver_form                # the form of rtm3d_decode3d_slots the timed step (and this block) ran
    # the same stage inputs through the solver's OTHER form (the flat entry rtm3d_decode3d): with the default - the published
    # subspace step SciPy runs - in the timed step this is the opt-in direct two-loop form, and the other way round
    from rtm3d_amd.model_utils import solve_boxes
    other = 'direct' if solver_form == 'published' else 'published'
    oth_boxd, oth_nit = [], 0
    for b in range(k):
        if raws_p[b] is None:
            continue
        xp, fp_, nitp, _ = solve_boxes(dets_p[0][b].numpy(), dets_p[3][b].numpy(), K, dim_ref, [0, -0.5, 20], device=dev, form=other)
        both = raws_p[b]['kept'] & (fp_ < 0.1)
        oth_nit += int((nitp != raws_p[b]['nit'])[both].sum())
        if both.any():
            oth_boxd.extend(list(angle_diff(box_params(xp[both]), box_params(raws_p[b]['x'][both]))))
    st[other + '_form'] = {'boxes': _box_stats(oth_boxd), 'iteration_count_differs': oth_nit}
    out['stage'] = st
    # ---------------------------------------------------------------- end to end (fp16 network on the device)
    def match_e2e(det, boxes, dets_o, raws, only_cells=None):
        """Device slots vs oracle detections, matched by (class, y, x) cell; only_cells restricts the oracle side."""
        n_dev = det.n.cpu().numpy()
        xs, fs = boxes.x.cpu().numpy(), boxes.fun.cpu().numpy()
        e = {'ref_detections': 0, 'dev_detections': int(n_dev[:k].sum()), 'matched': 0, 'missed': 0, 'vert_linf_px': 0.0,
             'score_linf': 0.0, 'kept_ref': 0, 'kept_dev': 0, 'kept_both': 0, 'box_linf': None, 'fun_rel_median': None}
        frel, boxd, vd = [], [], []
        for b in range(k):
            nd = int(n_dev[b])
            sl = slice(b * tk, b * tk + nd)
            cells = {}
            if nd:
                cl, mp, vv, sc = (t[sl].cpu().numpy() for t in (det.cls, det.mproj, det.verts, det.score))
                for j, (c, m) in enumerate(zip(cl, mp)):
                    cells[(int(c), int(m[0] // 4), int(m[1] // 4))] = j
            if dets_o[0][b] is None:
                continue
            raw = raws[b]
            for i, (c, m) in enumerate(zip(dets_o[0][b].numpy(), dets_o[2][b].numpy())):
                cell = (int(c), int(m[0] // 4), int(m[1] // 4))
                if only_cells is not None and (b,) + cell not in only_cells:
                    continue
                e['ref_detections'] += 1
                e['kept_ref'] += int(raw['kept'][i])
                j = cells.get(cell)
                if j is None:
                    e['missed'] += 1
                    continue
                e['matched'] += 1
                e['kept_dev'] += int(fs[sl][j] < 0.1)
                vd.append(float(np.abs(vv[j] - dets_o[3][b][i].numpy()).max()))
                e['score_linf'] = max(e['score_linf'], abs(float(sc[j]) - float(dets_o[1][b][i])))
                frel.append(abs(fs[sl][j] / raw['fun'][i] - 1.0))
                if raw['kept'][i] and fs[sl][j] < 0.1:
                    e['kept_both'] += 1
                    boxd.append(angle_diff(box_params(xs[sl][j:j + 1]), box_params(raw['x'][i:i + 1]))[0])
        if vd:
            e['vert_linf_px'] = max(vd)
            e['vert_px'] = {kk: vv_ for kk, vv_ in _dist(vd, 0.25).items()}
        if frel:
            e['fun_rel_median'] = float(np.median(frel))
        if boxd:
            # the fit is ill-conditioned for distant boxes (a 0.03 px vertex error moves a box at 50 m by centimetres): the
            # maximum is one object's; the distribution and the per-parameter columns [Ry, h, w, l, X, Y, Z] say how typical it is
            bd = np.stack(boxd)
            e['box_linf'] = float(bd.max())
            e['box_median'] = float(np.median(bd.max(1)))
            e['box_linf_per_param'] = [float(v) for v in bd.max(0)]
            e['boxes'] = _box_stats(boxd)
        return e

    # (a) the workload's natural detections
    det, boxes, logits_dev = model.detect3d(x_dev, Kd_all)
    torch.cuda.synchronize(dev)
    logits_dev = [l[:k] for l in logits_dev]
    raws_nat = [None if dets_ref[0][b] is None else solve_ref(dets_ref, b) for b in range(k)]
    e_nat = match_e2e(det, boxes, dets_ref, raws_nat)
    # (b) the same planted cuboids carried END TO END: the planting is applied to the device's own logits as the additive
    # difference (planted - natural) of the oracle's, so each planted vertex on the device = exact projection + the fp16
    # network's real error at that pixel; both sides then run their own 2D and 3D decode
    lg_dev = [l + torch.from_numpy(p_ - n_.numpy()).to(dev) for l, p_, n_ in zip(logits_dev, lg, logits_ref)]
    det2 = model.decode2d(lg_dev)
    boxes2 = decode3d_slots(det2, Kd, dim_ref, [0, -0.5, 20])
    torch.cuda.synchronize(dev)
    only = set((b, c, xx, yy) for b in range(k) for (c, yy, xx, _, _, _) in truth[b])
    e_pl = match_e2e(det2, boxes2, dets_p, raws_p, only)
    out['e2e'] = e_nat
    out['e2e_planted'] = e_pl
    # (c) the same two comparisons with the network in the fp32 VERIFICATION mode (Model.forward_logits_fp32: the same plan
    # on fp32 tensors, rtm3d_amd/verify.py) and the product's own decode kernels: what is left is fp32 round-off plus the
    # reference solver's own sensitivity to it
    lg32 = model.forward_logits_fp32(x_dev[:k])
    det3 = model.decode2d(lg32)
    boxes3 = decode3d_slots(det3, Kd, dim_ref, [0, -0.5, 20])
    lg32p = [l + torch.from_numpy(p_ - n_.numpy()).to(dev) for l, p_, n_ in zip(lg32, lg, logits_ref)]
    det4 = model.decode2d(lg32p)
    boxes4 = decode3d_slots(det4, Kd, dim_ref, [0, -0.5, 20])
    torch.cuda.synchronize(dev)
    model.release_verify()                     # free the fp32 workspace
    out['e2e_fp32_mode'] = match_e2e(det3, boxes3, dets_ref, raws_nat)
    out['e2e_fp32_mode_planted'] = match_e2e(det4, boxes4, dets_p, raws_p, only)
    out['e2e_fp32_mode']['logit_linf_rel'] = max(float((a[:k].cpu() - b_).abs().max() / max(1.0, float(b_.abs().max())))
                                                 for a, b_ in zip(lg32, logits_ref))
    # (d) the reference's own sensitivity at the vertex error each mode was measured at (uniform noise of that amplitude on
    # every vertex coordinate of the planted images' detections, `draws` draws; boxes compared on the planted objects the
    # reference keeps in both runs)
    rng = np.random.default_rng(7)
    sens = {}
    for mode, e_ in (('fp16', e_pl), ('fp32_mode', out['e2e_fp32_mode_planted'])):
        eps = float(e_['vert_px']['p50']) if e_.get('vert_px') else 0.0
        boxd, nit_changed, n_obj = [], 0, 0
        for _ in range(draws if eps > 0 else 0):
            for b in range(k):
                if dets_p[0][b] is None:
                    continue
                v = dets_p[3][b].numpy()
                r2 = solve_ref(dets_p, b, (v + rng.uniform(-eps, eps, v.shape)).astype(np.float32))
                both = raws_p[b]['kept'] & r2['kept']
                nit_changed += int((r2['nit'] != raws_p[b]['nit'])[both].sum()); n_obj += int(both.sum())
                if both.any():
                    boxd.extend(list(angle_diff(box_params(r2['x'][both]), box_params(raws_p[b]['x'][both]))))
        sens[mode] = {'eps_px': eps, 'draws': draws, 'solves': n_obj, 'iteration_count_changed': nit_changed, 'boxes': _box_stats(boxd)}
    out['reference_sensitivity'] = sens
    # flat summary (the names VERDICT r01 / r02 asked for)
    bs16, bs32 = e_pl.get('boxes'), out['e2e_fp32_mode_planted'].get('boxes')
    out.update({'stage_box_linf': st['box_linf'], 'e2e_vert_linf_px': max(e_nat['vert_linf_px'], e_pl['vert_linf_px']),
                'e2e_box_linf': e_pl['box_linf'], 'matched': e_nat['matched'] + e_pl['matched'], 'missed': e_nat['missed'] + e_pl['missed'],
                'reference_kept_boxes_compared': e_pl['kept_both'],
                'e2e_box_fp16': bs16['box_linf'] if bs16 else None,
                'e2e_box_fp32_mode': bs32['box_linf'] if bs32 else None,
                'reference_sensitivity_at_fp16_vertex_error': sens['fp16']['boxes']['box_linf'] if sens['fp16']['boxes'] else None,
                'reference_sensitivity_at_fp32_vertex_error': sens['fp32_mode']['boxes']['box_linf'] if sens['fp32_mode']['boxes'] else None,
                'e2e_box_linf_fp32_mode': out['e2e_fp32_mode_planted']['box_linf'],
                'e2e_box_median_fp32_mode': out['e2e_fp32_mode_planted'].get('box_median'),
                'seconds': None})
    out['note'] = ('stage: device decode kernels on the oracle fp32 logits of the benchmark images with %d exact cuboid projections '
                   'planted per image (bar: identical indices, boxes 1e-4).  e2e: fp16 network on the device vs the fp32 oracle end to '
                   'end, detections matched by (class, y, x); the synthetic-weight workload itself has no cuboid-consistent key points '
                   '(the reference keeps none), so box |d| is measured on the same planted cuboids carried through the network '
                   'additively (device logits + oracle(planted - natural)): planted vertices on the device = exact + real fp16 error.  '
                   'e2e_fp32_mode*: the same comparisons with the network in the fp32 verification mode (same plan, fp32 tensors, '
                   'fp64 accumulation; product decode kernels).  reference_sensitivity: the oracle re-run on its own detections with the '
                   'vertices moved by uniform noise of each mode\'s median vertex error; per-box L-inf over [Ry, h, w, l, X, Y, Z] in '
                   'rad / m' % planted)
    out['seconds'] = round(time.perf_counter() - t_start, 1)
    return out


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(('127.0.0.1', 0))
        return so.getsockname()[1]


def launch_ranks(n, argv):
    """Start the N ranks of `--gpus N` as FRESH child processes under torch.distributed.run (what the reference does with
    mp.spawn, /root/reference/train_multi_gpu.py:239-245) and return their exit code.  Called before anything in this
    process has touched the GPU; the current process is never replaced (no exec): it waits and exits with the children's rc."""
    import subprocess
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC (RCCL needs it on this driver)
    # threads per rank from what this process may really use (scheduler affinity / cgroup quota, the figure cpu_baseline reports),
    # not from os.cpu_count(): 8 ranks x 32 OpenMP threads inside a 16-CPU quota only time-slice against each other while every
    # rank folds BatchNorms and draws its synthetic images
    env.setdefault('OMP_NUM_THREADS', str(max(1, host_cpu_info()['usable'] // n)))
    env['RTM3D_BENCH_LAUNCHED'] = '1'
    env['RTM3D_BENCH_SPAWN_T'] = repr(time.time())          # wall clock at spawn: ranks report spawn -> first timed step
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.abspath(__file__)] + list(argv)
    print('bench.py: starting %d ranks: %s' % (n, ' '.join(cmd)), file=sys.stderr)
    return subprocess.run(cmd, env=env).returncode


def multi_diagnostics(world, B, steps, dt, rec, local, dev, gather_us, startup_s=None):
    """Diagnostics of an N-rank run, outside the timed region: max-over-ranks wall time, every rank's own ms/step, and how
    many ranks' record blocks arrived intact in this rank's gathered batch (checksum of each rank's local block, gathered
    separately, against the block sums of the gathered records)."""
    if dist.get_backend() == 'gloo':               # dry launch / one-GPU rehearsal: gloo collectives on host tensors
        dev = torch.device('cpu')
    mine = torch.tensor([dt], dtype=torch.float64, device=dev)
    allt = torch.empty(world, dtype=torch.float64, device=dev)
    dist.all_gather_into_tensor(allt, mine)
    t = mine.clone()
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    multi = {'per_rank_ms_per_step': [round(v / steps * 1e3, 3) for v in allt.tolist()]}
    # checksum of a block = int64 sum of its fp32 bit patterns: exact and independent of the order a reduction adds in (a float sum of
    # the (B,100,32) block and a row sum of the gathered tensor round differently: seen as ranks_seen 1 of 2 in a rehearsal)
    cs = local.contiguous().view(torch.int32).to(torch.int64).sum().reshape(1).to(dev)
    allcs = torch.empty(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(allcs, cs)
    ok = rec.shape[0] == world * B
    blocks = rec.contiguous().view(torch.int32).reshape(world, -1).to(torch.int64).sum(1).to(dev) if ok else None
    multi['ranks_seen'] = int((blocks == allcs).sum().item()) if ok else 0
    multi['gathered_shape'] = list(rec.shape)
    multi['allgather_us_last_step'] = round(gather_us, 1) if gather_us is not None else None
    multi['allgather_bytes_per_rank'] = int(local.numel() * 4)
    if startup_s is not None:
        # wall time from the launcher's spawn to this rank's first timed step (process start, imports, weight synthesis + BN folding,
        # plan recording, warm-up): the slowest rank's, i.e. what an N-rank run costs before it measures anything
        su = torch.tensor([startup_s], dtype=torch.float64, device=dev)
        dist.all_reduce(su, op=dist.ReduceOp.MAX)
        multi['startup_s_spawn_to_first_timed_step'] = round(float(su.item()), 2)
        multi['omp_threads_per_rank'] = int(os.environ.get('OMP_NUM_THREADS', '0') or 0)
    return float(t.item()), multi


def _startup_s(t0_perf):
    """Seconds from the launcher's spawn (RTM3D_BENCH_SPAWN_T, wall clock) to the start of the timed region (perf_counter t0)."""
    spawn = os.environ.get('RTM3D_BENCH_SPAWN_T')
    if not spawn:
        return None
    return (time.time() - (time.perf_counter() - t0_perf)) - float(spawn)


def dry_launch(args, world, rank):
    """`--dry-launch`: the launcher, the rank/shard plumbing, the preallocated all-gather of (B, topk, 32) records and the
    JSON line rehearsed over gloo on CPU tensors - NO GPU is touched and nothing of the hot path runs, so the line is
    marked INVALID and carries no throughput.  Exists so that `bench.py --gpus N` can be tested where there is no N-GPU box."""
    from rtm3d_amd import distributed as rdist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29511')
    dist.init_process_group(backend='gloo', rank=rank, world_size=world)
    B, topk = args.batch, 100
    dev = torch.device('cpu')
    lo, hi, per = rdist.padded_shard(B * world, rank, world)
    assert (lo, hi, per) == (rank * B, rank * B + B, B)
    g = torch.Generator().manual_seed(99 + rank)
    local = torch.rand(B, topk, rdist.RECORD, generator=g)
    local[:, :, 0] = rank                                   # every block names its rank
    out = rdist.gathered_buffer(local)

    def fence():
        dist.barrier()
    for _ in range(args.warmup):
        rdist.all_gather_records(local, always=True, out=out)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        rec = rdist.all_gather_records(local, always=True, out=out)
    fence()
    dt = time.perf_counter() - t0
    dt, multi = multi_diagnostics(world, B, args.steps, dt, rec, local, dev, None, _startup_s(t0))
    multi['block_ranks'] = [int(v) for v in rec.reshape(world, B, topk, rdist.RECORD)[:, 0, 0, 0].tolist()]
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {'records': rec})
        print(json.dumps({'metric': 'images_per_sec', 'value': None, 'unit': 'images/s', 'n_gpus': world, 'steps': args.steps,
                          'warmup': args.warmup, 'ms_per_step': dt / args.steps * 1e3, 'higher_is_better': True, 'scaling': 'weak',
                          'vs_baseline': None, 'dtype': 'fp16', 'data': 'synthetic',
                          'config': {'workload': 'DRY LAUNCH: launcher + gloo all-gather of (%d, %d, 32) records only' % (B, topk),
                                     'global_batch': B * world, 'parallelism': 'dp%d' % world},
                          'INVALID': 'dry launch (gloo, CPU tensors, no hot path): launcher rehearsal only',
                          'multi_gpu': multi}))
    dist.barrier()
    dist.destroy_process_group()


def main():
    args = parse_args()
    launched = 'RANK' in os.environ
    if not launched and (args.gpus > 1 or args.force_launch):
        # BEFORE any GPU call: N fresh rank processes, this one only waits for them.  device_count() does not initialise HIP
        if not args.dry_launch and not args.rehearse_one_gpu:
            have = torch.cuda.device_count()
            if have < args.gpus:
                raise SystemExit('bench.py: --gpus %d but this node shows %d GPUs' % (args.gpus, have))
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.gpus != world:
        # a launcher that started a different number of ranks than the line would claim: refuse, never measure N silently
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d' % (args.gpus, world))
    if args.dry_launch:
        return dry_launch(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU path')
    if args.rehearse_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    # under a launcher (RANK set) the process group is created even for one rank, so that the collective path of the
    # N > 1 runs (RCCL all-gather on the side stream + the diagnostics below) can be rehearsed on a one-GPU box
    use_dist = world > 1 or launched
    if use_dist:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if args.rehearse_one_gpu:
            dist.init_process_group(backend='gloo')
        else:
            dist.init_process_group(backend='nccl', device_id=dev)

    import rtm3d_amd
    from rtm3d_amd import weights, distributed as rdist
    if args.v2_min_tiles is not None:
        from rtm3d_amd import plan as _plan
        _plan.V2_MIN_TILES = args.v2_min_tiles
    if args.no_conv128:
        from rtm3d_amd import plan as _plan
        _plan.USE_CONV128 = False
    for spec in args.bn_tile:
        from rtm3d_amd import plan as _plan
        name, n = spec.rsplit('=', 1)
        _plan.BN_TILE_OVERRIDE[name] = int(n)
    bb = args.backbone
    B, H, W = args.batch, args.height, args.width
    cfg = rtm3d_amd.kitti_config(bb)
    seed, hb = SYNTH.get(bb, (1, -6.0))
    if args.heat_bias is not None:
        hb = args.heat_bias
    sd = weights.synth_state_dict(bb, seed, 'trained', heat_bias=hb)
    if args.zero_weights:
        sd = type(sd)((kk, vv if kk.endswith(('running_var', 'num_batches_tracked')) else torch.zeros_like(vv)) for kk, vv in sd.items())
    model = rtm3d_amd.create_model(cfg).to(dev).eval()
    model.load_state_dict(sd)
    if args.graph:
        model.use_graph = True
    wcache_note = None
    if use_dist and world > 1 and args.shared_weight_cache:
        # Every rank loads the same state dict; folding BatchNorm, composing the neck's 1x1 pairs and packing 30 M weights is
        # ~1.5 s of numpy per rank on the rank's share of the host cores (usable // world threads).  Rank 0 does it once and
        # writes the on-disk weight cache (rtm3d_amd/weight_cache.py, keyed by a digest of the state dict and of the packers);
        # the other ranks build their plans from that file behind a barrier.
        import tempfile
        wdir = os.environ.get('RTM3D_WEIGHT_CACHE_DIR') or os.path.join(tempfile.gettempdir(), 'rtm3d_wcache_%s_%s' % (
            os.environ.get('MASTER_PORT', '0'), os.environ.get('RTM3D_BENCH_SPAWN_T', '0').replace('.', '_')))
        os.environ['RTM3D_WEIGHT_CACHE_DIR'] = wdir
        t_w = time.perf_counter()
        if rank == 0:
            model._plan_for(B, H, W, dev, 'peaks' if args.sparse_heads else 'dense')      # packs and saves
        dist.barrier()
        if rank != 0:
            model._plan_for(B, H, W, dev, 'peaks' if args.sparse_heads else 'dense')      # reads rank 0's file
        wc = model._wcache
        wcache_note = {'dir': wdir, 'rank': rank, 'hits': wc.hits, 'misses': wc.misses, 'plan_build_s': round(time.perf_counter() - t_w, 2)}
    # this rank's shard of the global synthetic batch (image b uses seed 1234+b: rank independent)
    x = weights.synth_images(B, H, W, seed=1234, first=rank * B).to(dev)
    K = torch.as_tensor(np.tile(weights.synth_intrinsics(), (B, 1)), dtype=torch.float64, device=dev)
    topk = int(cfg.DETECTOR.TOPK_CANDIDATES)

    from rtm3d_amd.pipeline import Detect3DPipeline
    pipe = Detect3DPipeline(model, B, dev, gather='always' if use_dist else True, decode3d=not args.diag_no_decode3d, side_cus=args.side_cus,
                            depth=args.depth or None, side_streams=args.side_streams or None, sparse_heads=args.sparse_heads,
                            solver_form=args.solver_form) if not args.serial else None
    if pipe is not None and use_dist:
        pipe.time_gather = True                 # event pair around the collective on the side stream (diagnostics)

    imgs_u8 = None
    if args.from_uint8:
        if pipe is None or (H, W) != (384, 1280):
            raise SystemExit('--from-uint8 needs the pipelined 384x1280 configuration')
        from rtm3d_amd import preprocess
        gen = torch.Generator().manual_seed(4321 + rank)
        imgs_u8 = [torch.randint(0, 256, (360, 1240, 3), generator=gen, dtype=torch.uint8).to(dev) for _ in range(B)]
        if args.from_uint8 == 'once':
            x, _, _ = preprocess.preprocess_batch(imgs_u8, (H, W), cfg.DATASET.MEAN, cfg.DATASET.STD, resize_to=1280)
            imgs_u8 = None
        rhw = preprocess.resized_size(360, 1240, 1280)
        K0 = preprocess.resize_K(weights.synth_intrinsics(), (360, 1240), rhw)
        K0 = preprocess.adjust_K(K0, (W - rhw[1]) // 2, (H - rhw[0]) // 2)
        K = torch.as_tensor(np.tile(K0, (B, 1)), dtype=torch.float64, device=dev)

    def step():
        if imgs_u8 is not None:                     # n1 in front: uint8 images -> Resize + letterbox + normalise -> plan
            i = pipe.submit_uint8(imgs_u8, K, (H, W), resize_to=1280)
            return i, pipe.det[i % pipe.depth]
        if pipe is not None:                        # two-stream pipeline: decode3d(i) overlaps forward(i+1)
            i = pipe.submit(x, K)
            return i, pipe.det[i % pipe.depth]
        det, boxes, _ = model.detect3d(x, K, sparse_heads=args.sparse_heads, solver_form=args.solver_form)
        rec = rdist.pack_records(det.n, det.cls, det.score, det.mproj, det.verts, det.bbox, topk, boxes)
        return rdist.all_gather_records(rec, always=use_dist), det

    # ---- warm-up (also records the plan) and choice of the dominant kernel for the live probe.  The per-op pass runs in every
    # run, plain or --full: the timed steps bracket the op it picks with the probe's events
    rec, det = step()
    torch.cuda.synchronize(dev)
    plan = model._plan_for(B, H, W, dev, 'peaks' if args.sparse_heads else 'dense')
    head_ch = list(model._head_channels)                     # (num_classes, 16, 2, 2) for the rtm3d head table
    outs = [torch.empty(B, c, H // 4, W // 4, dtype=torch.float32, device=dev) for c in (head_ch[:1] if args.sparse_heads else head_ch)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    optrs = [o.data_ptr() for o in outs] + [0] * (4 - len(outs))
    plan.forward_timed(stream, x.data_ptr(), optrs)
    info = plan.forward_timed(stream, x.data_ptr(), optrs)
    peak_info = None
    if args.sparse_heads:
        pk = [t.data_ptr() for t in plan.peak_out] + [0, 0]
        plan.peak.forward_timed(stream, 0, pk)
        peak_info = plan.peak.forward_timed(stream, 0, pk)
    # wall time of the three stages in the REAL replay (side lanes on: the neck's up-sampling chains overlap its top-down chain,
    # which the one-op-after-the-other pass above cannot see): events at the stage boundaries, best of five replays (--full)
    stage_wall = None
    if args.full and not args.sparse_heads:
        nm_ = [i['name'] for i in info]
        first = lambda pred: next((k for k, n in enumerate(nm_) if pred(n)), None)
        marks = [first(lambda n: n.startswith('backbone')), first(lambda n: n.startswith(('kfpn', 'fusion'))), first(lambda n: n.startswith('heads'))]
        if all(m is not None for m in marks) and marks == sorted(marks):
            runs = [plan.forward_marks(stream, x.data_ptr(), optrs, marks) for _ in range(6)][1:]
            stage_wall = dict(zip(('backbone', 'neck', 'heads'), [min(r[k] for r in runs) for k in range(3)]))
    dom = max(range(len(info)), key=lambda i: info[i]['ms'])
    if not args.graph:
        plan.probe_set(dom)
    for _ in range(max(0, args.warmup - 1)):
        step()
    if not args.graph:
        plan.probe_set(dom)                     # reset the probe ring: only timed steps are averaged

    def fence():
        if pipe is not None:
            pipe.drain()
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        rec, det = step()
    fence()
    dt = time.perf_counter() - t0
    last_step = rec
    multi = None
    dom_ms, dom_n = plan.probe_read() if not args.graph else (info[dom]['ms'], 0)
    n_det = det.n.sum().item()
    if pipe is not None:
        rec = pipe.results(rec)
    if use_dist:
        torch.cuda.synchronize(dev)
        local = pipe.rec_local[last_step % pipe.depth] if pipe is not None else rec[rank * B:(rank + 1) * B]
        dt, multi = multi_diagnostics(world, B, args.steps, dt, rec, local, dev, pipe.gather_us(last_step) if pipe is not None else None,
                                      _startup_s(t0))
        if wcache_note is not None:
            notes = [None] * world
            dist.all_gather_object(notes, wcache_note)
            multi['shared_weight_cache'] = {'dir': wcache_note['dir'], 'per_rank': [{k: n[k] for k in ('rank', 'hits', 'misses', 'plan_build_s')} for n in notes],
                                            'note': 'rank 0 folds + packs (misses) and writes the file, ranks >= 1 build their plan from it (hits) behind a barrier'}
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {'records': rec})          # the last timed step's records, before anything else runs

    if rank == 0:
        ms_step = dt / args.steps * 1e3
        total_images = B * world * args.steps
        flops_fwd = plan.plan.total_flops()
        d = info[dom]
        # HBM-side traffic of the dominant kernel: PMC counters cannot be collected live inside a timed
        # run, so the per-launch figure comes from the committed rocprofv3 --pmc profile of this workload
        # (the file says when and on which tree it was collected: a stale figure shows in the line - `traffic_source`,
        # `traffic_age_days`, and `traffic_tree` against `tree` = the kernels' source hash of THIS run)
        traffic, traffic_src, traffic_age, traffic_tree = None, None, None, None
        for prof in ('r06_pmc_heads.json', 'r05_pmc_heads.json', 'r04_pmc_heads.json', 'r03_pmc_heads.json', 'r02_pmc_heads.json', 'r01_pmc_heads.json'):
            try:
                with open(os.path.join(ROOT, 'profiles', prof)) as f:
                    pmc = json.load(f)
                if B == 32 and (H, W) == (384, 1280) and d['name'] in pmc['kernels']:
                    traffic = pmc['kernels'][d['name']]['hbm_bytes_corrected'] / 1e9
                    traffic_tree = pmc.get('csrc_sha1')
                    when = pmc.get('collected_utc')
                    if when:
                        import datetime
                        traffic_age = round((datetime.datetime.utcnow() - datetime.datetime.strptime(when[:19], '%Y-%m-%dT%H:%M:%S')).total_seconds() / 86400.0, 2)
                    traffic_src = 'profiles/%s (GB per launch, (2*FETCH_SIZE+WRITE_SIZE)*1024; collected %s, commit %s, kernel sources %s)' % (
                        prof, when or 'at an unrecorded time (file predates round 5)', pmc.get('commit', 'unrecorded'), (traffic_tree or 'unrecorded')[:12])
                    break
            except (OSError, KeyError, ValueError):
                pass
        roof = {'bound': 'mfma', 'kernel': '%s (%s)' % (d['kernel'], d['name']),
                'achieved': d['flops'] / (dom_ms * 1e-3) / 1e12 if dom_ms > 0 else None,
                'peak': PEAK_FP16_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                'frac': (d['flops'] / (dom_ms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS) if dom_ms > 0 else None,
                'traffic': traffic, 'traffic_source': traffic_src, 'traffic_age_days': traffic_age,
                'traffic_is_of_this_tree': (traffic_tree == csrc_sha1()) if traffic_tree else None,
                'launch_ms': dom_ms, 'launches_timed': dom_n,
                'flops_per_launch': d['flops'],
                'whole_forward_frac': flops_fwd / (sum(i['ms'] for i in info) * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS}
        # north_star's target is quoted on the backbone alone: its ops' algorithmic FLOPs over their hipEvent times (per-op pass)
        bb_ms = sum(i['ms'] for i in info if i['name'].startswith('backbone'))
        bb_fl = sum(i['flops'] for i in info if i['name'].startswith('backbone'))
        if bb_ms > 0:
            roof['backbone_ms'] = bb_ms
            roof['backbone_frac'] = bb_fl / (bb_ms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS
        # the three stages of the forward (per-op hipEvent pass): MFMA fraction of each stage's conv FLOPs, and for the ops that
        # carry no FLOPs (pools, spatial softmax) or whose bytes / time exceeds their flops / time relative to the peaks, HBM
        stages = {}
        for nm, pred in (('backbone', lambda n: n.startswith('backbone')),
                         ('neck', lambda n: n.startswith(('kfpn', 'fusion'))),
                         ('heads', lambda n: n.startswith('heads'))):
            ops = [i for i in info if pred(i['name'])]
            ms = sum(i['ms'] for i in ops)
            if ms <= 0:
                continue
            fl, by = sum(i['flops'] for i in ops), sum(i['bytes'] for i in ops)
            mf, hb = fl / (ms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS, by / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS
            hbm_ms = sum(i['ms'] for i in ops if i['ms'] > 0 and i['bytes'] / PEAK_HBM_GBS / 1e9 > i['flops'] / PEAK_FP16_MFMA_TFLOPS / 1e12)
            stages[nm] = {'ms': round(ms, 4), 'launches': len(ops), 'gflop': round(fl / 1e9, 1), 'frac': round(mf, 4), 'bound': 'mfma',
                          'algorithmic_gb': round(by / 1e9, 3), 'hbm_frac': round(hb, 4),
                          'ms_in_hbm_bound_ops': round(hbm_ms, 4)}
            if stage_wall is not None:
                # `ms` = sum of the ops' own times, one after the other on one stream; `wall_ms` = the stage in the replay the timed
                # steps run (its lanes overlap the launches of independent ops)
                stages[nm]['wall_ms'] = round(stage_wall[nm], 4)
                stages[nm]['frac_wall'] = round(fl / (stage_wall[nm] * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS, 4)
        roof['per_stage'] = stages
        out = {'metric': 'images_per_sec', 'value': total_images / dt, 'unit': 'images/s', 'n_gpus': world,
               'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms_step, 'higher_is_better': True,
               'scaling': 'weak', 'vs_baseline': None, 'dtype': 'fp16', 'data': 'synthetic',
               'config': {'workload': 'rtm3d_%s_kitti forward+decode2d+decode3d, bs=%d/GPU, %dx%d, fp16 storage fp32 accumulate'
                                      % (bb.lower().replace('-', ''), B, H, W),
                          'global_batch': B * world, 'parallelism': 'dp%d' % world,
                          'detections_per_batch_rank0': int(n_det), 'gflop_per_image': flops_fwd / B / 1e9,
                          'solver_form': args.solver_form or _default_solver_form()},
               'roofline': roof, 'multi_gpu': multi}
        # the plan-level A/B switches this process ran with (environment, read once at import: rtm3d_amd/plan.py); the product: all True
        from rtm3d_amd import plan as _p
        out['config']['plan_switches'] = {'FOLD_PROJECT_C128': _p.FOLD_PROJECT_C128, 'FOLD_NECK_UP': _p.FOLD_NECK_UP, 'USE_CONV64S2': _p.USE_CONV64S2,
                                          'S2D_ONLY': _p.S2D_ONLY, 'USE_CONV128': _p.USE_CONV128}
        if not all(out['config']['plan_switches'].values()):
            out['DIAGNOSTIC_plan_switches'] = 'a plan-level A/B switch is off: not the product configuration'
        if args.diag_no_decode3d:
            out['INVALID'] = 'diagnostic run without the 3D decode'
        if args.v2_min_tiles is not None:
            out['DIAGNOSTIC_v2_min_tiles'] = args.v2_min_tiles
        if args.no_conv128:
            out['DIAGNOSTIC_no_conv128'] = True
        if args.bn_tile:
            out['DIAGNOSTIC_bn_tile'] = args.bn_tile
        if args.from_uint8:
            out['config']['input'] = ('B uint8 360x1240x3 images in HBM -> Resize(1280, bilinear) + letterbox + normalise on the device (rtm3d_preprocess_batch, fp16 NHWC4 output) in every step'
                                      if args.from_uint8 == 'step' else 'the same uint8 images preprocessed ONCE outside the timed region into the fp32 NCHW batch fed in every step')
            out['NOTE'] = 'row n1 measurement, not the BASELINE line (whose input is the normalised fp32 batch)'
        if args.sparse_heads:
            out['DIAGNOSTIC_sparse_heads'] = ('detect3d call surface with peaks-only regression heads: heat map dense, offset_fr_main / main_offset at the '
                                              '<= %d peaks per image through a patch plan (not the BASELINE line: Model.forward() returns four dense maps)' % topk)
            out['config']['gflop_per_image_dense_part'] = flops_fwd / B / 1e9
            out['sparse_heads'] = {'patch_plan_ms': round(sum(i['ms'] for i in peak_info), 4),
                                   'patch_plan_gflop_per_batch': round(sum(i['flops'] for i in peak_info) / 1e9, 1),
                                   'ops': [{'name': i['name'], 'kernel': i['kernel'], 'ms': round(i['ms'], 4)} for i in peak_info]}
        if args.rehearse_one_gpu:
            out['INVALID'] = 'rehearsal: %d ranks share ONE GPU and gather over gloo through host memory; not a throughput measurement' % world
        if args.zero_weights:
            out['DIAGNOSTIC'] = 'all-zero weights: every activation is zero (not the benchmark workload)'
        if args.graph:
            out['DIAGNOSTIC_graph'] = 'hipGraph replay; roofline.launch_ms from the per-op pass, not from the timed region'
        if args.heat_bias is not None:
            out['DIAGNOSTIC'] = 'heat-map bias overridden to %g (not the benchmark workload)' % args.heat_bias
        if args.per_op:
            tot = sum(i['ms'] for i in info)
            print('%-28s %-22s %9s %9s %8s' % ('op', 'kernel', 'ms', 'TFLOP/s', 'GB/s'), file=sys.stderr)
            for i in info:
                print('%-28s %-22s %9.3f %9.1f %8.0f' % (i['name'][:28], i['kernel'], i['ms'], i['flops'] / i['ms'] / 1e9 if i['ms'] else 0,
                                                         i['bytes'] / i['ms'] / 1e6 if i['ms'] else 0), file=sys.stderr)
            print('forward total %.3f ms (per-op event timing)' % tot, file=sys.stderr)
        # --full only, after the line's own figures: each of these takes runs of its own (tens of seconds of CPU oracle)
        if args.full and not args.no_cpu_baseline and world == 1:
            out['cpu_baseline'] = cpu_baseline(bb, sd, H, W, cfg, full=args.cpu_full, threads=args.cpu_threads)
        else:
            out['cpu_baseline'] = None
        if args.full and not args.no_parity and world == 1 and not args.from_uint8 and not args.sparse_heads:
            out['parity'] = parity_check(model, cfg, sd, bb, x, args.parity_images, dev, solver_form=args.solver_form)
        else:
            out['parity'] = None
        if (args.full and not args.no_sparse_probe and world == 1 and pipe is not None and not args.sparse_heads and not args.from_uint8
                and not args.diag_no_decode3d and model._head_variant in (None, 'rtm3d')):
            # informational, outside the timed region and never `value`: the same batch through the detect3d call surface with the
            # regression heads evaluated at the detected peaks only (what `bench.py --sparse-heads` times as a DIAGNOSTIC line)
            try:
                sp = Detect3DPipeline(model, B, dev, gather=False, sparse_heads=True)
                for _ in range(3):
                    sp.submit(x, K)
                sp.drain(); torch.cuda.synchronize(dev)
                ns = max(5, min(args.steps, 20))
                t1 = time.perf_counter()
                for _ in range(ns):
                    sp.submit(x, K)
                sp.drain(); torch.cuda.synchronize(dev)
                dts = time.perf_counter() - t1
                out['detect_surface_sparse_heads'] = {'DIAGNOSTIC': 'not the BASELINE metric: Model.forward() and `value` keep four dense logit maps',
                                                      'images_per_s': B * ns / dts, 'ms_per_step': dts / ns * 1e3, 'steps': ns}
            except Exception as e:                 # the probe must never cost the line
                out['detect_surface_sparse_heads'] = {'error': repr(e)[:200]}
        print(json.dumps(out))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
