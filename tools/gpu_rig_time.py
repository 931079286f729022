"""hipEvent times of rtm3d_rig_fuse on one MI355X at C = 6 cameras, topk = 100, for R = 1 and R = 32 rigs, with about 20 kept
boxes per camera (64 objects per rig, each seen by one to three cameras: the scene of tests/rig_cases.py) and with all 100 slots
of every camera kept (200 objects, each seen by every second camera), for each metric, through the C entry point with preallocated
buffers; rtm3d_rig_scatter_ids and one rtm3d_tracks_update on the fused records (B = R, topk = cap = 256, 128 slots, steady
state) next to it for scale.  Median of 20 timed groups of 10 calls after a warm-up.
Every configuration ("step") runs in a fresh child process under its own time limit, one after the other; the first step that
fails, faults or runs out of time ends the run, and nothing more is started.
Prints the table; with an argument, also appends it to that file (profiles/rig.txt holds its output)."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, TOPK, CAP, T, GROUPS, PER = 6, 100, 256, 128, 20, 10
STEP_LIMIT = 120                                   # seconds per step
STEPS = [(R, kept) for R in (1, 32) for kept in ('20', 'all')]


def scene(R, kept, rng):
    import numpy as np
    from tests import rig_cases as rc
    ext = np.stack([rc.ring(C, rng) for _ in range(R)])
    recs = []
    for r in range(R):
        objs = []
        for i in range(64 if kept == '20' else 200):
            cams = rng.choice(C, size=int(rng.integers(1, 4)), replace=False) if kept == '20' else [(i + 2 * m) % C for m in range(3)]
            objs.append(rc.obj(rc.site(i, rng, per_row=16) - np.array([0, 0, 50.0]), dict(zip([int(v) for v in cams], rc.scores(rng, len(cams)))),
                               rng, cls=i % 3))
        recs.append(rc.render(objs, ext[r], TOPK, rng, junk=kept == '20'))
    return np.ascontiguousarray(np.concatenate(recs)), np.ascontiguousarray(ext.reshape(R * C, 12))


def step(R, kept):
    import numpy as np
    import torch
    from rtm3d_amd import _lib, rig, track
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(7))
    rec, ext = scene(R, kept, rng)
    d_rec, d_ext = torch.from_numpy(rec).to(dev), torch.from_numpy(ext).to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = torch.empty(R, CAP, 32, dtype=torch.float32, device=dev)
    box = torch.empty(R, CAP, 7, dtype=torch.float64, device=dev)
    info = torch.empty(R, CAP, 4, dtype=torch.int32, device=dev)
    mp = torch.empty(R * C, TOPK, dtype=torch.int32, device=dev)
    n = torch.empty(R, 2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.rtm3d_rig_workspace_bytes(R, C, TOPK)), dtype=torch.uint8, device=dev)
    ids_cam = torch.empty(R * C, TOPK, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            fn()
        t = []
        for _ in range(GROUPS):
            e0.record()
            for _ in range(PER):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / PER)
        return float(np.median(t)), float(np.min(t))

    kept_per_cam = float(((rec[..., 31] == 2) & (rec[..., 1] >= 0.3)).sum()) / (R * C)
    for metric, thresh in (('bev', 0.1), ('iou3d', 0.05), ('dist', -1.5)):
        p = rig.RigParams(metric=metric, thresh=thresh, min_score=0.3).to_c()
        fuse = lambda: _lib.check(lib.rtm3d_rig_fuse(stream, R, C, TOPK, CAP, d_rec.data_ptr(), d_ext.data_ptr(), ctypes.byref(p), out.data_ptr(),
                                                     box.data_ptr(), info.data_ptr(), mp.data_ptr(), n.data_ptr(), ws.data_ptr()), 'rig_fuse')
        t = timed(fuse)
        nn = n.cpu().numpy()
        print('rig_fuse R=%2d C=%d topk=%d cap=%d, %5.1f kept per camera, %-5s: %7.1f (%.1f); %.1f clusters per rig, %d dropped'
              % (R, C, TOPK, CAP, kept_per_cam, metric, t[0], t[1], nn[:, 0].mean(), int(nn[:, 1].sum())), flush=True)
    trk = track.Tracker(R, T, None, dev)
    tp = trk.params.to_c()
    ids = torch.empty(R, CAP, dtype=torch.int32, device=dev)
    tws = torch.empty(int(lib.rtm3d_tracks_workspace_bytes(R, CAP, T)), dtype=torch.uint8, device=dev)
    upd = lambda: _lib.check(lib.rtm3d_tracks_update(stream, R, CAP, T, out.data_ptr(), 1.0, None, ctypes.byref(tp), trk.state.data_ptr(),
                                                     ids.data_ptr(), tws.data_ptr()), 'tracks_update')
    t = timed(upd)
    print('  tracks_update on the fused records B=%d topk=%d T=%d, 3d (for scale):  %7.1f (%.1f); %d slots tracked'
          % (R, CAP, T, t[0], t[1], int((ids != 0).sum())), flush=True)
    sc = lambda: _lib.check(lib.rtm3d_rig_scatter_ids(stream, R, C, TOPK, CAP, mp.data_ptr(), ids.data_ptr(), ids_cam.data_ptr()), 'rig_scatter_ids')
    t = timed(sc)
    print('  rig_scatter_ids (one launch):                                        %7.1f (%.1f); %d camera slots with an id'
          % (t[0], t[1], int((ids_cam != 0).sum())), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--step':
        step(int(sys.argv[2]), sys.argv[3])
        return 0
    lines = ['rig fusion kernels, us per call (three launches): median (min) of %d groups of %d back-to-back calls, hipEvent' % (GROUPS, PER)]
    print(lines[0], flush=True)
    rc = 0
    for R, kept in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', str(R), kept], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True, timeout=STEP_LIMIT, cwd=ROOT)
        except subprocess.TimeoutExpired as e:
            lines.append('step R=%d kept=%s: no result within %d s; nothing more is started' % (R, kept, STEP_LIMIT))
            print(lines[-1], flush=True)
            print(e.stdout or '', flush=True)
            rc = 124
            break
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(('rig_fuse', '  '))]
        print('\n'.join(got) if r.returncode == 0 else r.stdout, flush=True)
        lines.extend(got)
        if r.returncode != 0:
            lines.append('step R=%d kept=%s ended with status %d; nothing more is started' % (R, kept, r.returncode))
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'a') as f:
            f.write('\n'.join(lines) + '\n')
    return rc


if __name__ == '__main__':
    sys.exit(main())
