"""hipEvent times of the optimiser step on one MI355X over the DLA-34 parameter shapes (weights.state_dict_spec: 180 parameters,
29.9 M fp32 elements, 94 floating-point buffers), three hyper classes: the one launch of rtm3d_optim_step through the C entry
point (with and without the EMA), ``Adamax.step`` of rtm3d_amd/optim.py with its host work, and torch.optim.Adamax on the same
device tensors in its default form (foreach) and with foreach=False.  Next to each launch: the bytes the rule must move (28 B
per element, 36 B with the EMA) and the multiple of the time those bytes take at the "4 reads + 1 write" rate of
profiles/r04_hbm_rates.txt (4.44 TB/s at its 2048-workgroup row).  Two steps are first checked against torch's fp64 Adamax on the
same gradients (the bar of tests/test_gpu_optim.py).  Median (min) of 20 timed groups of 10 calls after a warm-up; the working set (0.6 - 1.1 GB) is
larger than every cache.

    python tools/gpu_optim_time.py [FILE] [--lib PATH]

With FILE the table is appended to it (profiles/optim.txt holds its output).  --lib PATH times the launch through another
build of the library as well (e.g. ``make EXTRA=-DOPT_NT_ALL OUT=... OBJ=...``: non-temporal loads for p, m, u, e too)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS, PER = 20, 10
RATE = 4.44e12            # profiles/r04_hbm_rates.txt, "4 reads + 1 write", grid 2048 x 256


def build_model(torch, dev, seed=0):
    from rtm3d_amd import weights
    g = torch.Generator().manual_seed(seed)
    model = torch.nn.Module()
    names, cls = [], {}
    for key, shape, kind, _ in weights.state_dict_spec('DLA-34'):
        name = key.replace('.', '_')
        if kind == 'bn_count':
            model.register_buffer(name, torch.zeros((), dtype=torch.int64))
        elif kind in ('bn_mean', 'bn_var'):
            model.register_buffer(name, torch.rand(shape, generator=g) + 0.5)
        else:
            model.register_parameter(name, torch.nn.Parameter(torch.randn(shape, generator=g) * 0.05))
            names.append(name)
            cls[name] = (0.01, 0.0005) if kind in ('conv', 'deconv') else (0.02, 0.0001) if kind == 'conv_bias' else (0.01, 0.0)
    model.to(dev)
    groups = [{'name': n, 'params': [getattr(model, n)], 'lr': cls[n][0], 'weight_decay': cls[n][1]} for n in names]
    return model, groups


def main():
    import numpy as np
    import torch
    from rtm3d_amd import _lib, optim
    args = sys.argv[1:]
    other = None
    if '--lib' in args:
        i = args.index('--lib')
        other = args[i + 1]
        del args[i:i + 2]
    dev = torch.device('cuda', 0)
    lib = _lib.load()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            f()
        t = []
        for _ in range(GROUPS):
            e0.record()
            for _ in range(PER):
                f()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / PER)
        return float(np.median(t)), float(min(t))

    def fill_grads(params, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        for p in params:
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(torch.randn(p.shape, generator=g, device=dev) * 0.1)

    res, notes = [], []
    elems = None
    for ema in (None, 0.9999):
        model, groups = build_model(torch, dev)
        params = [g['params'][0] for g in groups]
        elems = sum(p.numel() for p in params)
        buf_elems = sum(b.numel() for b in model.buffers() if b.dtype.is_floating_point)
        opt = optim.Adamax(groups)
        if ema is not None:
            e = optim.ModelEMA(model, ema)
            opt.attach_ema(e)
        # agreement: two steps here, in torch fp32 and in torch fp64 on the same gradients; the bar of tests/test_gpu_optim.py
        tmodel, tgroups = build_model(torch, dev)
        tparams = [g['params'][0] for g in tgroups]
        tg = lambda ps: [{'params': [q], 'lr': g['lr'], 'weight_decay': g['weight_decay']} for q, g in zip(ps, tgroups)]
        topt = torch.optim.Adamax(tg(tparams))
        dparams = [torch.nn.Parameter(q.detach().double()) for q in tparams]
        dopt = torch.optim.Adamax(tg(dparams))
        for step in range(2):
            opt.zero_grad()
            fill_grads(params, step)
            fill_grads(tparams, step)
            for q, t in zip(dparams, tparams):
                q.grad = t.grad.double()
            opt.step()
            topt.step()
            dopt.step()
        worst, worst_torch = 0.0, 0.0
        for a, b, d in zip(params, tparams, dparams):
            own = float((b.detach().double() - d.detach()).abs().max())
            bar = max(4.0 * own, 4.0 * float(np.spacing(np.float32(d.detach().abs().max().item()))))
            worst = max(worst, float((a.detach().double() - d.detach()).abs().max()) / bar)
            worst_torch = max(worst_torch, own / bar)
        assert worst <= 1.0, 'the launch leaves the bar around torch\'s fp64 run: %.2f x' % worst
        notes.append('EMA %s: after 2 steps every parameter tensor lies within %.2f of its bar around torch\'s fp64 Adamax (bar: max(4 x torch\'s '
                     'own fp32-vs-fp64 distance, 4 ulp); torch\'s fp32 run: %.2f); %d segments, %d chunks'
                     % ('on' if ema else 'off', worst, worst_torch, opt._tables[0].numel() // 56, opt._tables[2]))
        del dopt, dparams
        seg, chunks, nc = opt._tables
        h = opt._hyper
        stream = _lib.stream_ptr(dev)
        loss = torch.ones((), device=dev)
        tag = 'with the EMA' if ema else 'without the EMA'
        nbytes = (36.0 if ema else 28.0) * elems + (12.0 * buf_elems if ema else 0.0)

        def f_launch(fn=lib.rtm3d_optim_step):
            rc = fn(stream, seg.data_ptr(), chunks.data_ptr(), nc, ctypes.byref(h), loss.data_ptr(), opt._skipped.data_ptr())
            assert rc == 0

        res.append(('rtm3d_optim_step %s, one launch, guard on' % tag, timed(f_launch), nbytes))
        if other:
            olib = ctypes.CDLL(other)
            olib.rtm3d_optim_step.restype, olib.rtm3d_optim_step.argtypes = _lib.SIGNATURES['rtm3d_optim_step']
            res.append(('  the same through %s' % os.path.basename(os.path.dirname(other)), timed(lambda: f_launch(olib.rtm3d_optim_step)), nbytes))
            res.append(('  and once more through the product build', timed(f_launch), nbytes))
        res.append(('Adamax.step(loss) %s, with its host work' % tag, timed(lambda: opt.step(loss)), nbytes))
        if ema is None:
            res.append(('Adamax.zero_grad(): one memset of the gradient arena', timed(opt.zero_grad), 4.0 * elems))
            res.append(('torch.optim.Adamax.step(), default (foreach)', timed(topt.step), None))
            topt1 = torch.optim.Adamax([{'params': g['params'], 'lr': g['lr'], 'weight_decay': g['weight_decay']} for g in tgroups],
                                       foreach=False)
            res.append(('torch.optim.Adamax.step(), foreach=False', timed(topt1.step), None))
            res.append(('torch zero_grad(set_to_none=False)', timed(lambda: topt.zero_grad(set_to_none=False)), None))
        assert opt.skipped() == 0
        del model, opt, tmodel, topt
        torch.cuda.empty_cache()

    lines = ['optimiser step, us per call: median (min) of %d groups of %d back-to-back calls, hipEvent' % (GROUPS, PER),
             'DLA-34 shapes: %d parameters, %d elements, three hyper classes; floor = bytes / %.2f TB/s ("4 reads + 1 write", '
             'profiles/r04_hbm_rates.txt)' % (len(groups), elems, RATE / 1e12)]
    lines += ['  ' + n for n in notes]
    for name, (m, lo), nbytes in res:
        tail = ''
        if nbytes:
            floor = nbytes / RATE * 1e6
            tail = '  %.0f MB, %.2f TB/s, %.2f x the floor of %.0f us' % (nbytes / 1e6, nbytes / m / 1e6, m / floor, floor)
        lines.append('  %-62s %9.1f (%.1f)%s' % (name + ':', m, lo, tail))
    by = {n: t[0] for n, t, _ in res}
    ours = by['Adamax.step(loss) without the EMA, with its host work']
    for n in ('torch.optim.Adamax.step(), default (foreach)', 'torch.optim.Adamax.step(), foreach=False'):
        lines.append('  Adamax.step %.1f us against %s %.1f us: %s' % (ours, n, by[n], 'the launch is %.1fx faster' % (by[n] / ours)
                                                                      if by[n] > ours else 'the launch is NOT faster'))
    print('\n'.join(lines))
    if args:
        with open(args[0], 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
