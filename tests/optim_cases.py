"""Cases of the optimiser-step tests (tests/test_optim_cpu.py, tests/test_gpu_optim.py) and of the fixture
(tests/golden/make_solver_golden.py).  Deterministic numpy only.

A case is a dict:
    tensors   [{'n', 'lr', 'wd', 'shift'}]: a parameter of n elements in a hyper class (lr, wd); shift = 1, 2, 3 makes it a view
              that starts that many elements into a larger buffer (4, 8, 12 bytes off a 16-byte boundary)
    buffers   [n]: floating-point buffers of the model (EMA-only segments; they need ema)
    betas, eps, ema (decay or None), seed
    grad      'normal' (N(0, 0.1^2) per element and step) or 'zero'
    poke_g    [(tensor, element, step, value)]: gradient elements overwritten at a step (1-based)
    poke_p    [(tensor, element, value)]: initial parameter elements overwritten
The shapes are the smallest at which the launch code can go wrong (chunk = RTM3D_OPTIM_CHUNK), not the network's."""
import numpy as np

from tests import optim_ref as ref

F32 = np.float32
CHUNK = 4096
STEPS = 6
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 3 * CHUNK + 5)
# the reference's three classes: weights (BASE_LR, WEIGHT_DECAY), norm (BASE_LR, 0), bias (BASE_LR * factor, WEIGHT_DECAY_BIAS)
CLASSES3 = ((0.01, 0.0005), (0.01, 0.0), (0.02, 0.0001))
DENORMAL = float(np.float32(1e-41))


def _case(tensors, buffers=(), betas=(0.9, 0.999), eps=1e-8, ema=None, seed=0, grad='normal', poke_g=(), poke_p=()):
    return {'tensors': [dict(t) for t in tensors], 'buffers': list(buffers), 'betas': betas, 'eps': eps, 'ema': ema, 'seed': seed,
            'grad': grad, 'poke_g': list(poke_g), 'poke_p': list(poke_p)}


def _t(n, cls=0, shift=0, classes=CLASSES3):
    return {'n': n, 'lr': classes[cls][0], 'wd': classes[cls][1], 'shift': shift}


def make(name):
    if name == 'sizes':                       # every size around the vector width, the wave, the workgroup and the chunk; 3 classes; EMA
        return _case([_t(n, i % 3) for i, n in enumerate(SIZES)], ema=0.9999, seed=1)
    if name == 'sizes_noema':
        return _case([_t(n, i % 3) for i, n in enumerate(SIZES)], seed=1)
    if name == 'many':                        # more chunks than workgroups: 300 tensors of 1 .. 16 elements
        rng = np.random.default_rng(2)
        return _case([_t(int(n), i % 3) for i, n in enumerate(rng.integers(1, 17, 300))], ema=0.999, seed=2)
    if name == 'views':                       # the scalar path next to the 16-byte path
        ts = [_t(n, i % 3, shift) for i, (n, shift) in enumerate(((5, 1), (300, 2), (CHUNK + 7, 3), (300, 0), (CHUNK + 7, 0), (1, 3), (4, 1)))]
        return _case(ts, ema=0.9999, seed=3)
    if name == 'views_noema':
        ts = [_t(n, i % 3, shift) for i, (n, shift) in enumerate(((5, 1), (300, 2), (CHUNK + 7, 3), (300, 0), (1, 3)))]
        return _case(ts, seed=3)
    if name == 'beta_lo':                     # w = 0.7 >= 0.5: the other lerp branch
        return _case([_t(n, i % 3) for i, n in enumerate((5, 257, CHUNK + 1))], betas=(0.3, 0.999), ema=0.9999, seed=4)
    if name == 'lr0':
        return _case([{'n': 257, 'lr': 0.0, 'wd': 0.0005, 'shift': 0}, {'n': 5, 'lr': 0.0, 'wd': 0.0, 'shift': 0}], ema=0.9999, seed=5)
    if name == 'zero_grad':                   # u1 = eps at the first step, m stays 0
        return _case([_t(n, i % 3) for i, n in enumerate((5, 257))], grad='zero', seed=6)
    if name == 'denormal':                    # a denormal gradient (wd = 0: it reaches m and u as it is) and a denormal parameter
        return _case([_t(9, 1), _t(260, 0)], ema=0.9999, seed=7,
                     poke_g=[(0, 2, s, DENORMAL) for s in range(1, STEPS + 1)] + [(1, 258, 1, -DENORMAL)],
                     poke_p=[(0, 5, DENORMAL), (1, 3, -DENORMAL)])
    if name == 'nonfinite':                   # one NaN and one Inf gradient element, each at one step
        return _case([_t(9, 1), _t(260, 0)], ema=0.9999, seed=8, poke_g=[(0, 4, 2, float('nan')), (1, 129, 3, float('inf'))])
    if name == 'buffers':                     # EMA-only segments: floating-point buffers, aligned sizes and tails
        return _case([_t(64, 0), _t(64, 1)], buffers=(64, 3, CHUNK + 1), ema=0.99, seed=9)
    raise KeyError(name)


GPU_CASES = ('sizes', 'sizes_noema', 'many', 'views', 'views_noema', 'beta_lo', 'lr0', 'zero_grad', 'denormal', 'nonfinite', 'buffers')


def initial(case):
    """-> (parameters, buffers): lists of fp32 arrays."""
    rng = np.random.default_rng([case['seed'], 0])
    ps = [rng.standard_normal(t['n']).astype(F32) for t in case['tensors']]
    bs = [rng.standard_normal(n).astype(F32) for n in case['buffers']]
    for i, j, v in case['poke_p']:
        ps[i][j] = v
    return ps, bs


def grads(case, step):
    """The gradients of step 1, 2, ...: a list of fp32 arrays."""
    rng = np.random.default_rng([case['seed'], step])
    gs = [(rng.standard_normal(t['n']) * 0.1).astype(F32) for t in case['tensors']]
    if case['grad'] == 'zero':
        gs = [np.zeros_like(g) for g in gs]
    for i, j, s, v in case['poke_g']:
        if s == step:
            gs[i][j] = v
    return gs


def buffers_at(case, step):
    """The model's floating-point buffers as the forward pass of ``step`` leaves them (stand-in for BatchNorm statistics)."""
    rng = np.random.default_rng([case['seed'], 1000 + step])
    return [rng.standard_normal(n).astype(F32) for n in case['buffers']]


def restate(case, steps=STEPS, losses=None, dt=F32):
    """Run the restatement: -> a list, per step, of {'p', 'm', 'u', 'e', 'eb'} (lists of arrays; e, eb are None without an EMA;
    eb are the buffers' averages).  ``losses``: per step None or a value; a NaN / Inf value skips the step's update - the counts
    t and n advance all the same."""
    ps, bs = initial(case)
    ps = [p.astype(dt) for p in ps]
    ms, us = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    es = [p.copy() for p in ps] if case['ema'] is not None else None
    ebs = [b.astype(dt) for b in bs] if case['ema'] is not None else None
    out = []
    for t in range(1, steps + 1):
        loss = None if losses is None else losses[t - 1]
        if loss is None or np.isfinite(loss):
            gs = [g.astype(dt) for g in grads(case, t)]
            for i, tn in enumerate(case['tensors']):
                k = ref.scalars(tn['lr'], tn['wd'], case['betas'], case['eps'], t, dt)
                ps[i], ms[i], us[i] = ref.update(ps[i], gs[i], ms[i], us[i], k)
            if es is not None:
                d, omd = ref.ema_scalars(case['ema'], t, dt)
                es = [ref.ema(e, p, d, omd) for e, p in zip(es, ps)]
                ebs = [ref.ema(e, b.astype(dt), d, omd) for e, b in zip(ebs, buffers_at(case, t))]
        out.append({'p': [a.copy() for a in ps], 'm': [a.copy() for a in ms], 'u': [a.copy() for a in us],
                    'e': None if es is None else [a.copy() for a in es], 'eb': None if ebs is None else [a.copy() for a in ebs]})
    return out


_cache = {}


def restated(name):
    """The fp32 restatement of a named case over STEPS steps, computed once and read only."""
    if name not in _cache:
        r = restate(make(name))
        for s in r:
            for v in s.values():
                for a in v or ():
                    a.setflags(write=False)
        _cache[name] = r
    return _cache[name]


# ---- the fixture's trajectories: torch.optim.Adamax itself, fp32 and fp64 (tests/golden/optim_cases.npz)
FIXTURE_STEPS, FIXTURE_RECORD = 30, (1, 6, 30)
FIXTURE_CASES = ('fx_plain', 'fx_decay', 'fx_beta_lo')


def make_fixture(name):
    sizes = (1, 5, 257, 1500)
    if name == 'fx_plain':                    # torch's defaults, no weight decay
        return _case([{'n': n, 'lr': 0.002, 'wd': 0.0, 'shift': 0} for n in sizes], seed=11)
    if name == 'fx_decay':                    # the reference's three classes
        return _case([_t(n, i % 3) for i, n in enumerate(sizes)], seed=12)
    if name == 'fx_beta_lo':
        return _case([_t(n, i % 3) for i, n in enumerate((5, 300))], betas=(0.3, 0.99), seed=13)
    raise KeyError(name)


def ulp_floor(a):
    """4 fp32 ulp of the largest finite magnitude of a tensor."""
    a = np.abs(np.asarray(a, np.float64))
    a = a[np.isfinite(a)]
    return 4.0 * float(np.spacing(F32(a.max(initial=0.0))))


def trajectory_bar(g, name, i, step):
    """The bar of tensor i of a fixture case after ``step``: (torch's fp64 values, torch's own fp32-vs-fp64 distance, the bar
    max(4 x that distance, 4 ulp of the tensor's largest magnitude))."""
    t32, t64 = g['%s/p32_%d_%d' % (name, step, i)], g['%s/p64_%d_%d' % (name, step, i)]
    d = float(np.abs(t32.astype(np.float64) - t64).max(initial=0.0))
    return t64, d, max(4.0 * d, ulp_floor(t64))


# ---- the facade's fixture: a tiny module with conv, norm and bias names, an excluded scope and a frozen parameter
SCHED = {'warmup_iters': 5, 'milestones': (8, 12), 'max_iters': 20, 'iterations': 24, 'resume_at': 10, 'warmup_factor': 0.001, 'gamma': 0.1}
SCHED_RUNS = tuple((name, method) for name in ('WarmupMultiStepLR', 'WarmupCosineLR') for method in ('linear', 'constant'))


def tiny_module():
    import torch
    torch.manual_seed(0)

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 3, 1)
            self.norm = torch.nn.BatchNorm2d(3)

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(2, 3, 3)
            self.norm = torch.nn.BatchNorm2d(3)
            self.block = Block()
            self.frozen = torch.nn.Linear(2, 2)
            self.fc = torch.nn.Linear(3, 2)
            self.fc.weight.requires_grad_(False)

    return Tiny()


def solver_config(scheduler='WarmupMultiStepLR', method='linear'):
    """A namespace with the SOLVER keys the reference reads (build_optimizer, build_lr_scheduler)."""
    import types
    return types.SimpleNamespace(SOLVER=types.SimpleNamespace(
        BASE_LR=0.01, WEIGHT_DECAY=0.0005, WEIGHT_DECAY_NORM=0.0, BIAS_LR_FACTOR=2.0, WEIGHT_DECAY_BIAS=0.0001, EXCLUDE_SCOPE=('frozen',),
        LR_SCHEDULER_NAME=scheduler, STEPS=SCHED['milestones'], GAMMA=SCHED['gamma'], MAX_ITER=SCHED['max_iters'],
        WARMUP_FACTOR=SCHED['warmup_factor'], WARMUP_ITERS=SCHED['warmup_iters'], WARMUP_METHOD=method))
