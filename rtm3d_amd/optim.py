"""The optimiser stage of a training loop on the device: the reference's ``solver.step(loss)`` as one HIP launch.

    solver = Solver(model, cfg, ema=0.9999)          # reference: Solver(model, cfg)
    ...
    loss, items = rtm3d_loss(pred, targets)
    solver.step(loss)                                 # zero_grad, backward, Adamax + EMA + guard (one launch), scheduler

The rule is written out in include/rtm3d_hip.h ("optimiser step") and restated in numpy in tests/optim_ref.py; the kernel is
csrc/optim.hip.  ``param_groups`` is the reference's build_optimizer rule, ``WarmupMultiStepLR`` / ``WarmupCosineLR`` its two
schedules in plain Python floats, ``Adamax`` the update over three flat device arenas (gradients, first moment, infinity norm)
with torch's state_dict layout, ``ModelEMA`` the weight average kept in a fourth arena and updated by the same launch.  "Solver"
elsewhere in this package is the L-BFGS-B 3D fit; the facade keeps the reference's class name because that is what a reference
train.py constructs.

Deviations from the reference, all documented where they act:
  * a non-finite loss skips the step on the device and counts it (``Solver.skipped()``); the reference tests the loss on the host
    each step and ends training;
  * a parameter whose ``.grad`` is None at ``step`` takes a zero gradient (its moments decay, weight decay applies); torch skips it;
  * ``zero_grad()`` clears and keeps the gradients (torch's ``set_to_none=False``) - every ``p.grad`` is a view of ``grad_arena``;
  * betas and eps are one pair for all groups (per-group values are refused on load);
  * ``Solver.load_state_dict`` takes the reference's extra scheduler step but not its ``optimizer.step()``, which is a no-op there
    (no gradient exists yet) and would not be one here.

Device tensors only; there is no CPU path."""
import ctypes
import math
from bisect import bisect_right
from collections import Counter

import torch

from . import _lib

# the reference's SOLVER defaults (models/configs/detault.py:43-72) for keys a cfg does not carry
SOLVER_DEFAULTS = {
    'LR_SCHEDULER_NAME': 'WarmupMultiStepLR', 'BASE_LR': 0.01, 'WEIGHT_DECAY': 0.0005, 'WEIGHT_DECAY_NORM': 0.0,
    'GAMMA': 0.1, 'STEPS': (20000, 50000), 'WARMUP_FACTOR': 1.0 / 1000, 'WARMUP_ITERS': 1000, 'WARMUP_METHOD': 'linear',
    'EXCLUDE_SCOPE': (), 'BIAS_LR_FACTOR': 1.0, 'WEIGHT_DECAY_BIAS': 0.0005,
}
MAX_CLASSES = 16
CHUNK = 4096                               # RTM3D_OPTIM_CHUNK
KIND_UPDATE_EMA, KIND_UPDATE, KIND_EMA = 0, 1, 2
_ALIGN = 4                                 # arena slices start at multiples of 4 elements = 16 bytes


def _solver_cfg(cfg, key):
    """cfg.SOLVER.<key> of a CfgNode, a namespace or a dict; the reference's default where the key (or the node) is missing."""
    sub = cfg.get('SOLVER') if cfg is not None and hasattr(cfg, 'get') else getattr(cfg, 'SOLVER', None)
    if sub is not None:
        v = sub.get(key) if hasattr(sub, 'get') else getattr(sub, key, None)
        if v is not None:
            return v
    if key not in SOLVER_DEFAULTS:
        raise ValueError('rtm3d_amd.optim: cfg.SOLVER.%s is not set and the reference has no default for it' % key)
    return SOLVER_DEFAULTS[key]


def param_groups(cfg, model):
    """The reference's build_optimizer rule: one group {name, params: [p], lr, weight_decay} per trainable parameter outside
    SOLVER.EXCLUDE_SCOPE, in named_parameters() order."""
    groups = []
    exclude = tuple(_solver_cfg(cfg, 'EXCLUDE_SCOPE'))
    base_lr = _solver_cfg(cfg, 'BASE_LR')
    for name, p in model.named_parameters():
        if not p.requires_grad or any(name.startswith(s) for s in exclude):
            continue
        lr, wd = base_lr, _solver_cfg(cfg, 'WEIGHT_DECAY')
        if name.endswith('norm.weight') or name.endswith('norm.bias'):
            wd = _solver_cfg(cfg, 'WEIGHT_DECAY_NORM')
        elif name.endswith('.bias'):
            lr, wd = base_lr * _solver_cfg(cfg, 'BIAS_LR_FACTOR'), _solver_cfg(cfg, 'WEIGHT_DECAY_BIAS')
        groups.append({'name': name, 'params': [p], 'lr': lr, 'weight_decay': wd})
    return groups


# ---------------------------------------------------------------------------------------------------- schedules
def _warmup_factor(method, it, warmup_iters, warmup_factor):
    if it >= warmup_iters:
        return 1.0
    if method == 'constant':
        return warmup_factor
    if method == 'linear':
        alpha = it / warmup_iters
        return warmup_factor * (1 - alpha) + alpha
    raise ValueError('rtm3d_amd.optim: warm-up method %r is neither "constant" nor "linear"' % (method,))


class _WarmupLR:
    """What the two schedules share with torch's scheduler base: base_lrs from the groups' initial_lr, last_epoch (an iteration
    count), one step at construction, ``step()`` writes every group's 'lr'."""

    def __init__(self, optimizer, warmup_factor, warmup_iters, warmup_method, last_epoch):
        self.optimizer = optimizer
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        if last_epoch == -1:
            for g in optimizer.param_groups:
                g.setdefault('initial_lr', g['lr'])
        self.base_lrs = [g['initial_lr'] for g in optimizer.param_groups]
        self.last_epoch = last_epoch
        self.step()

    def _warm(self):
        return _warmup_factor(self.warmup_method, self.last_epoch, self.warmup_iters, self.warmup_factor)

    def step(self):
        self.last_epoch += 1
        self._last_lr = self.get_lr()
        for g, lr in zip(self.optimizer.param_groups, self._last_lr):
            g['lr'] = lr

    def get_last_lr(self):
        return self._last_lr

    def state_dict(self):
        return {'last_epoch': self.last_epoch}

    def load_state_dict(self, state):
        """As torch: the count is taken, the groups' 'lr' change at the next step()."""
        self.last_epoch = int(state['last_epoch'])


class WarmupMultiStepLR(_WarmupLR):
    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=0.001, warmup_iters=1000, warmup_method='linear', last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError('rtm3d_amd.optim.WarmupMultiStepLR: the milestones %r do not increase' % (milestones,))
        self.milestones, self.gamma = milestones, gamma
        super().__init__(optimizer, warmup_factor, warmup_iters, warmup_method, last_epoch)

    def get_lr(self):
        warm = self._warm()
        return [base * warm * self.gamma ** bisect_right(self.milestones, self.last_epoch) for base in self.base_lrs]


class WarmupCosineLR(_WarmupLR):
    def __init__(self, optimizer, max_iters, warmup_factor=0.001, warmup_iters=1000, warmup_method='linear', last_epoch=-1):
        self.max_iters = max_iters
        super().__init__(optimizer, warmup_factor, warmup_iters, warmup_method, last_epoch)

    def get_lr(self):
        warm = self._warm()
        return [base * warm * 0.5 * (1.0 + math.cos(math.pi * self.last_epoch / self.max_iters)) for base in self.base_lrs]


def build_lr_scheduler(cfg, optimizer):
    name = _solver_cfg(cfg, 'LR_SCHEDULER_NAME')
    kw = dict(warmup_factor=_solver_cfg(cfg, 'WARMUP_FACTOR'), warmup_iters=_solver_cfg(cfg, 'WARMUP_ITERS'),
              warmup_method=_solver_cfg(cfg, 'WARMUP_METHOD'))
    if name == 'WarmupMultiStepLR':
        return WarmupMultiStepLR(optimizer, _solver_cfg(cfg, 'STEPS'), _solver_cfg(cfg, 'GAMMA'), **kw)
    if name == 'WarmupCosineLR':
        return WarmupCosineLR(optimizer, _solver_cfg(cfg, 'MAX_ITER'), **kw)
    raise ValueError('rtm3d_amd.optim: SOLVER.LR_SCHEDULER_NAME %r is neither WarmupMultiStepLR nor WarmupCosineLR' % (name,))


# ---------------------------------------------------------------------------------------------------- arenas
def _check_tensor(t, what):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('rtm3d_amd.optim: %s must be a contiguous fp32 device tensor (got %s, %s%s)'
                         % (what, t.dtype, t.device, '' if t.is_contiguous() else ', not contiguous'))


def _offsets(sizes):
    """Start of each slice in a flat arena (multiples of 4 elements, so every slice is 16-byte aligned) and the arena's length."""
    offs, at = [], 0
    for n in sizes:
        offs.append(at)
        at += (n + _ALIGN - 1) // _ALIGN * _ALIGN
    return offs, max(at, _ALIGN)


class ModelEMA:
    """The reference's weight average (models/nets/module.py, ModelEMA) as one flat device arena that the optimiser's launch
    updates: e = e * d + (1 - d) * p with d = decay * (1 - exp(-updates / 2000)), over every floating-point entry of
    ``model.state_dict()`` (parameters after their update; buffers such as BatchNorm's running statistics as they are).
    Integer buffers keep the value they had at construction, as in the reference."""

    def __init__(self, model, decay=0.9999):
        self.decay_base = float(decay)
        self.updates = 0
        sd = model.state_dict(keep_vars=True)
        self._keys = list(sd.keys())
        self._float = [(k, v) for k, v in sd.items() if v.dtype.is_floating_point]
        for k, v in self._float:
            _check_tensor(v, 'state_dict entry %r' % k)
        self._other = {k: v.detach().clone() for k, v in sd.items() if not v.dtype.is_floating_point}
        offs, total = _offsets([v.numel() for _, v in self._float])
        dev = self._float[0][1].device if self._float else None
        self.arena = torch.zeros(total, dtype=torch.float32, device=dev)
        self._views = {}
        with torch.no_grad():
            for (k, v), o in zip(self._float, offs):
                self._views[k] = self.arena[o:o + v.numel()].view(v.shape)
                self._views[k].copy_(v)

    def decay(self, n):
        return self.decay_base * (1 - math.exp(-n / 2000))

    def tensors(self):
        """[(key, live model tensor, EMA view)] of the floating-point entries."""
        return [(k, v, self._views[k]) for k, v in self._float]

    def state_dict(self):
        """Keyed like model.state_dict(); the floating-point values are views into the arena."""
        return {k: (self._views[k] if k in self._views else self._other[k]) for k in self._keys}

    def copy_to(self, model):
        """Copy the average into ``model`` (same architecture)."""
        model.load_state_dict(self.state_dict())
        return model


class Adamax:
    """torch.optim.Adamax's rule over every parameter in one launch (csrc/optim.hip).  ``groups`` is a list of
    {params: [p, ...], lr, weight_decay, ...} dicts or an iterable of parameters (then ``lr`` / ``weight_decay`` apply)."""

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8, *, lr=0.002, weight_decay=0.0):
        groups = list(groups)
        if not groups:
            raise ValueError('rtm3d_amd.optim.Adamax: no parameters')
        if not isinstance(groups[0], dict):
            groups = [{'params': groups}]
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0.0:
            raise ValueError('rtm3d_amd.optim.Adamax: betas %r / eps %r out of range' % (betas, eps))
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.param_groups, self._params, self._group_of = [], [], []
        seen = set()
        for gi, g in enumerate(groups):
            g = dict(g)
            ps = [g['params']] if isinstance(g['params'], torch.Tensor) else list(g['params'])
            for p in ps:
                _check_tensor(p, 'a parameter')
                if id(p) in seen:
                    raise ValueError('rtm3d_amd.optim.Adamax: a parameter appears in more than one group')
                seen.add(id(p))
                self._params.append(p)
                self._group_of.append(gi)
            g['params'] = ps
            g.setdefault('lr', lr)
            g.setdefault('weight_decay', weight_decay)
            for k, v in (('betas', self.betas), ('eps', self.eps), ('foreach', None), ('maximize', False), ('differentiable', False),
                         ('capturable', False)):
                g.setdefault(k, v)
            self.param_groups.append(g)
        self.device = self._params[0].device
        if any(p.device != self.device for p in self._params):
            raise ValueError('rtm3d_amd.optim.Adamax: parameters on more than one device')
        sizes = [p.numel() for p in self._params]
        self._offs, total = _offsets(sizes)
        self.grad_arena = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._m = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._u = torch.zeros(total, dtype=torch.float32, device=self.device)
        cut = lambda a: [a[o:o + n].view(p.shape) for o, n, p in zip(self._offs, sizes, self._params)]
        self._grad_views, self._m_views, self._u_views = cut(self.grad_arena), cut(self._m), cut(self._u)
        self._skipped = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._t = 0
        self._ema = None
        self._assign = None                     # hyper class per group, as planned
        self._tables = None
        self._hyper = _lib.OptimHyperC()

    # ---- gradients
    def _point_grads(self):
        """Before the launch: every p.grad is its view of the arena.  A missing gradient is a zero gradient (torch would skip the
        parameter), a foreign one is copied in."""
        for p, v in zip(self._params, self._grad_views):
            g = p.grad
            if g is v:
                continue
            if g is None:
                v.zero_()
            elif g.data_ptr() != v.data_ptr() or g.shape != v.shape or g.dtype != v.dtype or not g.is_contiguous():
                v.copy_(g)                       # a foreign gradient: into its view
            p.grad = v

    def zero_grad(self, set_to_none=False):
        """One memset of the gradient arena; every p.grad is (again) its view of the arena.  ``set_to_none=True`` is refused: the
        views are what lets one launch read every gradient."""
        if set_to_none:
            raise ValueError('rtm3d_amd.optim.Adamax.zero_grad: gradients live in grad_arena and are cleared, not dropped')
        self.grad_arena.zero_()
        for p, v in zip(self._params, self._grad_views):
            if p.grad is not v:
                p.grad = v

    # ---- the plan
    def attach_ema(self, ema):
        """Update ``ema`` (a ModelEMA of the same model) in the launch of every step."""
        self._ema, self._assign = ema, None

    def _classes(self):
        pairs, assign = {}, []
        for g in self.param_groups:
            assign.append(pairs.setdefault((float(g['lr']), float(g['weight_decay'])), len(pairs)))
        if len(pairs) > MAX_CLASSES:
            raise ValueError('rtm3d_amd.optim.Adamax: %d distinct (lr, weight_decay) pairs; one launch takes %d hyper classes'
                             % (len(pairs), MAX_CLASSES))
        return list(pairs.keys()), assign

    def _plan(self, assign):
        lib = _lib.load()
        segs = []
        ema_view = {}
        if self._ema is not None:
            ema_view = {live.data_ptr(): e for _, live, e in self._ema.tensors() if live.numel()}
        mine = set()
        for p, gi, gv, mv, uv in zip(self._params, self._group_of, self._grad_views, self._m_views, self._u_views):
            e = ema_view.get(p.data_ptr()) if p.numel() else None
            mine.add(p.data_ptr())
            segs.append((p.data_ptr(), gv.data_ptr(), mv.data_ptr(), uv.data_ptr(), e.data_ptr() if e is not None else None, p.numel(),
                         KIND_UPDATE_EMA if e is not None else KIND_UPDATE, assign[gi]))
        if self._ema is not None:                # what the optimiser does not update: frozen parameters, floating-point buffers
            for _, live, e in self._ema.tensors():
                if live.numel() and live.data_ptr() not in mine:
                    segs.append((live.data_ptr(), None, None, None, e.data_ptr(), live.numel(), KIND_EMA, 0))
        n = len(segs)
        c_segs = (_lib.OptimSegmentC * n)(*[_lib.OptimSegmentC(*s) for s in segs])
        sizes = (ctypes.c_longlong * n)(*[s[5] for s in segs])
        sb, cb, nc = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
        _lib.check(lib.rtm3d_optim_table_bytes(n, sizes, ctypes.byref(sb), ctypes.byref(cb), ctypes.byref(nc)), 'optim_table_bytes')
        seg_tab = (_lib.OptimSegmentC * n)()
        chunk_tab = (_lib.OptimChunkC * max(nc.value, 1))()
        _lib.check(lib.rtm3d_optim_plan(n, c_segs, seg_tab, chunk_tab, ctypes.byref(nc)), 'optim_plan')
        up = lambda buf, nbytes: torch.frombuffer(bytearray(ctypes.string_at(buf, nbytes)), dtype=torch.uint8).to(self.device)
        self._tables = (up(seg_tab, sb.value), up(chunk_tab, max(cb.value, 8)), nc.value)
        self._assign = assign

    # ---- the step
    def step(self, loss=None):
        """One launch.  ``loss``: a scalar fp32 device tensor whose value guards the step (NaN or +-Inf: nothing is written, the
        skipped counter goes up by one), or None (always update).  Never synchronises."""
        lib = _lib.load()
        self._point_grads()
        classes, assign = self._classes()
        if assign != self._assign:
            self._plan(assign)
        self._t += 1
        b1 = self.betas[0]
        h = self._hyper
        for c, (lr, wd) in enumerate(classes):
            h.nclr[c] = -(lr / (1 - b1 ** self._t))
            h.wd[c] = wd
        h.w, h.beta2, h.eps = 1 - b1, self.betas[1], self.eps
        if self._ema is not None:
            self._ema.updates += 1
            d = self._ema.decay(self._ema.updates)
            h.ema_d, h.ema_omd = d, 1.0 - d
        guard = None
        if loss is not None:
            guard = loss.detach()
            if guard.numel() != 1 or not guard.is_cuda:
                raise ValueError('rtm3d_amd.optim.Adamax.step: the guard is one scalar on the device')
            if guard.dtype != torch.float32:
                guard = guard.float()
        seg, chunks, nc = self._tables
        if nc:
            _lib.check(lib.rtm3d_optim_step(_lib.stream_ptr(self.device), seg.data_ptr(), chunks.data_ptr(), nc, ctypes.byref(h),
                                            guard.data_ptr() if guard is not None else None, self._skipped.data_ptr()), 'optim_step')

    def skipped(self):
        """The number of steps the guard skipped (reads the device counter: one synchronisation)."""
        return int(self._skipped.item())

    # ---- torch's Adamax layout
    def state_dict(self):
        """{'state': {i: {step, exp_avg, exp_inf}}, 'param_groups': [...]} as torch.optim.Adamax writes it; exp_avg / exp_inf are
        views of the arenas (torch.save or copy.deepcopy to keep a snapshot)."""
        state = {}
        if self._t:
            for i, (mv, uv) in enumerate(zip(self._m_views, self._u_views)):
                state[i] = {'step': torch.tensor(float(self._t)), 'exp_avg': mv, 'exp_inf': uv}
        groups, at = [], 0
        for g in self.param_groups:
            out = {k: v for k, v in g.items() if k != 'params'}
            out['params'] = list(range(at, at + len(g['params'])))
            at += len(g['params'])
            groups.append(out)
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        groups, state = sd['param_groups'], sd['state']
        if len(groups) != len(self.param_groups) or any(len(a['params']) != len(b['params']) for a, b in zip(groups, self.param_groups)):
            raise ValueError('rtm3d_amd.optim.Adamax.load_state_dict: the groups do not match this optimiser\'s')
        for g in groups:
            if tuple(g.get('betas', self.betas)) != self.betas or g.get('eps', self.eps) != self.eps or g.get('maximize', False):
                raise ValueError('rtm3d_amd.optim.Adamax.load_state_dict: betas / eps differ from this optimiser\'s (one pair serves '
                                 'every group), or maximize is set')
        order = [i for g in groups for i in g['params']]
        steps = set()
        for i in order:
            if i in state:
                steps.add(float(state[i]['step']))
        if len(steps) > 1 or (steps and any(i not in state for i in order)):
            raise ValueError('rtm3d_amd.optim.Adamax.load_state_dict: the parameters are at different steps (%s) or some have no '
                             'state; one count serves every parameter here' % sorted(steps))
        t = steps.pop() if steps else 0.0
        if t != int(t) or t < 0:
            raise ValueError('rtm3d_amd.optim.Adamax.load_state_dict: step %r' % t)
        with torch.no_grad():
            self._m.zero_()
            self._u.zero_()
            for k, i in enumerate(order):
                if i in state:
                    self._m_views[k].copy_(state[i]['exp_avg'])
                    self._u_views[k].copy_(state[i]['exp_inf'])
        self._t = int(t)
        for mine, theirs in zip(self.param_groups, groups):
            mine.update({k: v for k, v in theirs.items() if k != 'params'})


class Solver:
    """The reference's Solver (solver/Solver.py) on the device: ``step(loss)``, ``learn_rate``, ``optimizer``, ``scheduler``,
    ``solver_name``, ``state_dict`` / ``load_state_dict`` with its three keys; plus ``skipped()`` and, with ``ema=decay``, ``ema``."""

    def __init__(self, model, cfg, ema=None):
        self._optimizer = Adamax(param_groups(cfg, model))
        self._scheduler = build_lr_scheduler(cfg, self._optimizer)
        if ema is not None:
            self.ema = ModelEMA(model, 0.9999 if ema is True else float(ema))
            self._optimizer.attach_ema(self.ema)
        # which group's lr to report: the reference's heuristic
        gs = self._optimizer.param_groups
        largest = max(len(g['params']) for g in gs)
        if largest == 1:
            lr = Counter(g['lr'] for g in gs).most_common()[0][0]
            self._best_param_group_id = next(i for i, g in enumerate(gs) if g['lr'] == lr)
        else:
            self._best_param_group_id = next(i for i, g in enumerate(gs) if len(g['params']) == largest)

    @property
    def solver_name(self):
        return type(self._optimizer).__name__ + '_' + type(self._scheduler).__name__

    @property
    def optimizer(self):
        return self._optimizer

    @property
    def scheduler(self):
        return self._scheduler

    @property
    def learn_rate(self):
        return self._optimizer.param_groups[self._best_param_group_id]['lr']

    def skipped(self):
        return self._optimizer.skipped()

    def step(self, loss):
        """``loss``: a tensor (its mean is the objective) or a dict of tensors (the sum of their means), as the reference's step
        takes them.  Clears the gradients, runs backward, the launch and the scheduler; returns the objective.  No synchronisation."""
        if torch.is_tensor(loss):
            total = loss.mean()
        elif isinstance(loss, dict):
            total = sum(v.mean() for v in loss.values())
        else:
            raise TypeError('rtm3d_amd.optim.Solver.step: a loss tensor or a dict of loss tensors, not %s' % type(loss).__name__)
        self._optimizer.zero_grad()
        total.backward()
        self._optimizer.step(total)              # the objective's own address is the guard: no host test of the loss
        self._scheduler.step()
        return total

    def state_dict(self):
        return {'best_param_group_id': self._best_param_group_id, 'optimizer': self._optimizer.state_dict(),
                'scheduler': {'last_epoch': self._scheduler.last_epoch}}

    def load_state_dict(self, state_dict):
        """The reference's load: its keys are popped from ``state_dict``, and a loaded scheduler takes one step at once
        (solver/Solver.py:58-63) - a resumed run is one iteration ahead in its schedule, there and here."""
        self._best_param_group_id = state_dict.pop('best_param_group_id', self._best_param_group_id)
        if 'optimizer' in state_dict:
            self._optimizer.load_state_dict(state_dict.pop('optimizer'))
        if 'scheduler' in state_dict:
            cp = state_dict.pop('scheduler')
            self._scheduler.load_state_dict({'last_epoch': cp['last_epoch']})
            self._scheduler.step()
