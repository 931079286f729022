#!/usr/bin/env python
"""Reference-run fixture of the optimiser stage: tests/golden/optim_cases.npz.

    python tests/golden/make_solver_golden.py <root of the reference checkout>

RUNS, on the CPU, the reference's own solver code and torch's own Adamax, and stores what they return; this script contains no
reference source and derives no value itself.
  groups/*   the reference's build_optimizer (solver/OptimizerBuilder.py) on tests/optim_cases.tiny_module() with
             tests/optim_cases.solver_config(): per parameter group the name of its parameter, its lr and its weight decay
  sched/*    the reference's Solver (solver/Solver.py) with each of its two schedulers and both warm-up methods: every group's
             fp64 lr after construction and after each of 24 iterations (optimizer.step(); scheduler.step()), and the same from a
             second Solver that took the first one's state_dict() after 10 iterations through the reference's Solver.load_state_dict
  <case>/*   torch.optim.Adamax (foreach=False) over the gradients of tests/optim_cases.FIXTURE_CASES, once with fp32 and once
             with fp64 tensors: every parameter after the recorded steps.  The distance between the two is torch's own precision.

What has to stand in for missing pieces: fvcore is not installed, so fvcore.common.config is a stub module whose CfgNode is a
plain class (the reference only uses it as an annotation); the configuration is a namespace with the keys the reference reads."""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import optim_cases as oc  # noqa: E402


def import_reference(root):
    for n in ('fvcore', 'fvcore.common', 'fvcore.common.config'):
        sys.modules[n] = types.ModuleType(n)
    sys.modules['fvcore.common.config'].CfgNode = type('CfgNode', (), {})
    sys.path.insert(0, root)
    from solver.Solver import Solver
    from solver.OptimizerBuilder import build_optimizer
    return Solver, build_optimizer


def lrs(solver):
    return [float(g['lr']) for g in solver.optimizer.param_groups]


def main(root):
    Solver, build_optimizer = import_reference(root)
    out = {}
    # the groups
    model = oc.tiny_module()
    opt = build_optimizer(oc.solver_config(), model)
    names = {id(p): n for n, p in model.named_parameters()}
    out['groups/name'] = np.array([names[id(g['params'][0])] for g in opt.param_groups])
    out['groups/lr'] = np.array([g['lr'] for g in opt.param_groups], np.float64)
    out['groups/weight_decay'] = np.array([g['weight_decay'] for g in opt.param_groups], np.float64)
    assert all(len(g['params']) == 1 for g in opt.param_groups)
    # the schedules
    S = oc.SCHED
    for sched, method in oc.SCHED_RUNS:
        cfg = oc.solver_config(sched, method)
        solver = Solver(oc.tiny_module(), cfg)
        rows, resumed = [lrs(solver)], None
        for it in range(1, S['iterations'] + 1):
            solver.optimizer.step()
            solver.scheduler.step()
            rows.append(lrs(solver))
            if resumed is not None:
                resumed[0].optimizer.step()
                resumed[0].scheduler.step()
                resumed[1].append(lrs(resumed[0]))
            if it == S['resume_at']:
                state = copy.deepcopy(solver.state_dict())
                other = Solver(oc.tiny_module(), cfg)
                other.load_state_dict(state)
                resumed = (other, [lrs(other)])
        key = 'sched/%s_%s' % (sched, method)
        out[key + '/lr'] = np.array(rows, np.float64)
        out[key + '/resumed_lr'] = np.array(resumed[1], np.float64)
        out[key + '/resumed_last_epoch'] = np.array(resumed[0].scheduler.last_epoch)
        out[key + '/best_param_group_id'] = np.array(solver._best_param_group_id)
        out[key + '/solver_name'] = np.array(solver.solver_name)
        print(key, 'lr of group 0:', ' '.join('%.3g' % r[0] for r in rows))
    # torch's Adamax
    for name in oc.FIXTURE_CASES:
        c = oc.make_fixture(name)
        for tag, dt in (('p32', torch.float32), ('p64', torch.float64)):
            ps = [torch.from_numpy(p.copy()).to(dt).requires_grad_(True) for p in oc.initial(c)[0]]
            opt = torch.optim.Adamax([{'params': [p], 'lr': t['lr'], 'weight_decay': t['wd']} for p, t in zip(ps, c['tensors'])],
                                     betas=c['betas'], eps=c['eps'], foreach=False)
            for step in range(1, oc.FIXTURE_STEPS + 1):
                for p, g in zip(ps, oc.grads(c, step)):
                    p.grad = torch.from_numpy(g).to(dt)
                opt.step()
                if step in oc.FIXTURE_RECORD:
                    for i, p in enumerate(ps):
                        out['%s/%s_%d_%d' % (name, tag, step, i)] = p.detach().numpy().copy()
        for step in oc.FIXTURE_RECORD:
            d = max(float(np.abs(out['%s/p32_%d_%d' % (name, step, i)].astype(np.float64) - out['%s/p64_%d_%d' % (name, step, i)]).max())
                    for i in range(len(c['tensors'])))
            print(name, 'step', step, 'max |fp32 - fp64| %.3g' % d)
    path = os.path.join(HERE, 'optim_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
