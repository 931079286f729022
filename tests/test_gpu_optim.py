"""GPU: the optimiser step on the device (rtm3d_optim_step through rtm3d_amd.optim) against the numpy restatement
tests/optim_ref.py - BIT FOR BIT in p, m, u and e after each of 6 steps (any NaN equals any NaN: which NaN a result is, is not
part of the rule) - and against torch's own Adamax (tests/golden/optim_cases.npz) within the bar of tests/test_optim_cpu.py.
The shapes are the smallest at which the launch code can go wrong, not the network's."""
import copy

import numpy as np
import pytest
import torch

from rtm3d_amd import optim
from tests import optim_cases as oc, optim_ref as ref
from tests.util import load_golden

pytestmark = pytest.mark.gpu
PAD = 7.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


class Bag(torch.nn.Module):
    """Parameters p0, p1, ..., floating-point buffers b0, b1, ... and one integer buffer."""

    def __init__(self, params, buffers):
        super().__init__()
        for i, p in enumerate(params):
            self.register_parameter('p%d' % i, p)
        for i, b in enumerate(buffers):
            self.register_buffer('b%d' % i, b)
        self.register_buffer('count', torch.tensor([3, 1, 4], dtype=torch.int64, device=params[0].device))


class Rig:
    """A case on the device: parameters inside padded flat buffers (views that start ``shift`` elements in), an Adamax over one
    group per parameter and, where the case has one, the EMA."""

    def __init__(self, case, dev):
        self.case, self.dev = case, dev
        ps0, bs0 = oc.initial(case)
        self.flats, params = [], []
        for t, a in zip(case['tensors'], ps0):
            flat = torch.full((a.size + 8,), PAD, dtype=torch.float32, device=dev)
            v = flat[t['shift']:t['shift'] + a.size]
            v.copy_(torch.from_numpy(a))
            p = torch.nn.Parameter(v)
            assert p.data_ptr() % 16 == 4 * t['shift'] and p.data_ptr() == v.data_ptr()
            self.flats.append(flat)
            params.append(p)
        self.params = params
        self.model = Bag(params, [torch.from_numpy(b).to(dev) for b in bs0])
        self.opt = optim.Adamax([{'params': [p], 'lr': t['lr'], 'weight_decay': t['wd']} for p, t in zip(params, case['tensors'])],
                                betas=case['betas'], eps=case['eps'])
        self.ema = None
        if case['ema'] is not None:
            self.ema = optim.ModelEMA(self.model, case['ema'])
            self.opt.attach_ema(self.ema)
        self.t = 0

    def step(self, loss=None):
        self.t += 1
        self.opt.zero_grad()
        for p, g in zip(self.params, oc.grads(self.case, self.t)):
            assert p.grad.data_ptr() >= self.opt.grad_arena.data_ptr()
            p.grad.copy_(torch.from_numpy(g))
        for i, b in enumerate(oc.buffers_at(self.case, self.t)):
            getattr(self.model, 'b%d' % i).copy_(torch.from_numpy(b))
        self.opt.step(None if loss is None else torch.tensor(loss, dtype=torch.float32, device=self.dev))

    def read(self):
        """{'p', 'm', 'u', 'e', 'eb'} as the restatement returns them."""
        torch.cuda.synchronize()
        n = lambda ts: [t.detach().cpu().numpy().copy() for t in ts]
        out = {'p': n(self.params), 'm': n(self.opt._m_views), 'u': n(self.opt._u_views), 'e': None, 'eb': None}
        if self.ema is not None:
            sd = self.ema.state_dict()
            assert list(sd.keys()) == list(self.model.state_dict().keys())
            assert torch.equal(sd['count'], self.model.count)                          # integer buffers are left alone
            out['e'] = n([sd['p%d' % i] for i in range(len(self.params))])
            out['eb'] = n([sd['b%d' % i] for i in range(len(self.case['buffers']))])
        return out

    def padding_untouched(self):
        return all(bool((f[:t['shift']] == PAD).all()) and bool((f[t['shift'] + t['n']:] == PAD).all())
                   for f, t in zip(self.flats, self.case['tensors']))


def assert_same(got, want, what):
    for k in ('p', 'm', 'u', 'e', 'eb'):
        if want[k] is None:
            assert got[k] is None
            continue
        assert len(got[k]) == len(want[k])
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert ref.same_bits(a, b), (what, k, i, ref.first_difference(a, b))


@pytest.mark.parametrize('name', oc.GPU_CASES)
def test_device_equals_the_restatement_bit_for_bit(dev, name):
    """After each of 6 steps: the sizes around the vector width, wave, workgroup and chunk with three hyper classes (wd = 0 and
    wd != 0), EMA on and off; 300 tiny tensors (more chunks than workgroups); views 1, 2, 3 elements into a buffer (the scalar
    path) next to aligned ones; beta1 = 0.3; lr = 0; all-zero gradients; a denormal gradient and parameter; a NaN and an Inf
    gradient element; EMA-only buffer segments."""
    case = oc.make(name)
    want = oc.restated(name)
    rig = Rig(case, dev)
    for t in range(oc.STEPS):
        rig.step()
        assert_same(rig.read(), want[t], (name, 'step', t + 1))
    assert rig.padding_untouched() and rig.opt.skipped() == 0
    if name == 'many':
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        assert rig.opt._tables[2] >= 300 > cus, 'the chunk table is no longer than the grid (%d chunks, %d compute units)' % (rig.opt._tables[2], cus)
    if name == 'nonfinite':
        got = rig.read()
        assert np.isnan(got['p'][0][4]) and np.isfinite(np.delete(got['p'][0], 4)).all()
        assert np.isnan(got['p'][1][129]) and np.isfinite(np.delete(got['p'][1], 129)).all()
    if name == 'views':
        assert {p.data_ptr() % 16 for p in rig.params} == {0, 4, 8, 12}


def test_guard_skips_and_counts(dev):
    """A NaN, +Inf or -Inf loss: every byte of p, m, u, e as before, the counter up by one; the next finite step equals the
    restatement with t (and the EMA's count) advanced over the skipped steps; no loss address: the update always applies."""
    case = oc.make('sizes')
    losses = [0.5, float('nan'), 1.5, float('inf'), float('-inf'), None]
    want = oc.restate(case, len(losses), losses=losses)
    rig = Rig(case, dev)
    skipped, before = 0, None
    for t, loss in enumerate(losses):
        rig.step(loss)
        got = rig.read()
        assert_same(got, want[t], ('guard', 'step', t + 1))
        if loss is not None and not np.isfinite(loss):
            skipped += 1
            for k in 'pmue':
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got[k], before[k])), (t, k)
        assert rig.opt.skipped() == skipped
        before = got
    assert skipped == 3 and rig.opt._t == 6 and rig.ema.updates == 6
    plain = oc.restated('sizes')
    assert not ref.same_bits(want[5]['p'][9], plain[5]['p'][9])                        # (the skips did change the trajectory)


def test_two_runs_leave_equal_bytes(dev):
    for name in ('sizes', 'views'):
        runs = []
        for _ in range(2):
            rig = Rig(oc.make(name), dev)
            for _ in range(3):
                rig.step(1.0)
            runs.append(rig.read())
        for k in 'pmue':
            assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][k], runs[1][k])), (name, k)


@pytest.mark.parametrize('name', oc.FIXTURE_CASES)
def test_device_follows_torch_adamax(dev, name):
    """30 steps against torch's own fp64 trajectory, per tensor and recorded step within max(4 x torch's own fp32-vs-fp64
    distance, 4 fp32 ulp of the tensor's largest magnitude).  The device equals the restatement bit for bit, so the figures are
    those of tests/test_optim_cpu.py: 1.00 x torch's own distance on 29 of 30 triples, 1.39 x on one."""
    g = load_golden('optim_cases.npz')
    case = oc.make_fixture(name)
    want = oc.restate(case, oc.FIXTURE_STEPS)
    rig = Rig(case, dev)
    for step in range(1, oc.FIXTURE_STEPS + 1):
        rig.step()
        if step in oc.FIXTURE_RECORD:
            got = rig.read()['p']
            for i, a in enumerate(got):
                t64, d, bar = oc.trajectory_bar(g, name, i, step)
                err = float(np.abs(a.astype(np.float64) - t64).max())
                print('%s step %d tensor %d: device vs torch fp64 %.3g, torch fp32 vs fp64 %.3g, bar %.3g' % (name, step, i, err, d, bar))
                assert err <= bar, (name, step, i, err, bar)
                assert ref.same_bits(a, want[step - 1]['p'][i])


def test_refusals(dev):
    p = torch.nn.Parameter(torch.zeros(8, device=dev))
    with pytest.raises(ValueError, match='contiguous fp32 device tensor'):
        optim.Adamax([torch.nn.Parameter(torch.zeros(8))])
    with pytest.raises(ValueError, match='contiguous fp32 device tensor'):
        optim.Adamax([torch.nn.Parameter(torch.zeros(8, device=dev, dtype=torch.float64))])
    with pytest.raises(ValueError, match='contiguous fp32 device tensor'):
        optim.Adamax([torch.nn.Parameter(torch.zeros(8, 2, device=dev).t())])
    with pytest.raises(ValueError, match='more than one group'):
        optim.Adamax([{'params': [p]}, {'params': [p]}])
    with pytest.raises(ValueError, match='no parameters'):
        optim.Adamax([])
    ps = [torch.nn.Parameter(torch.zeros(4, device=dev)) for _ in range(17)]
    opt = optim.Adamax([{'params': [q], 'lr': 0.001 * (i + 1)} for i, q in enumerate(ps)])
    with pytest.raises(ValueError, match='17 distinct .* 16 hyper classes'):
        opt.step()
    opt = optim.Adamax([p])
    with pytest.raises(ValueError, match='cleared, not dropped'):
        opt.zero_grad(set_to_none=True)
    with pytest.raises(ValueError, match='one scalar on the device'):
        opt.step(torch.zeros(2, device=dev))
    with pytest.raises(ValueError, match='one scalar on the device'):
        opt.step(torch.zeros(()))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the facade
class Net(torch.nn.Module):
    """Three layers with the names the builder's rule looks at; plain torch on the device."""

    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(6, 8)
        self.norm = torch.nn.BatchNorm1d(8)
        self.fc2 = torch.nn.Linear(8, 3)

    def forward(self, x):
        return self.fc2(torch.relu(self.norm(self.fc1(x))))


def net(dev, seed=0):
    torch.manual_seed(seed)
    return Net().to(dev).train()


def batch(dev, step):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(16, 6, generator=g).to(dev), torch.randn(16, 3, generator=g).to(dev)


def loss_of(model, dev, step):
    x, y = batch(dev, step)
    with torch.backends.cudnn.flags(enabled=False):                                    # ATen's own batch norm
        return ((model(x) - y) ** 2).mean()


def flat_cfg(**kw):
    """A schedule that is flat from the start (no warm-up, a far milestone)."""
    return {'SOLVER': dict({'WARMUP_ITERS': 0, 'STEPS': (1000,), 'BASE_LR': 0.01, 'BIAS_LR_FACTOR': 2.0}, **kw)}


def bytes_of(model):
    torch.cuda.synchronize()
    return [v.detach().cpu().numpy().tobytes() for v in model.state_dict().values()]


def test_solver_step_on_a_torch_module(dev):
    model = net(dev)
    solver = optim.Solver(model, flat_cfg(), ema=0.999)
    opt = solver.optimizer
    assert solver.solver_name == 'Adamax_WarmupMultiStepLR' and solver.learn_rate == 0.01
    assert [g['name'] for g in opt.param_groups] == [n for n, _ in model.named_parameters()]
    before = copy.deepcopy(model.state_dict())
    solver.step(loss_of(model, dev, 0))                                               # (the first step plans: one upload)
    loss = loss_of(model, dev, 1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                                            # step never waits for the device
    try:
        out = solver.step(loss)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert out.shape == () and torch.equal(out, loss)
    lo, hi = opt.grad_arena.data_ptr(), opt.grad_arena.data_ptr() + 4 * opt.grad_arena.numel()
    for (n, p), v in zip(model.named_parameters(), opt._grad_views):
        assert p.grad is not None and lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi, n
        assert p.grad.data_ptr() == v.data_ptr() and p.grad.shape == p.shape and bool(p.grad.ne(0).any())
        assert not torch.equal(p.detach(), before[n])
    assert solver.skipped() == 0 and solver.scheduler.last_epoch == 2 and solver.ema.updates == 2
    # the EMA: keyed like the model, the floating-point entries views of its arena, copy_to fills another model
    esd = solver.ema.state_dict()
    assert list(esd.keys()) == list(model.state_dict().keys())
    a0, a1 = solver.ema.arena.data_ptr(), solver.ema.arena.data_ptr() + 4 * solver.ema.arena.numel()
    for k, v in esd.items():
        if v.dtype.is_floating_point:
            assert a0 <= v.data_ptr() < a1 and v.shape == model.state_dict()[k].shape, k
    assert int(esd['norm.num_batches_tracked']) == 0 and int(model.norm.num_batches_tracked) == 2
    assert not torch.equal(esd['norm.running_mean'], before['norm.running_mean'])      # an EMA-only segment moved
    other = solver.ema.copy_to(net(dev, seed=5))
    for k, v in other.state_dict().items():
        assert torch.equal(v, esd[k]), k
    # a dict of losses, as the reference's step takes
    solver.step({'a': loss_of(model, dev, 2), 'b': loss_of(model, dev, 3)})
    with pytest.raises(TypeError, match='a loss tensor or a dict'):
        solver.step(3.0)
    # a non-finite loss through the facade: nothing moves, the schedule goes on
    snap = bytes_of(model)
    solver.step(loss_of(model, dev, 4) * float('nan'))
    assert solver.skipped() == 1 and solver.scheduler.last_epoch == 4
    now = bytes_of(model)
    keys = list(model.state_dict().keys())
    for k, a, b in zip(keys, snap, now):
        if 'running' not in k and 'tracked' not in k:                                  # (the forward pass moved the statistics)
            assert a == b, k


def twin(dev, cfg=None, ema=None):
    model = net(dev)
    return model, optim.Solver(model, cfg or flat_cfg(), ema=ema)


def test_foreign_and_missing_gradients(dev):
    """A foreign .grad is copied into its view and re-pointed; a None .grad counts as a zero gradient (torch skips such a
    parameter: a documented deviation) - its moments decay and weight decay applies."""
    (ma, sa), (mb, sb) = twin(dev), twin(dev)
    sa.step(loss_of(ma, dev, 0))
    sb.step(loss_of(mb, dev, 0))
    assert bytes_of(ma) == bytes_of(mb)
    gs = [torch.randn(p.shape, generator=torch.Generator().manual_seed(i)).to(dev) for i, p in enumerate(ma.parameters())]
    # a: the gradients written into the views; b: foreign tensors, and None where a holds zeros
    sa.optimizer.zero_grad()
    for i, (p, g) in enumerate(zip(ma.parameters(), gs)):
        if i != 2:
            p.grad.copy_(g)
    for i, (p, g) in enumerate(zip(mb.parameters(), gs)):
        p.grad = None if i == 2 else g.clone()
        assert i == 2 or p.grad.data_ptr() != sb.optimizer._grad_views[i].data_ptr()
    w2 = list(mb.parameters())[2].detach().clone()
    sa.optimizer.step()
    sb.optimizer.step()
    assert bytes_of(ma) == bytes_of(mb)
    for p, v in zip(mb.parameters(), sb.optimizer._grad_views):
        assert p.grad is v                                                             # re-pointed, the None one too
    assert not torch.equal(list(mb.parameters())[2].detach(), w2)                      # the zero gradient still moved it (m != 0)
    for a, b in zip(sa.optimizer._m_views + sa.optimizer._u_views, sb.optimizer._m_views + sb.optimizer._u_views):
        assert torch.equal(a, b)


def test_state_dict_round_trips_through_torch_adamax(dev):
    model, solver = twin(dev)
    for step in range(3):
        solver.step(loss_of(model, dev, step))
    opt = solver.optimizer
    sd = copy.deepcopy(opt.state_dict())
    assert sorted(sd.keys()) == ['param_groups', 'state'] and sorted(sd['state'].keys()) == list(range(6))
    assert all(sorted(s.keys()) == ['exp_avg', 'exp_inf', 'step'] and float(s['step']) == 3.0 for s in sd['state'].values())
    assert [g['params'] for g in sd['param_groups']] == [[i] for i in range(6)]
    # into a real torch.optim.Adamax over a copy of the model, one step there and one here on the same gradients
    clone = copy.deepcopy(model)
    topt = torch.optim.Adamax([{'params': [p], 'lr': g['lr'], 'weight_decay': g['weight_decay']}
                               for p, g in zip(clone.parameters(), opt.param_groups)], foreach=False)
    topt.load_state_dict(copy.deepcopy(sd))
    for p, mv, uv in zip(clone.parameters(), opt._m_views, opt._u_views):
        assert torch.equal(topt.state[p]['exp_avg'], mv) and torch.equal(topt.state[p]['exp_inf'], uv) and float(topt.state[p]['step']) == 3.0
    loss_of(clone, dev, 3).backward()
    topt.step()
    solver.step(loss_of(model, dev, 3))
    for (n, a), b in zip(model.named_parameters(), clone.parameters()):
        err = float((a.detach() - b.detach()).abs().max())
        assert err <= 4 * float(np.spacing(np.float32(a.detach().abs().max().item()))), (n, err)      # torch's kernels contract; 4 ulp
    # and torch's state back into a fresh optimiser here
    back = copy.deepcopy(topt.state_dict())
    model2, solver2 = twin(dev)
    solver2.optimizer.load_state_dict(back)
    assert solver2.optimizer._t == 4
    for p, mv, uv in zip(clone.parameters(), solver2.optimizer._m_views, solver2.optimizer._u_views):
        assert torch.equal(topt.state[p]['exp_avg'], mv) and torch.equal(topt.state[p]['exp_inf'], uv)
    # parameters at different steps cannot be represented here
    back['state'][0]['step'] = torch.tensor(9.0)
    with pytest.raises(ValueError, match='different steps'):
        solver2.optimizer.load_state_dict(back)
    back = copy.deepcopy(topt.state_dict())
    back['param_groups'][1]['betas'] = (0.5, 0.999)
    with pytest.raises(ValueError, match='betas'):
        solver2.optimizer.load_state_dict(back)


def test_save_load_and_three_more_steps_equal_six(dev):
    """On a flat schedule (the reference's load takes one extra scheduler step, which a warm-up would show)."""
    ma, sa = twin(dev)
    for step in range(6):
        sa.step(loss_of(ma, dev, step))
    mb, sb = twin(dev)
    for step in range(3):
        sb.step(loss_of(mb, dev, step))
    saved = copy.deepcopy({'model': mb.state_dict(), 'solver': sb.state_dict()})
    assert sorted(saved['solver'].keys()) == ['best_param_group_id', 'optimizer', 'scheduler']
    mc = net(dev, seed=9)
    mc.load_state_dict(saved['model'])
    sc = optim.Solver(mc, flat_cfg())
    sc.load_state_dict(saved['solver'])
    assert saved['solver'] == {} and sc.scheduler.last_epoch == 4 and sc.optimizer._t == 3
    for step in range(3, 6):
        sc.step(loss_of(mc, dev, step))
    assert bytes_of(ma) == bytes_of(mc)
    for a, b in zip(sa.optimizer._m_views + sa.optimizer._u_views, sc.optimizer._m_views + sc.optimizer._u_views):
        assert torch.equal(a, b)


@pytest.mark.parametrize('sched,method', oc.SCHED_RUNS)
def test_solver_schedule_and_resume_equal_the_reference_run(dev, sched, method):
    """The facade on the fixture's module: every group's lr over 24 steps, learn_rate, the names, and a second Solver resumed
    through load_state_dict after 10, all == the reference's own Solver."""
    g = load_golden('optim_cases.npz')
    key = 'sched/%s_%s' % (sched, method)
    cfg = oc.solver_config(sched, method)
    quad = lambda m: sum((p ** 2).sum() for p in m.parameters() if p.requires_grad)
    lrs = lambda s: [q['lr'] for q in s.optimizer.param_groups]
    model = oc.tiny_module().to(dev)
    solver = optim.Solver(model, cfg)
    assert solver.solver_name == str(g[key + '/solver_name']) and solver._best_param_group_id == int(g[key + '/best_param_group_id'])
    rows, resumed = [lrs(solver)], None
    for it in range(1, oc.SCHED['iterations'] + 1):
        solver.step(quad(model))
        rows.append(lrs(solver))
        assert solver.learn_rate == rows[-1][solver._best_param_group_id]
        if resumed is not None:
            resumed[0].step(quad(resumed[2]))
            resumed[1].append(lrs(resumed[0]))
        if it == oc.SCHED['resume_at']:
            state = copy.deepcopy(solver.state_dict())
            m2 = oc.tiny_module().to(dev)
            other = optim.Solver(m2, cfg)
            other.load_state_dict(state)
            resumed = (other, [lrs(other)], m2)
    assert (np.array(rows, np.float64) == g[key + '/lr']).all()
    assert (np.array(resumed[1], np.float64) == g[key + '/resumed_lr']).all()
    assert resumed[0].scheduler.last_epoch == int(g[key + '/resumed_last_epoch'])
    assert solver.skipped() == 0
