"""Backward pass of the neck's softmax fusion and its transposed convs on the device (include/rtm3d_hip.h, "neck fusion backward";
csrc/neck_backward.hip).

``TrainableFusion(heads)`` takes the hand-off of ``TrainableHeads(model, input_grad=True)`` - dz, the gradient of the fused map -
one stage up: through

    z = z0 + sum_i u_i * softmax_{H W}(u_i.detach()),     u_i = fusion_up{i}(kfpn_h{i}),    i = 3, 4, 5

(models/nets/keypoint_fpn_fusion.py, forward) to the six ``kfpn_fusion.fusion_up{L}.{j}.conv_tran.weight`` tensors, which become
trainable next to the heads, and to the gradients at z0, kfpn_h3, kfpn_h4 and kfpn_h5::

    heads = TrainableHeads(model, input_grad=True)
    fusion = TrainableFusion(heads)                     # the heads' parameters plus the six transposed-conv weights
    solver = optim.Solver(fusion, cfg)
    loss, items = RTM3DLoss(cfg)(fusion(x), targets)
    solver.step(loss)

``FusionBackward`` is the chain itself on raw maps: softmax statistics and du -> per transposed conv, last to first, wgrad and
dgrad.  The forward's saved activations (kfpn_h*, the intermediate up maps, u*) are the plan's own tensors.

``fusion_scale`` (a power of two, T): the softmax weights are about 1 / (H W), so du and every dX behind it are stored times
S T (S: the heads' grad_scale); the weight gradients leave unscaled.  The default is measured, not guessed
(tools/gpu_fusion_grad_scale.py, profiles/neck_backward.txt, section 1):
%s
Labels or weights with larger gradients want a smaller T: an overflow shows as Inf / NaN weight gradients, which ``nonfinite()``
counts.

The FPN half of the neck (kfpn_up*, the composed proj + head 1x1 convs) is rtm3d_amd/fpn_train.py: ``TrainableNeck`` composes a
TrainableFusion, runs the plan's training lowering and adds the kfpn_up path to ``input_grads()['kfpn_h*']``, which here are the
FUSION-PATH terms only.
LEFT UNDONE: the backbone backward; graph-replayed plans; head_precision='mxfp8'; training BatchNorm.
"""
import ctypes

import numpy as np

from . import _lib
from . import head_train as ht

SCALE_TABLE = """\
    on the loss-gradient fixture's labels (fx_b1, fx_b2_empty; 24 x 40 map) with synth_state_dict weights, through the model, the
    fp64 reference's largest gradient activations behind dz (max |dz| = 0.052) are, unscaled,
        max |du3| = 2.2e-4, |du4| = 3.2e-4, |du5| = 4.3e-4 (medians of the non-zero elements: 1e-7 .. 6e-7),
        max |dX| of fusion_up3.0 = 2.3e-4, up4.1 = 3.0e-4, up4.0 = 8.6e-4, up5.2 = 1.0e-4, up5.1 = 1.4e-4, up5.0 = 2.4e-4;
    with S = 2 ** 14 the share of the non-zero reference elements below fp16's smallest normal is
        T = 1: 3.0 %   T = 4: 0.84 %   T = 16: 0.28 %   T = 64: 0.13 %   T = 256: 0.08 %   T = 1024: 0.07 %
    and 2 ** 8 is the largest power of two T that keeps S T x 8.6e-4 = 3594 sixteen times below fp16's 65504.
"""
__doc__ = __doc__ % SCALE_TABLE

DEFAULT_FUSION_SCALE = 256.0
DEFAULT_SLICE_WORKGROUPS = 1024           # wgrad workgroups a launch aims at: 4 output tiles x 16 taps x slices
FUSION_LEVELS = (3, 4, 5)                 # the reference's level numbers of operands 1, 2, 3


def check(B, H, W, levels, grad_scale, fusion_scale):
    """The host check of a fusion-backward geometry (rtm3d_neck_backward_check; runs without a GPU).  Raises RuntimeError."""
    _lib.check(_lib.load().rtm3d_neck_backward_check(int(B), int(H), int(W), int(levels), float(grad_scale), float(fusion_scale)),
               'neck_backward_check')


def default_slices():
    return max(1, min(64, DEFAULT_SLICE_WORKGROUPS // 64))


def rotate_deconv_weights(w16):
    """fp16 ConvTranspose2d weight (ci, co, 4, 4) -> the dgrad operand [tap = 4 ky + kx][ci][co] (same device).  No flip and no
    cin / cout swap: the weight is (ci, co) already."""
    ci, co = w16.shape[:2]
    return w16.permute(2, 3, 0, 1).reshape(16, ci, co).contiguous()


def weight_names(levels=3):
    """The reference's state-dict keys of the chains, operand after operand: [[name of deconv j of operand l]]."""
    return [['kfpn_fusion.fusion_up%d.%d.conv_tran.weight' % (FUSION_LEVELS[l], j) for j in range(l + 1)] for l in range(levels)]


class FusionBackward(object):
    """The fusion-backward chain for one geometry, on raw maps.  B, H, W: batch and MAP size (of z); operand l = 0 .. levels - 1 is
    a chain of l + 1 transposed convs whose first input is (H >> (l + 1)) x (W >> (l + 1)).  Owns the gradient maps (cleared
    once: the launches write interiors only), the workspace and the non-finite counter.  ``run`` issues the launches on the
    current stream and never synchronises.

    du[l]: (B, H + 2, W + 2, 256), the gradient at u_l times S T.  dx[l][j]: the gradient at the input of deconv j of operand l,
    border 1; dx[l][0] is the fusion-path term of d kfpn_h."""

    def __init__(self, B, H, W, device, levels=3, grad_scale=ht.DEFAULT_GRAD_SCALE, fusion_scale=None, want_slices=None):
        import torch
        fusion_scale = DEFAULT_FUSION_SCALE if fusion_scale is None else fusion_scale
        for what, v in (('grad_scale', grad_scale), ('fusion_scale', fusion_scale)):
            if not ht._is_pow2(v):
                raise ValueError('fusion backward: %s = %r is no power of two' % (what, v))
        check(B, H, W, levels, grad_scale, fusion_scale)
        self.B, self.H, self.W, self.levels = int(B), int(H), int(W), int(levels)
        self.S, self.T, self.device = float(grad_scale), float(fusion_scale), torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.want = int(want_slices) if want_slices is not None else default_slices()
        self.n_slices = max(ht.slices(self.B * (self.H >> s) * (self.W >> s), self.want)[0] for s in range(1, self.levels + 1))
        z16 = lambda h, w: torch.zeros(self.B, h + 2, w + 2, 256, dtype=torch.float16, device=self.device)
        self.du = [z16(self.H, self.W) for _ in range(self.levels)]
        self.dx = [[z16(*self.in_hw(l, j)) for j in range(l + 1)] for l in range(self.levels)]
        nbytes = int(_lib.load().rtm3d_neck_backward_workspace_bytes(self.B, self.levels, self.n_slices))
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=self.device)

    def in_hw(self, l, j):
        """Input size of deconv j of operand l."""
        s = l + 1 - j
        return self.H >> s, self.W >> s

    def du_map(self, l):
        return ht.hb_map(self.du[l].data_ptr(), 256, 1)

    def dx_map(self, l, j):
        return ht.hb_map(self.dx[l][j].data_ptr(), 256, 1)

    def run(self, dz, us, xs, wr, dw):
        """dz: rtm3d_hb_map of the H x W gradient of z (times S).  us[l]: map of u_l.  xs[l][j]: map of the input of deconv j of
        operand l (xs[l][0]: kfpn_h).  wr[l][j]: the rotated fp16 weight (rotate_deconv_weights).  dw[l][j]: fp32 (256, 256, 4, 4)
        device tensor or None (skipped)."""
        import torch
        lib = _lib.load()
        B, H, W, n = self.B, self.H, self.W, self.levels
        for l in range(n):
            for j in range(l + 1):
                t = dw[l][j]
                if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (256, 256, 4, 4) or t.dtype != torch.float32
                                      or not t.is_contiguous() or t.device != self.device):
                    raise ValueError('fusion backward: dw[%d][%d] must be a contiguous fp32 (256, 256, 4, 4) tensor on %s' % (l, j, self.device))
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            ws, nws = self.ws.data_ptr(), self.ws.numel() * 4
            arr = lambda maps: (_lib.HbMapC * n)(*maps)
            _lib.check(lib.rtm3d_neck_softmax_grad(st, B, H, W, n, ctypes.byref(dz), arr(list(us)), arr([self.du_map(l) for l in range(n)]),
                                                   self.T, ws, nws), 'neck_softmax_grad')
            for l in range(n):
                for j in range(l, -1, -1):
                    hi, wi = self.in_hw(l, j)
                    dy = self.du_map(l) if j == l else self.dx_map(l, j + 1)
                    _lib.check(lib.rtm3d_neck_deconv_wgrad(st, B, hi, wi, ctypes.byref(xs[l][j]), ctypes.byref(dy), self.S, self.T,
                                                           dw[l][j].data_ptr() if dw[l][j] is not None else None, self.want, ws, nws,
                                                           self.nonfinite.data_ptr()), 'neck_deconv_wgrad')
                    dx = self.dx_map(l, j)
                    _lib.check(lib.rtm3d_neck_deconv_dgrad(st, B, hi, wi, ctypes.byref(dy), wr[l][j].data_ptr(), ctypes.byref(dx)),
                               'neck_deconv_dgrad')


# --------------------------------------------------------------------------------------------------- through the model
def _deconv_group_src(idx):
    """Arena indices (ci, co, 4, 4) -> per sub-pixel phase the (taps, cout, cin) array plan.Plan.deconv hands the packer."""
    kd = {0: [(1, 0), (3, -1)], 1: [(0, 1), (2, 0)]}
    return [np.stack([idx[:, :, ky, kx].T for ky, _ in kd[py] for kx, _ in kd[px]], 0) for py in (0, 1) for px in (0, 1)]


class TrainableFusion(object):
    """The fusion half of the neck of ``heads.model`` as trainable fp32 CUDA leaves next to the heads' parameters; see the module
    docstring.  ``heads``: a TrainableHeads built with ``input_grad=True`` (refused otherwise).  ``named_parameters`` /
    ``parameters`` / ``state_dict(keep_vars=)`` cover the heads' parameters plus the six transposed-conv weights, so
    ``optim.Solver(fusion, cfg)`` and ``ModelEMA`` work unchanged.

    ``fusion(x)`` / ``fusion(None, preloaded=(B, H, W))`` refreshes both sets of packed weights, runs the model's dense fp16 plan
    and returns the logit maps under ONE autograd node whose backward runs the heads' chain, then the fusion chain.  The heads'
    refusals hold (mxfp8, graph-replayed plans, stale plans); refused by name as well: a plan that does not keep kfpn_h*, an
    intermediate up map or u* as a plain written tensor, or whose tensors overlap in memory."""

    def __init__(self, heads, fusion_scale=None, want_slices=None):
        import torch
        if not isinstance(heads, ht.TrainableHeads):
            raise TypeError('TrainableFusion: heads must be a TrainableHeads')
        if not heads._want_dz:
            raise ValueError('TrainableFusion: the heads were built without input_grad=True, so they produce no dz')
        fusion_scale = DEFAULT_FUSION_SCALE if fusion_scale is None else fusion_scale
        if not ht._is_pow2(fusion_scale):
            raise ValueError('TrainableFusion: fusion_scale = %r is no power of two' % (fusion_scale,))
        self.heads, self.model, self.device = heads, heads.model, heads.device
        self.S, self.T, self.want_slices = heads.S, float(fusion_scale), want_slices
        self.levels = len(FUSION_LEVELS)
        self._wnames = weight_names(self.levels)
        sd = self.model.state_dict()
        flat = [n for names in self._wnames for n in names]
        for n in flat:
            if n not in sd or tuple(sd[n].shape) != (256, 256, 4, 4):
                raise NotImplementedError('TrainableFusion: %s is missing or is no (256, 256, 4, 4) transposed-conv weight' % n)
        per = 256 * 256 * 16
        self._off = {n: i * per for i, n in enumerate(flat)}
        self._arena = torch.zeros(len(flat) * per, dtype=torch.float32, device=self.device)
        self._params = {}
        for n in flat:
            v = self._arena[self._off[n]:self._off[n] + per].view(256, 256, 4, 4)
            v.copy_(sd[n])
            self._params[n] = v.requires_grad_()
        self._bn = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64, device=self.device)          # row 0: no BatchNorm
        self._scale_of = torch.zeros(len(flat) * per, dtype=torch.int32, device=self.device)
        self._wr = [[torch.zeros(16, 256, 256, dtype=torch.float16, device=self.device) for _ in names] for names in self._wnames]
        self._rot_perm = [[torch.from_numpy(self._wsrc(n).transpose(2, 3, 0, 1).reshape(-1).astype(np.int32)).to(self.device) for n in names]
                          for names in self._wnames]
        self._plans = {}
        self._last = None

    def _wsrc(self, name):
        return self._off[name] + np.arange(256 * 256 * 16, dtype=np.int64).reshape(256, 256, 4, 4)

    # ---- nn.Module-like surface
    def named_parameters(self):
        return iter(list(self.heads.named_parameters()) + list(self._params.items()))

    def parameters(self):
        return iter([p for _, p in self.named_parameters()])

    def state_dict(self, keep_vars=False):
        out = self.heads.state_dict(keep_vars=keep_vars)
        for k, v in self._params.items():
            out[k] = v if keep_vars else v.detach()
        return out

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def export_to(self, model=None):
        """Write the heads' and the fusion's parameters back through ``model.load_state_dict``."""
        model = self.model if model is None else model
        sd = model.state_dict()
        for k, v in self.named_parameters():
            sd[k] = v.detach().cpu()
        model.load_state_dict(sd)
        if model is self.model:
            self._plans, self.heads._plans = {}, {}
        return model

    def nonfinite(self):
        """Non-finite parameter-gradient elements produced so far, the heads' included (one synchronisation per plan)."""
        return self.heads.nonfinite() + sum(int(st['fb'].nonfinite.item()) for st in self._plans.values())

    # ---- per-plan state
    def _map_of(self, rplan, s, what, hw, border):
        low = rplan.lowering
        key = (s.tid, s.coff, s.C)
        if key in low['s2d_only'] or key in low['unwritten']:
            raise NotImplementedError('TrainableFusion: the plan does not keep %s as a plain written tensor' % what)
        addr, b, h, w, C, P = rplan.tensor_info(s)
        if (b, h, w) != (rplan.plan.B,) + tuple(hw) or s.C != 256 or s.coff + 256 > C or P < border:
            raise RuntimeError('TrainableFusion: %s is %s with border %d, not the fusion geometry' % (what, (b, h, w, C), P))
        return ht.hb_map(addr, C, P, s.coff), (addr, addr + 2 * b * (h + 2 * P) * (w + 2 * P) * C, what)

    def _state(self, rplan, hst):
        import torch
        st = self._plans.get(id(rplan))
        if st is not None and st['plan'] is rplan and st['hst'] is hst:
            return st
        if rplan.graph_stats()[2]:
            raise NotImplementedError('TrainableFusion: the plan replays a captured graph; set model.use_graph = False')
        B, H, W = hst['shape']
        Hm, Wm = H // 4, W // 4
        check(B, Hm, Wm, self.levels, self.S, self.T)
        ops = {op.get('name'): op for op in rplan.plan.ops}
        named = rplan.plan.named
        us, xs, spans = [], [], []
        for l, L in enumerate(FUSION_LEVELS):
            chain = []
            for j in range(l + 1):
                op = ops.get('fusion_up%d.%d' % (L, j))
                if op is None or op.get('groups') != 4 or tuple(op['w'].shape) != (4, 4, 256, 256):
                    raise NotImplementedError('TrainableFusion: the plan has no four-phase 256 -> 256 launch fusion_up%d.%d' % (L, j))
                hw = (Hm >> (l + 1 - j), Wm >> (l + 1 - j))
                m, span = self._map_of(rplan, op['inp'][0], 'the input of fusion_up%d.%d' % (L, j), hw, 0)
                chain.append(m); spans.append(span)
                if j == 0 and (op['inp'][0].tid, op['inp'][0].coff) != (named['kfpn_h%d' % L].tid, named['kfpn_h%d' % L].coff):
                    raise RuntimeError('TrainableFusion: fusion_up%d.0 does not read kfpn_h%d' % (L, L))
                if j == l:
                    if (op['out'][0].tid, op['out'][0].coff) != (named['u%d' % L].tid, named['u%d' % L].coff):
                        raise RuntimeError('TrainableFusion: fusion_up%d.%d does not write u%d' % (L, j, L))
                    m, span = self._map_of(rplan, op['out'][0], 'u%d' % L, (Hm, Wm), 0)
                    us.append(m); spans.append(span)
            xs.append(chain)
        # the runtime gives every tensor an allocation of its own; a runtime that packed them into one arena by lifetime could hand a
        # saved activation's memory to a later tensor, so the address ranges are checked, not assumed
        for nm in ('z', 'h1', 'h2'):
            if nm in named:
                addr, b, h, w, C, P = rplan.tensor_info(named[nm])
                spans.append((addr, addr + 2 * b * (h + 2 * P) * (w + 2 * P) * C, nm))
        spans.sort()
        for (a0, a1, na), (b0, b1, nb) in zip(spans, spans[1:]):
            if b0 < a1:
                raise NotImplementedError('TrainableFusion: %s and %s overlap in device memory: a saved activation may be overwritten' % (na, nb))
        table, keep, found = [], [], set()
        flat = {('fusion_up%d.%d' % (L, j)): self._wnames[l][j] for l, L in enumerate(FUSION_LEVELS) for j in range(l + 1)}
        for rec in rplan.param_blobs:
            name = flat.get(rec['name'])
            if name is None:
                continue
            perm = np.concatenate([ht.perm_through(rec['pack'], src) for src in _deconv_group_src(self._wsrc(name))])
            if perm.size * 2 != rplan.blob_bytes(rec['w_blob']) or perm.max() >= self._arena.numel():
                raise RuntimeError('TrainableFusion: the gather table of %s does not match its blob' % rec['name'])
            d = torch.from_numpy(perm).to(self.device)
            keep.append(d)
            found.add(rec['name'])
            table.append((rplan.blob_address(rec['w_blob']), d.data_ptr(), perm.size, 0, 0))
        if len(found) != len(flat):
            raise RuntimeError('TrainableFusion: found %d of %d packed fusion_up arrays in the plan' % (len(found), len(flat)))
        for l in range(self.levels):
            for j in range(l + 1):
                table.append((self._wr[l][j].data_ptr(), self._rot_perm[l][j].data_ptr(), self._wr[l][j].numel(), 0, 0))
        c_jobs = (_lib.HbRefreshJobC * len(table))(*[_lib.HbRefreshJobC(*j) for j in table])
        _lib.check(_lib.load().rtm3d_head_refresh_check(len(table), c_jobs), 'head_refresh_check')
        d_jobs = torch.frombuffer(bytearray(ctypes.string_at(c_jobs, ctypes.sizeof(c_jobs))), dtype=torch.uint8).to(self.device)
        fb = FusionBackward(B, Hm, Wm, self.device, self.levels, self.S, self.T, self.want_slices)
        st = {'plan': rplan, 'hst': hst, 'us': us, 'xs': xs, 'jobs': c_jobs, 'd_jobs': d_jobs, 'keep': keep, 'fb': fb}
        self._plans = {k: v for k, v in self._plans.items() if v['plan'].ctx}
        self._plans[id(rplan)] = st
        return st

    def refresh(self, st=None):
        """Rebuild on the device, in one launch per plan, the packed forward weights of the six fusion_up launches and the rotated
        dgrad copies (rtm3d_head_refresh: kind 0, no BatchNorm)."""
        import torch
        for s in ([st] if st is not None else list(self._plans.values())):
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().rtm3d_head_refresh(_lib.stream_ptr(self.device), len(s['jobs']), s['jobs'], s['d_jobs'].data_ptr(),
                                                          self._arena.data_ptr(), self._scale_of.data_ptr(), self._bn.data_ptr()), 'head_refresh')

    # ---- forward / backward
    def __call__(self, x, preloaded=None):
        heads, m = self.heads, self.model
        if preloaded is not None:
            B, H, W = (int(v) for v in preloaded)
        else:
            B, _, H, W = x.shape
        rplan = m._plan_for(B, H, W, self.device, 'dense', 'fp16')
        hst = heads._state(rplan, B, H, W)
        st = self._state(rplan, hst)
        heads.refresh(hst)
        self.refresh(st)
        return _fusion_function().apply(self, st, x, preloaded, *[p for _, p in self.named_parameters()])

    def backward_explicit(self, st, dlogits, out=None):
        """The heads' chain, then the fusion chain, for the forward that left ``st``: -> {parameter name: fp32 gradient}."""
        import torch
        if self._plans.get(id(st['plan'])) is not st:
            raise RuntimeError('TrainableFusion: stale plan - the plan of this forward was rebuilt since (load_state_dict, export_to or eviction)')
        grads = self.heads.backward_explicit(st['hst'], dlogits, out)
        dw = []
        for names in self._wnames:
            row = []
            for n in names:
                t = out[n] if out is not None else torch.empty_like(self._params[n].detach())
                grads[n] = t
                row.append(t)
            dw.append(row)
        fb = st['fb']
        dz = ht.hb_map(st['hst']['hb'].dz.data_ptr(), 256, 0)
        fb.run(dz, st['us'], st['xs'], self._wr, dw)
        self._last = st
        return grads

    def input_grads(self, fp32=False):
        """The gradients the last backward left at the inputs of the fusion: {'z0', 'kfpn_h3', 'kfpn_h4', 'kfpn_h5'}.  fp16 NHWC
        device tensors (views), 'z0' (dz itself: the same tensor, no copy) times grad_scale and the others times grad_scale *
        fusion_scale; with ``fp32=True`` fresh fp32 NCHW tensors, unscaled.  The kfpn_h* entries are the FUSION-PATH terms only:
        fpn_train.TrainableNeck adds the kfpn_up path."""
        if self._last is None:
            raise RuntimeError('TrainableFusion.input_grads: run a backward first')
        fb = self._last['fb']
        out = {'z0': (self._last['hst']['hb'].dz, self.S)}
        for l, L in enumerate(FUSION_LEVELS):
            out['kfpn_h%d' % L] = (fb.dx[l][0][:, 1:-1, 1:-1], self.S * self.T)
        if not fp32:
            return {k: v for k, (v, _) in out.items()}
        return {k: v.permute(0, 3, 1, 2).float().div_(s).contiguous() for k, (v, s) in out.items()}


_FusionFunction = None


def _fusion_function():
    """The autograd node of TrainableFusion.__call__ (made on first use: this module imports without torch)."""
    global _FusionFunction
    if _FusionFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class _FusionFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, fusion, st, x, preloaded, *params):
                logits = fusion.model.forward_logits(x, preloaded=preloaded, heads='dense', head_precision='fp16')
                ctx.fusion, ctx.st, ctx.stamp = fusion, st, st['plan'].z_stamp
                ctx.shapes = [tuple(t.shape) for t in logits]
                return tuple(logits)

            @staticmethod
            @once_differentiable
            def backward(ctx, *grads):
                fusion, st = ctx.fusion, ctx.st
                if getattr(st['plan'], 'z_stamp', None) != ctx.stamp:
                    raise RuntimeError('TrainableFusion: stale plan - another forward of this shape has overwritten the saved activations')
                dl = [g.contiguous().float() if g is not None else torch.zeros(sh, dtype=torch.float32, device=fusion.device)
                      for g, sh in zip(grads, ctx.shapes)]
                got = fusion.backward_explicit(st, dl)
                return (None, None, None, None) + tuple(got[n] for n, _ in fusion.named_parameters())

    return _FusionFunction
