"""Backward pass of the FPN half of the neck on the device (include/rtm3d_hip.h, "neck FPN backward"; csrc/neck_fpn_backward.hip).

``TrainableNeck(heads)`` takes the hand-off of ``TrainableFusion`` - dz0 and the fusion-path terms of d kfpn_h3 / h4 / h5 - through

    h5 = head5(feat3);   x_{i-1} = proj_i(cat[up_i(h_i), feat_{i-1}]),   h_{i-1} = head_{i-1}(x_{i-1}),   i = 5, 4, 3;   z0 = h2

(models/nets/keypoint_fpn_fusion.py, _fpn) to every ``kfpn_head*`` / ``kfpn_proj*`` weight and bias and every ``kfpn_up*`` weight, which
become trainable next to the heads' and the fusion's parameters, and to the gradients at feat0 .. feat3, the hand-off to a later
backbone backward::

    heads = TrainableHeads(model, input_grad=True)
    neck = TrainableNeck(heads)                         # heads + fusion + FPN: every parameter behind the backbone
    solver = optim.Solver(neck, cfg)
    loss, items = RTM3DLoss(cfg)(neck(x), targets)
    solver.step(loss)

The plan runs head_{i-1} o proj_i as ONE composed 1x1 conv over the concat tensor [up | feat] (plan.py, _compose: A = Wh Wp,
b = Wh bp + bh), so the backward is the composed conv's, and the FACTOR RULE gives the reference's own gradients from it exactly
(nothing non-linear stands between the two): dWh = dA Wp^T + db bp^T, dWp = Wh^T dA, dbh = db, dbp = Wh^T db (head's input is
Wp ncat + bp, so proj's bias reaches head's weight) - weight-sized products, done by
torch on the device in fp64 and stored as fp32.  The default lowering folds the composed conv INTO kfpn_up (plan._neck_up_folds) and
keeps neither the concat tensors nor kfpn_up's output, so TrainableNeck runs the model on its TRAINING lowering
(``Model._plan_for(neck_fold=False)``), a plan of its own next to the default one.

``FpnBackward`` is the chain itself on raw maps, level after level from the map of z0 upwards: 1x1 wgrad and dgrad of the composed
conv, wgrad and dgrad of kfpn_up (rtm3d_neck_deconv_*, unchanged), and the sum of the FPN path and the fusion path at kfpn_h*.

``fpn_scale`` (a power of two, U): from the first dgrad on, every gradient activation is stored times S U (S: the heads' grad_scale);
the fusion's terms arrive times S T and are added times U / T.  dz times S T would overflow fp16 (0.052 x 2 ** 22), so the FPN
needs a scale of its own.  The default is measured, not guessed (tools/gpu_fpn_grad_scale.py, profiles/neck_fpn_backward.txt,
section 1):
%s
Labels or weights with larger gradients want a smaller U: an overflow shows as Inf / NaN parameter gradients, which ``nonfinite()``
counts.

LEFT UNDONE: the backbone backward (``input_grads()['feat*']`` is its hand-off); graph-replayed plans; head_precision='mxfp8';
training BatchNorm.
"""
import ctypes

import numpy as np

from . import _lib
from . import head_train as ht
from . import neck_train as nt

SCALE_TABLE = """\
    on the loss-gradient fixture's labels (fx_b1, fx_b2_empty; 24 x 40 map) with synth_state_dict weights, through the model, the
    fp64 reference's largest gradient activations behind dz (max |dz| = 0.052) are, unscaled,
        max |D_0| = 3.2e-2, |D_1| = 3.9e-2, |D_2| = 3.8e-2, |d feat3| = 1.7e-2 (medians of the non-zero elements: 5.5e-5 .. 1.4e-3),
        max |E_0| = 4.1e-2, |E_1| = 4.9e-2, |E_2| = 2.2e-2,   max |g_1| = 4.1e-2, |g_2| = 4.9e-2, |g_3| = 2.2e-2;
    with S = 2 ** 14 no non-zero reference element lies below fp16's smallest normal at any U >= 1, and
        U = 1: S U max = 810   U = 4: 3240   U = 16: 12961 (> 65504 / 16)
    so 2 ** 2 is the largest power of two U that keeps S U x 4.94e-2 = 3240 sixteen times below fp16's 65504.
"""
__doc__ = __doc__ % SCALE_TABLE

DEFAULT_FPN_SCALE = 4.0
DEFAULT_SLICE_WORKGROUPS = 1536           # wgrad workgroups a launch aims at: 2 co tiles x ceil(Cin / 128) ci tiles x slices (three resident per
                                          # CU by registers; a workgroup's tiles run one after the other, one prefetch deep)
FPN_LEVELS = (3, 4, 5)                    # the reference's level numbers of kfpn_up / kfpn_proj at chain levels k = 0, 1, 2
OC = 256


def check(B, H, W, Cin, factor):
    """The host check of one 1x1-conv backward (rtm3d_fpn_backward_check; runs without a GPU).  Raises RuntimeError."""
    _lib.check(_lib.load().rtm3d_fpn_backward_check(int(B), int(H), int(W), int(Cin), float(factor)), 'fpn_backward_check')


def default_slices(Cin):
    return max(1, min(256, DEFAULT_SLICE_WORKGROUPS // (2 * -(-int(Cin) // 128))))


def transpose_weights(a16):
    """fp16 1x1 weight (256, Cin) or (256, Cin, 1, 1) -> the dgrad operand [ci][co] (same device)."""
    return a16.reshape(a16.shape[0], a16.shape[1]).t().contiguous()


def param_names():
    """The reference's state-dict keys of the FPN half, top level first."""
    out = []
    for L in (5, 4, 3):
        out += ['kfpn_fusion.kfpn_head%d.weight' % L, 'kfpn_fusion.kfpn_head%d.bias' % L, 'kfpn_fusion.kfpn_up%d.conv_tran.weight' % L,
                'kfpn_fusion.kfpn_proj%d.weight' % L, 'kfpn_fusion.kfpn_proj%d.bias' % L]
    return out + ['kfpn_fusion.kfpn_head2.weight', 'kfpn_fusion.kfpn_head2.bias']


class FpnBackward(object):
    """The FPN-backward chain for one geometry, on raw maps.  B, H, W: batch and MAP size (of z0); feat_channels: channels of
    feat0 .. feat3, so level k = 0, 1, 2 works at (H >> k) x (W >> k) on Cin = 256 + feat_channels[k] channels and kfpn_head5 at
    (H >> 3) x (W >> 3) on feat_channels[3].  Owns the gradient maps (cleared once: the launches write interiors only), the
    workspace and the non-finite counter.  ``run`` issues the launches on the current stream and never synchronises.

    D[k]: (B, (H >> k) + 2, (W >> k) + 2, Cin_k), zero border 1: channels 0 .. 255 the gradient at kfpn_up{k + 3}'s output, the rest
    d feat_k.  E[k], g[k] (k = 0, 1, 2): (B, H >> (k + 1), W >> (k + 1), 256), the FPN-path term and the FULL gradient at
    kfpn_h{k + 3}.  dfeat3: (B, H >> 3, W >> 3, feat_channels[3]).  All times S U."""

    def __init__(self, B, H, W, device, feat_channels=(64, 128, 256, 512), grad_scale=ht.DEFAULT_GRAD_SCALE, fusion_scale=None,
                 fpn_scale=None, want_slices=None):
        import torch
        fusion_scale = nt.DEFAULT_FUSION_SCALE if fusion_scale is None else fusion_scale
        fpn_scale = DEFAULT_FPN_SCALE if fpn_scale is None else fpn_scale
        for what, v in (('grad_scale', grad_scale), ('fusion_scale', fusion_scale), ('fpn_scale', fpn_scale)):
            if not ht._is_pow2(v):
                raise ValueError('fpn backward: %s = %r is no power of two' % (what, v))
        if len(feat_channels) != 4:
            raise ValueError('fpn backward: four feature widths (feat0 .. feat3), got %r' % (feat_channels,))
        if H % 8 or W % 8:
            raise ValueError('fpn backward: the map is %d x %d, three levels need multiples of 8' % (H, W))
        self.B, self.H, self.W = int(B), int(H), int(W)
        self.S, self.T, self.U = float(grad_scale), float(fusion_scale), float(fpn_scale)
        self.fch = [int(c) for c in feat_channels]
        self.cin = [OC + c for c in self.fch[:3]] + [self.fch[3]]
        for k in range(4):
            check(self.B, self.H >> k, self.W >> k, self.cin[k], 1.0 / self.S if k == 0 else 1.0 / (self.S * self.U))
        check(self.B, self.H, self.W, self.cin[0], self.U)
        check(self.B, self.H, self.W, self.cin[0], self.U / self.T)
        nt.check(self.B, self.H, self.W, 3, self.S, self.U)                   # kfpn_up*: the fusion's transposed-conv entries with T := U
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.want = [int(want_slices) if want_slices is not None else default_slices(c) for c in self.cin]
        self.want_up = int(want_slices) if want_slices is not None else nt.default_slices()
        lib = _lib.load()
        nbytes = 0
        for k in range(4):
            n = ht.slices(self.B * (self.H >> k) * (self.W >> k), self.want[k])[0]
            nbytes = max(nbytes, int(lib.rtm3d_fpn_backward_workspace_bytes(self.cin[k], n)))
        for k in range(3):
            n = ht.slices(self.B * (self.H >> (k + 1)) * (self.W >> (k + 1)), self.want_up)[0]
            nbytes = max(nbytes, int(lib.rtm3d_neck_backward_workspace_bytes(self.B, 1, n)))
        z16 = lambda h, w, c, p: torch.zeros(self.B, h + 2 * p, w + 2 * p, c, dtype=torch.float16, device=self.device)
        self.D = [z16(self.H >> k, self.W >> k, self.cin[k], 1) for k in range(3)]
        self.E = [z16(self.H >> (k + 1), self.W >> (k + 1), OC, 0) for k in range(3)]
        self.g = [z16(self.H >> (k + 1), self.W >> (k + 1), OC, 0) for k in range(3)]
        self.dfeat3 = z16(self.H >> 3, self.W >> 3, self.cin[3], 0)
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=self.device)

    def hw(self, k):
        return self.H >> k, self.W >> k

    def run(self, dz, ncat, h, feat3, F, wr, wur, dA, db, dwu):
        """dz: rtm3d_hb_map of the H x W gradient of z0 (times S).  ncat[k] (k = 0 .. 2): map of the concat tensor, Cin_k channels
        from its coff.  h[k]: map of kfpn_h{k + 3}.  feat3: map of feat3.  F[k]: map of the fusion-path term of d kfpn_h{k + 3}
        (times S T).  wr[k] (k = 0 .. 3): fp16 [Cin_k][256], the transposed 1x1 weights as the forward used them (3: kfpn_head5).
        wur[k]: the rotated fp16 weight of kfpn_up{k + 3} (neck_train.rotate_deconv_weights).  Outputs, fp32 device tensors or None
        (skipped): dA[k] (256, Cin_k, 1, 1), db[k] (256,), k = 0 .. 3; dwu[k] (256, 256, 4, 4), k = 0 .. 2."""
        import torch
        lib = _lib.load()
        B = self.B
        for k in range(4):
            for t, shape, what in ((dA[k], (OC, self.cin[k], 1, 1), 'dA'), (db[k], (OC,), 'db'), (dwu[k] if k < 3 else None, (OC, OC, 4, 4), 'dwu')):
                if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32
                                      or not t.is_contiguous() or t.device != self.device):
                    raise ValueError('fpn backward: %s[%d] must be a contiguous fp32 %s tensor on %s' % (what, k, shape, self.device))
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            ws, nws, ctr = self.ws.data_ptr(), self.ws.numel() * 4, self.nonfinite.data_ptr()
            g = dz
            for k in range(4):
                Hk, Wk = self.hw(k)
                x = ncat[k] if k < 3 else feat3
                inv = 1.0 / self.S if k == 0 else 1.0 / (self.S * self.U)
                _lib.check(lib.rtm3d_fpn_conv1x1_wgrad(st, B, Hk, Wk, self.cin[k], ctypes.byref(x), ctypes.byref(g), inv, ptr(dA[k]), ptr(db[k]),
                                                       self.want[k], ws, nws, ctr), 'fpn_conv1x1_wgrad')
                out = ht.hb_map(self.D[k].data_ptr(), self.cin[k], 1) if k < 3 else ht.hb_map(self.dfeat3.data_ptr(), self.cin[3], 0)
                _lib.check(lib.rtm3d_fpn_conv1x1_dgrad(st, B, Hk, Wk, self.cin[k], ctypes.byref(g), wr[k].data_ptr(), self.U if k == 0 else 1.0,
                                                       ctypes.byref(out)), 'fpn_conv1x1_dgrad')
                if k == 3:
                    break
                Hi, Wi = self.hw(k + 1)
                dy = out                                                      # channels 0 .. 255 of the Cin-channel map
                _lib.check(lib.rtm3d_neck_deconv_wgrad(st, B, Hi, Wi, ctypes.byref(h[k]), ctypes.byref(dy), self.S, self.U, ptr(dwu[k]),
                                                       self.want_up, ws, nws, ctr), 'neck_deconv_wgrad')
                e = ht.hb_map(self.E[k].data_ptr(), OC, 0)
                _lib.check(lib.rtm3d_neck_deconv_dgrad(st, B, Hi, Wi, ctypes.byref(dy), wur[k].data_ptr(), ctypes.byref(e)), 'neck_deconv_dgrad')
                g = ht.hb_map(self.g[k].data_ptr(), OC, 0)
                _lib.check(lib.rtm3d_fpn_grad_add(st, B, Hi, Wi, ctypes.byref(e), ctypes.byref(F[k]), self.U / self.T, ctypes.byref(g)), 'fpn_grad_add')


# --------------------------------------------------------------------------------------------------- through the model
def conv_launch_names():
    """Names of the plan's four 1x1 launches, chain level k = 0 .. 3."""
    return ['kfpn_proj3+head2', 'kfpn_proj4+head3', 'kfpn_proj5+head4', 'kfpn_head5']


def gather_tables(params_off, derived_off, cin, launches):
    """The gather tables of the FPN's packed forward arrays.  params_off / derived_off: arena offsets of the parameters (by their
    reference key) and of the composed ('A', k) / ('b', k), k = 0 .. 2.  launches: {launch name: (packer, cout_pad)} as the recorder
    used them (RealizedPlan.param_blobs, or plan.lower + plan._CONV_PACKING).  -> {launch name: (weight perm, bias perm or None)}."""
    out = {}
    for k, name in enumerate(conv_launch_names()):
        pack, cout_pad = launches[name]
        w0 = derived_off[('A', k)] if k < 3 else params_off['kfpn_fusion.kfpn_head5.weight']
        b0 = derived_off[('b', k)] if k < 3 else params_off['kfpn_fusion.kfpn_head5.bias']
        src = (w0 + np.arange(OC * cin[k], dtype=np.int64)).reshape(1, OC, cin[k])                  # (taps, cout, cin)
        bp = np.full(cout_pad, -1, np.int32)
        bp[:OC] = b0 + np.arange(OC)
        out[name] = (ht.perm_through(pack, src), bp)
    for L in FPN_LEVELS:
        pack, _ = launches['kfpn_up%d' % L]
        idx = params_off['kfpn_fusion.kfpn_up%d.conv_tran.weight' % L] + np.arange(OC * OC * 16, dtype=np.int64).reshape(OC, OC, 4, 4)
        out['kfpn_up%d' % L] = (np.concatenate([ht.perm_through(pack, s) for s in nt._deconv_group_src(idx)]), None)
    return out


class TrainableNeck(object):
    """The whole neck of ``heads.model`` - fusion and FPN - as trainable fp32 CUDA leaves next to the heads' parameters; see the
    module docstring.  ``heads``: a TrainableHeads built with ``input_grad=True``.  Composes a ``TrainableFusion``;
    ``named_parameters`` / ``parameters`` / ``state_dict(keep_vars=)`` / ``export_to`` cover the heads', the fusion's and the FPN's
    parameters, so ``optim.Solver(neck, cfg)`` and ``ModelEMA`` work unchanged.

    ``neck(x)`` / ``neck(None, preloaded=(B, H, W))`` composes A and b on the device (fp64 product, then fp32), refreshes every
    packed array of the three stages, runs the model's dense fp16 plan of the TRAINING lowering and returns the logit maps under
    ONE autograd node whose backward runs the heads' chain, the fusion chain, the FPN chain and the factor rule.  The
    predecessors' refusals hold (mxfp8, graph-replayed plans, stale plans, overlapping tensors); refused as well: a plan that
    took the neck fold."""

    def __init__(self, heads, fusion_scale=None, fpn_scale=None, want_slices=None):
        import torch
        self.fusion = nt.TrainableFusion(heads, fusion_scale, want_slices)
        fpn_scale = DEFAULT_FPN_SCALE if fpn_scale is None else fpn_scale
        if not ht._is_pow2(fpn_scale):
            raise ValueError('TrainableNeck: fpn_scale = %r is no power of two' % (fpn_scale,))
        self.heads, self.model, self.device = heads, heads.model, heads.device
        self.S, self.T, self.U, self.want_slices = heads.S, self.fusion.T, float(fpn_scale), want_slices
        sd = self.model.state_dict()
        self._names = param_names()
        for n in self._names:
            if n not in sd:
                raise NotImplementedError('TrainableNeck: the model has no %s' % n)
        shape = lambda n: tuple(sd[n].shape)
        self.fch = [shape('kfpn_fusion.kfpn_proj%d.weight' % L)[0] for L in FPN_LEVELS] + [shape('kfpn_fusion.kfpn_head5.weight')[1]]
        self.cin = [OC + c for c in self.fch[:3]] + [self.fch[3]]
        want = {}
        for k, L in enumerate(FPN_LEVELS):
            want.update({'kfpn_fusion.kfpn_proj%d.weight' % L: (self.fch[k], self.cin[k], 1, 1), 'kfpn_fusion.kfpn_proj%d.bias' % L: (self.fch[k],),
                         'kfpn_fusion.kfpn_head%d.weight' % (L - 1): (OC, self.fch[k], 1, 1), 'kfpn_fusion.kfpn_head%d.bias' % (L - 1): (OC,),
                         'kfpn_fusion.kfpn_up%d.conv_tran.weight' % L: (OC, OC, 4, 4)})
        want.update({'kfpn_fusion.kfpn_head5.weight': (OC, self.fch[3], 1, 1), 'kfpn_fusion.kfpn_head5.bias': (OC,)})
        for n in self._names:
            if shape(n) != want[n]:
                raise NotImplementedError('TrainableNeck: %s is %s, the FPN of a 256-channel neck has %s' % (n, shape(n), want[n]))
        for c in self.cin:
            check(1, 1, 1, c, 1.0)
        # the arena: the parameters, then the composed A_k and b_k (k = 0 .. 2), every start 16-byte aligned
        sizes = [int(sd[n].numel()) for n in self._names]
        derived = [(('A', k), OC * self.cin[k]) for k in range(3)] + [(('b', k), OC) for k in range(3)]
        offs = np.concatenate([[0], np.cumsum([-(-n // 4) * 4 for n in sizes + [n for _, n in derived]])]).astype(np.int64)
        self._off = dict(zip(self._names, offs[:len(sizes)].tolist()))
        self._doff = dict(zip([key for key, _ in derived], offs[len(sizes):-1].tolist()))
        self._arena = torch.zeros(int(offs[-1]), dtype=torch.float32, device=self.device)
        self._params = {}
        for n, size in zip(self._names, sizes):
            v = self._arena[self._off[n]:self._off[n] + size].view(sd[n].shape)
            v.copy_(sd[n])
            self._params[n] = v.requires_grad_()
        self._A = [self._arena[self._doff[('A', k)]:self._doff[('A', k)] + OC * self.cin[k]].view(OC, self.cin[k]) for k in range(3)]
        self._b = [self._arena[self._doff[('b', k)]:self._doff[('b', k)] + OC] for k in range(3)]
        self._bn = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64, device=self.device)          # row 0: no BatchNorm
        self._scale_of = torch.zeros(int(offs[-1]), dtype=torch.int32, device=self.device)
        # the dgrad operands: refreshed by the same launch as the plan's blobs
        self._wr = [torch.zeros(self.cin[k], OC, dtype=torch.float16, device=self.device) for k in range(4)]
        self._wur = [torch.zeros(16, OC, OC, dtype=torch.float16, device=self.device) for _ in FPN_LEVELS]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).astype(np.int32)).to(self.device)
        self._wr_perm = [up(self._asrc(k).T) for k in range(4)]
        self._wur_perm = [up(self._usrc(L).transpose(2, 3, 0, 1)) for L in FPN_LEVELS]
        self._plans = {}
        self._last = None

    def _asrc(self, k):
        """Arena index of every element of the 1x1 weight the forward uses at chain level k, shaped (256, Cin_k)."""
        w0 = self._doff[('A', k)] if k < 3 else self._off['kfpn_fusion.kfpn_head5.weight']
        return w0 + np.arange(OC * self.cin[k], dtype=np.int64).reshape(OC, self.cin[k])

    def _usrc(self, L):
        return self._off['kfpn_fusion.kfpn_up%d.conv_tran.weight' % L] + np.arange(OC * OC * 16, dtype=np.int64).reshape(OC, OC, 4, 4)

    # ---- nn.Module-like surface
    def named_parameters(self):
        return iter(list(self.fusion.named_parameters()) + list(self._params.items()))

    def parameters(self):
        return iter([p for _, p in self.named_parameters()])

    def state_dict(self, keep_vars=False):
        out = self.fusion.state_dict(keep_vars=keep_vars)
        for k, v in self._params.items():
            out[k] = v if keep_vars else v.detach()
        return out

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def export_to(self, model=None):
        """Write the heads', the fusion's and the FPN's parameters back through ``model.load_state_dict``."""
        model = self.model if model is None else model
        sd = model.state_dict()
        for k, v in self.named_parameters():
            sd[k] = v.detach().cpu()
        model.load_state_dict(sd)
        if model is self.model:
            self._plans, self.fusion._plans, self.heads._plans = {}, {}, {}
        return model

    def nonfinite(self):
        """Non-finite parameter-gradient elements produced so far, the heads' and the fusion's included."""
        return self.fusion.nonfinite() + sum(int(st['fpn'].nonfinite.item()) for st in self._plans.values())

    # ---- per-plan state
    def _map_of(self, rplan, s, what, hw, width):
        low = rplan.lowering
        key = (s.tid, s.coff, s.C)
        if key in low['s2d_only'] or key in low['unwritten'] or s.tid in low['widen']:
            raise NotImplementedError('TrainableNeck: the plan does not keep %s as a plain written tensor' % what)
        addr, b, h, w, C, P = rplan.tensor_info(s)
        if (b, h, w) != (rplan.plan.B,) + tuple(hw) or s.C != width or s.coff + width > C:
            raise RuntimeError('TrainableNeck: %s is %s (slice of %d at %d), not the FPN geometry' % (what, (b, h, w, C), s.C, s.coff))
        return ht.hb_map(addr, C, P, s.coff), (addr, addr + 2 * b * (h + 2 * P) * (w + 2 * P) * C, what)

    def _state(self, rplan, fst):
        import torch
        st = self._plans.get(id(rplan))
        if st is not None and st['plan'] is rplan and st['fst'] is fst:
            return st
        if getattr(rplan, 'neck_fold', None) is not False or rplan.lowering['widen']:
            raise NotImplementedError('TrainableNeck: the plan took the neck fold; the FPN backward needs the training lowering '
                                      '(Model._plan_for(neck_fold=False))')
        if rplan.graph_stats()[2]:
            raise NotImplementedError('TrainableNeck: the plan replays a captured graph; set model.use_graph = False')
        B, H, W = fst['hst']['shape']
        Hm, Wm = H // 4, W // 4
        ops = {op.get('name'): op for op in rplan.plan.ops}
        named = rplan.plan.named
        ncat, hmaps, spans = [], [], {}
        names = conv_launch_names()
        for k in range(4):
            op = ops.get(names[k])
            if op is None or op.get('groups') != 1 or tuple(op['w'].shape) != (1, 1, OC, self.cin[k]):
                raise NotImplementedError('TrainableNeck: the plan has no 1x1 launch %s of %d -> 256 channels' % (names[k], self.cin[k]))
            m, span = self._map_of(rplan, op['inp'][0], 'the input of ' + names[k], (Hm >> k, Wm >> k), self.cin[k])
            ncat.append(m); spans[span[0]] = span
            out_name = 'z0' if k == 0 else 'kfpn_h%d' % (k + 2)
            if (op['out'][0].tid, op['out'][0].coff) != (named[out_name].tid, named[out_name].coff):
                raise RuntimeError('TrainableNeck: %s does not write %s' % (names[k], out_name))
        if (ops[names[3]]['inp'][0].tid, ops[names[3]]['inp'][0].coff) != (named['feat3'].tid, named['feat3'].coff):
            raise RuntimeError('TrainableNeck: kfpn_head5 does not read feat3')
        for k, L in enumerate(FPN_LEVELS):
            op = ops.get('kfpn_up%d' % L)
            if op is None or op.get('groups') != 4 or tuple(op['w'].shape) != (4, 4, OC, OC):
                raise NotImplementedError('TrainableNeck: the plan has no four-phase 256 -> 256 launch kfpn_up%d' % L)
            if (op['inp'][0].tid, op['inp'][0].coff) != (named['kfpn_h%d' % L].tid, named['kfpn_h%d' % L].coff):
                raise RuntimeError('TrainableNeck: kfpn_up%d does not read kfpn_h%d' % (L, L))
            o = op['out'][0]
            if o.tid != ops[names[k]]['inp'][0].tid or o.coff != 0 or o.C != OC:
                raise RuntimeError('TrainableNeck: kfpn_up%d does not write channels 0 .. 255 of the concat tensor' % L)
            m, span = self._map_of(rplan, op['inp'][0], 'kfpn_h%d' % L, (Hm >> (k + 1), Wm >> (k + 1)), OC)
            hmaps.append(m); spans[span[0]] = span
        for nm in ('z0', 'z', 'h1', 'h2', 'u3', 'u4', 'u5'):
            if nm in named:
                addr, b, h, w, C, P = rplan.tensor_info(named[nm])
                spans[addr] = (addr, addr + 2 * b * (h + 2 * P) * (w + 2 * P) * C, nm)
        order = sorted(spans.values())
        for (a0, a1, na), (b0, b1, nb) in zip(order, order[1:]):
            if b0 < a1:
                raise NotImplementedError('TrainableNeck: %s and %s overlap in device memory: a saved activation may be overwritten' % (na, nb))
        launches = {rec['name']: (rec['pack'], rec['cout_pad']) for rec in rplan.param_blobs if rec['name'] in set(names) | {'kfpn_up%d' % L for L in FPN_LEVELS}}
        if len(launches) != 7:
            raise RuntimeError('TrainableNeck: found %d of 7 packed kfpn arrays in the plan' % len(launches))
        blobs = {rec['name']: rec for rec in rplan.param_blobs if rec['name'] in launches}
        table, keep = [], []
        for name, (wperm, bperm) in gather_tables(self._off, self._doff, self.cin, launches).items():
            for perm, bid, kind in ((wperm, blobs[name]['w_blob'], 0), (bperm, blobs[name]['bias_blob'], 1)):
                if perm is None:
                    continue
                if perm.size * (2 if kind == 0 else 4) != rplan.blob_bytes(bid) or perm.max() >= self._arena.numel():
                    raise RuntimeError('TrainableNeck: a gather table of %s does not match its blob' % name)
                d = torch.from_numpy(perm).to(self.device)
                keep.append(d)
                table.append((rplan.blob_address(bid), d.data_ptr(), perm.size, kind, 0))
        for t, p in list(zip(self._wr, self._wr_perm)) + list(zip(self._wur, self._wur_perm)):
            table.append((t.data_ptr(), p.data_ptr(), t.numel(), 0, 0))
        c_jobs = (_lib.HbRefreshJobC * len(table))(*[_lib.HbRefreshJobC(*j) for j in table])
        _lib.check(_lib.load().rtm3d_head_refresh_check(len(table), c_jobs), 'head_refresh_check')
        d_jobs = torch.frombuffer(bytearray(ctypes.string_at(c_jobs, ctypes.sizeof(c_jobs))), dtype=torch.uint8).to(self.device)
        fpn = FpnBackward(B, Hm, Wm, self.device, self.fch, self.S, self.T, self.U, self.want_slices)
        feat3 = ncat.pop()
        st = {'plan': rplan, 'fst': fst, 'hst': fst['hst'], 'ncat': ncat, 'h': hmaps, 'feat3': feat3, 'jobs': c_jobs, 'd_jobs': d_jobs,
              'keep': keep, 'fpn': fpn}
        self._plans = {k: v for k, v in self._plans.items() if v['plan'].ctx}
        self._plans[id(rplan)] = st
        return st

    def compose(self):
        """A_k = Wh Wp, b_k = Wh bp + bh into the arena: the fp64 product, then fp32 (plan.py, _compose)."""
        import torch
        with torch.no_grad():
            for k, L in enumerate(FPN_LEVELS):
                wh = self._params['kfpn_fusion.kfpn_head%d.weight' % (L - 1)].detach().view(OC, self.fch[k]).double()
                wp = self._params['kfpn_fusion.kfpn_proj%d.weight' % L].detach().view(self.fch[k], self.cin[k]).double()
                self._A[k].copy_(wh @ wp)
                self._b[k].copy_(wh @ self._params['kfpn_fusion.kfpn_proj%d.bias' % L].detach().double()
                                 + self._params['kfpn_fusion.kfpn_head%d.bias' % (L - 1)].detach().double())

    def refresh(self, st=None):
        """Compose A and b, then rebuild on the device, in one launch per plan, the packed forward weights and fp32 biases of the
        four 1x1 launches, the packed weights of the three kfpn_up launches and the dgrad copies (rtm3d_head_refresh, no BatchNorm)."""
        import torch
        self.compose()
        for s in ([st] if st is not None else list(self._plans.values())):
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().rtm3d_head_refresh(_lib.stream_ptr(self.device), len(s['jobs']), s['jobs'], s['d_jobs'].data_ptr(),
                                                          self._arena.data_ptr(), self._scale_of.data_ptr(), self._bn.data_ptr()), 'head_refresh')

    # ---- forward / backward
    def __call__(self, x, preloaded=None):
        heads, fusion, m = self.heads, self.fusion, self.model
        if preloaded is not None:
            B, H, W = (int(v) for v in preloaded)
        else:
            B, _, H, W = x.shape
        rplan = m._plan_for(B, H, W, self.device, 'dense', 'fp16', neck_fold=False)
        hst = heads._state(rplan, B, H, W)
        fst = fusion._state(rplan, hst)
        st = self._state(rplan, fst)
        heads.refresh(hst)
        fusion.refresh(fst)
        self.refresh(st)
        return _neck_function().apply(self, st, x, preloaded, *[p for _, p in self.named_parameters()])

    def backward_explicit(self, st, dlogits, out=None):
        """The heads' chain, the fusion chain, the FPN chain and the factor rule for the forward that left ``st``:
        -> {parameter name: fp32 gradient}."""
        import torch
        if self._plans.get(id(st['plan'])) is not st:
            raise RuntimeError('TrainableNeck: stale plan - the plan of this forward was rebuilt since (load_state_dict, export_to or eviction)')
        grads = self.fusion.backward_explicit(st['fst'], dlogits, out)
        new = lambda n: out[n] if out is not None else torch.empty_like(self._params[n].detach())
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        dA = [f32(OC, self.cin[k], 1, 1) for k in range(3)] + [new('kfpn_fusion.kfpn_head5.weight')]
        db = [f32(OC) for k in range(3)] + [new('kfpn_fusion.kfpn_head5.bias')]
        dwu = [new('kfpn_fusion.kfpn_up%d.conv_tran.weight' % L) for L in FPN_LEVELS]
        fb = st['fst']['fb']
        F = [fb.dx_map(l, 0) for l in range(3)]
        dz = ht.hb_map(st['hst']['hb'].dz.data_ptr(), OC, 0)
        st['fpn'].run(dz, st['ncat'], st['h'], st['feat3'], F, self._wr, self._wur, dA, db, dwu)
        grads['kfpn_fusion.kfpn_head5.weight'], grads['kfpn_fusion.kfpn_head5.bias'] = dA[3], db[3]
        for k, L in enumerate(FPN_LEVELS):
            grads['kfpn_fusion.kfpn_up%d.conv_tran.weight' % L] = dwu[k]
            nh, npj = 'kfpn_fusion.kfpn_head%d' % (L - 1), 'kfpn_fusion.kfpn_proj%d' % L
            wh = self._params[nh + '.weight'].detach().view(OC, self.fch[k]).double()
            wp = self._params[npj + '.weight'].detach().view(self.fch[k], self.cin[k]).double()
            a64, b64 = dA[k].view(OC, self.cin[k]).double(), db[k].double()
            bp = self._params[npj + '.bias'].detach().double()
            for n, v in ((nh + '.weight', a64 @ wp.t() + torch.outer(b64, bp)), (npj + '.weight', wh.t() @ a64), (nh + '.bias', b64), (npj + '.bias', wh.t() @ b64)):
                grads[n] = new(n)
                grads[n].copy_(v.view(grads[n].shape))
        self._last = st
        return grads

    def input_grads(self, fp32=False):
        """The gradients the last backward left in front of every stage of the neck: {'z0', 'kfpn_h3', 'kfpn_h4', 'kfpn_h5', 'feat0',
        'feat1', 'feat2', 'feat3'}.  fp16 NHWC device tensors (views), 'z0' times grad_scale and the others times grad_scale *
        fpn_scale; with ``fp32=True`` fresh fp32 NCHW tensors, unscaled.  The kfpn_h* entries are the FULL gradients (fusion path
        plus kfpn_up path); feat0 .. feat3 are the hand-off to a backbone backward."""
        if self._last is None:
            raise RuntimeError('TrainableNeck.input_grads: run a backward first')
        fpn = self._last['fpn']
        su = self.S * self.U
        out = {'z0': (self._last['hst']['hb'].dz, self.S), 'feat3': (fpn.dfeat3, su)}
        for k, L in enumerate(FPN_LEVELS):
            out['kfpn_h%d' % L] = (fpn.g[k], su)
            out['feat%d' % k] = (fpn.D[k][:, 1:-1, 1:-1, OC:], su)
        if not fp32:
            return {k: v for k, (v, _) in out.items()}
        return {k: v.permute(0, 3, 1, 2).float().div_(s).contiguous() for k, (v, s) in out.items()}


_NeckFunction = None


def _neck_function():
    """The autograd node of TrainableNeck.__call__ (made on first use: this module imports without torch)."""
    global _NeckFunction
    if _NeckFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class _NeckFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, neck, st, x, preloaded, *params):
                logits = neck.model.forward_logits(x, preloaded=preloaded, heads='dense', head_precision='fp16', neck_fold=False)
                ctx.neck, ctx.st, ctx.stamp = neck, st, st['plan'].z_stamp
                ctx.shapes = [tuple(t.shape) for t in logits]
                return tuple(logits)

            @staticmethod
            @once_differentiable
            def backward(ctx, *grads):
                neck, st = ctx.neck, ctx.st
                if getattr(st['plan'], 'z_stamp', None) != ctx.stamp:
                    raise RuntimeError('TrainableNeck: stale plan - another forward of this shape has overwritten the saved activations')
                dl = [g.contiguous().float() if g is not None else torch.zeros(sh, dtype=torch.float32, device=neck.device)
                      for g, sh in zip(grads, ctx.shapes)]
                got = neck.backward_explicit(st, dl)
                return (None, None, None, None) + tuple(got[n] for n, _ in neck.named_parameters())

    return _NeckFunction
