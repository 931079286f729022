"""Backward pass of the detection heads on the device (include/rtm3d_hip.h, "head backward"; csrc/head_backward.hip).

``TrainableHeads(model)`` is what stands between ``RTM3DLoss`` and ``optim.Solver`` when the four heads of a pretrained
checkpoint are fine-tuned with the backbone and the neck frozen::

    heads = TrainableHeads(model)                       # the head convs' parameters as fp32 CUDA leaves
    solver = optim.Solver(heads, cfg)
    loss, items = RTM3DLoss(cfg)(heads(x), targets)     # the model's dense fp16 plan; logits with a grad_fn
    solver.step(loss)                                   # zero_grad, loss.backward() (rtm3d_loss_grad, then the chain below), Adamax;
                                                        # the next heads(x) refreshes the plan's packed weights on the device

``HeadBackward`` is the chain itself on raw maps (the forward's saved activations z, h1, h2 ... are the plan's own tensors):
go -> final-conv wgrad / dgrad -> per 256 -> 256 conv, last to first, wgrad and dgrad -> dz.

DEVIATION from the reference: BatchNorm is FROZEN (FrozenBatchNorm).  Running statistics and the affine pair are constants - the
function the folded plan computes; the reference trains BN on batch statistics.  Trainable: weight and bias of every head conv.

``grad_scale`` (a power of two, S): the fp16 gradient activations are stored times S, parameter gradients leave unscaled.  The
default, 2 ** 14, is measured, not guessed (tools/gpu_head_grad_scale.py, profiles/head_backward.txt): on the loss-gradient
fixture's labels (fx_b1, fx_b2_empty) with synth_state_dict weights the fp64 reference's largest gradient activations are
max |go| = 0.224, |dh2| = 0.023, |dh1| = 0.023, |dz| = 0.052 (unscaled), and 2 ** 14 is the largest power of two S that keeps
S x 0.224 = 3665 sixteen times below fp16's 65504.  Labels or weights with larger gradients want a smaller S: an overflow shows
as Inf / NaN parameter gradients, which ``nonfinite()`` counts.
"""
import ctypes

import numpy as np

from . import _lib
from . import plan as plan_mod
from .weights import head_table

DEFAULT_GRAD_SCALE = 16384.0
DEFAULT_SLICE_WORKGROUPS = 1024           # wgrad workgroups a launch aims at: 4 output tiles x 9 taps x G branches x slices


def _is_pow2(v):
    m, _ = np.frexp(float(v))
    return np.isfinite(v) and v > 0 and m == 0.5


def check(B, H, W, K, num_conv, grad_scale):
    """The host check of a head-backward geometry (rtm3d_head_backward_check; runs without a GPU).  Raises RuntimeError."""
    k = (ctypes.c_int * 4)(*(list(K) + [0] * 4)[:4])
    _lib.check(_lib.load().rtm3d_head_backward_check(int(B), int(H), int(W), len(K), k, int(num_conv), float(grad_scale)), 'head_backward_check')


def slices(npix, want):
    """(n_slices, tiles_per_slice) of the K-split over ``npix`` pixels when ``want`` slices are asked for."""
    n, t = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().rtm3d_head_backward_slices(int(npix), int(want), ctypes.byref(n), ctypes.byref(t)), 'head_backward_slices')
    return n.value, t.value


def default_slices(G):
    return max(1, min(64, -(-DEFAULT_SLICE_WORKGROUPS // (36 * G))))


def hb_map(ptr, C, P, coff=0, gstride=0):
    return _lib.HbMapC(ctypes.c_void_p(int(ptr)), int(C), int(P), int(coff), int(gstride))


def rotate_weights(wf16):
    """fp16 folded weights (G, cout, 256, 3, 3) -> the dgrad operand [G][tap][ci][cout padded to 16 / 256] (same device)."""
    import torch
    G, co, ci = wf16.shape[:3]
    kc = 16 if co <= 16 else 256
    out = torch.zeros(G, 9, ci, kc, dtype=torch.float16, device=wf16.device)
    out[..., :co] = wf16.reshape(G, co, ci, 9).permute(0, 3, 2, 1)
    return out.contiguous()


class HeadBackward(object):
    """The head-backward chain for one geometry, on raw maps.  B, H, W: batch and MAP size; K: output channels per head;
    num_conv: HEADER_NUM_CONV.  Owns the gradient maps (cleared once: the launches write interiors only), the workspace and the
    non-finite counter.  ``run`` issues the launches on the current stream and never synchronises."""

    def __init__(self, B, H, W, K, num_conv, device, grad_scale=DEFAULT_GRAD_SCALE, input_grad=False, want_slices=None):
        import torch
        self.B, self.H, self.W, self.K, self.G, self.num_conv = int(B), int(H), int(W), [int(k) for k in K], len(K), int(num_conv)
        if not _is_pow2(grad_scale):
            raise ValueError('head backward: grad_scale = %r is no power of two' % (grad_scale,))
        check(B, H, W, self.K, num_conv, grad_scale)
        self.S, self.input_grad, self.device = float(grad_scale), bool(input_grad), torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.want = int(want_slices) if want_slices is not None else default_slices(self.G)
        self.n_slices, self.tiles_per_slice = slices(self.B * self.H * self.W, self.want)
        G = self.G
        z16 = lambda *shape: torch.zeros(*shape, dtype=torch.float16, device=self.device)
        self.go = z16(B, H + 2, W + 2, G * 16)
        # dh[k]: the gradient at the output of conv k (1: the dilation-6 conv); its reader is that conv's dgrad
        self.dh = [None] + [z16(B, H + 2 * self._dil(k), W + 2 * self._dil(k), G * 256) for k in range(1, self.num_conv + 1)]
        self.dz = z16(B, H, W, 256) if self.input_grad else None
        nbytes = int(_lib.load().rtm3d_head_backward_workspace_bytes(G, self.n_slices))
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=self.device)

    @staticmethod
    def _dil(k):
        return 6 if k == 1 else 1

    def go_map(self):
        return hb_map(self.go.data_ptr(), self.G * 16, 1, 0, 16)

    def dh_map(self, k):
        return hb_map(self.dh[k].data_ptr(), self.G * 256, self._dil(k), 0, 256)

    def _wgrad(self, lib, st, dil, cout, valid, dy, x, scales, dws, dbs):
        G = self.G
        arr = lambda ts: (ctypes.c_void_p * 4)(*([t.data_ptr() if t is not None else None for t in ts] + [None] * (4 - G)))
        _lib.check(lib.rtm3d_head_wgrad(st, self.B, self.H, self.W, G, dil, cout, (ctypes.c_int * 4)(*(list(valid) + [0] * (4 - G))),
                                        ctypes.byref(dy), ctypes.byref(x), self.S, arr(scales if scales is not None else [None] * G),
                                        arr(dws), arr(dbs), self.want, self.ws.data_ptr(), self.ws.numel() * 4, self.nonfinite.data_ptr()),
                   'head_wgrad')

    def run(self, dlogits, acts, wr, wr_out, scales, dw, db, dwo, dbo):
        """dlogits: G contiguous fp32 (B, K[g], H, W) device tensors.  acts[k], k = 0 .. num_conv: rtm3d_hb_map of z (k = 0) and of
        conv k's output.  wr[k] (k = 1 .. num_conv; index 0 unused): rotated folded fp16 weights of conv k (rotate_weights);
        wr_out: of the final convs.  scales[k][g]: fp32 (256,) BN scale or None.  Outputs, each a list over g of fp32 tensors or None
        (skipped): dw[k], db[k] (k = 1 .. num_conv), dwo, dbo.  dz: self.dz when input_grad."""
        import torch
        lib = _lib.load()
        G, B, H, W = self.G, self.B, self.H, self.W
        for g, t in enumerate(dlogits):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, self.K[g], H, W) or t.dtype != torch.float32 or not t.is_contiguous() \
                    or t.device != self.device:
                raise ValueError('head backward: the gradient of logit map %d must be a contiguous fp32 %s tensor on %s'
                                 % (g, (B, self.K[g], H, W), self.device))
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            go = self.go_map()
            _lib.check(lib.rtm3d_head_go(st, B, H, W, G, (ctypes.c_int * 4)(*(self.K + [0] * (4 - G))),
                                         (ctypes.c_void_p * 4)(*([t.data_ptr() for t in dlogits] + [None] * (4 - G))), self.S, ctypes.byref(go)),
                       'head_go')
            n = self.num_conv
            self._wgrad(lib, st, 1, 16, self.K, go, acts[n], None, dwo, dbo)
            dhn = self.dh_map(n)
            _lib.check(lib.rtm3d_head_dgrad(st, B, H, W, G, 1, 1, 16, ctypes.byref(go), wr_out.data_ptr(), ctypes.byref(acts[n]), ctypes.byref(dhn)),
                       'head_dgrad')
            for k in range(n, 0, -1):
                dy = self.dh_map(k)
                self._wgrad(lib, st, self._dil(k), 256, [256] * G, dy, acts[k - 1], scales[k], dw[k], db[k])
                if k > 1:
                    out = self.dh_map(k - 1)
                    _lib.check(lib.rtm3d_head_dgrad(st, B, H, W, G, 1, 1, 256, ctypes.byref(dy), wr[k].data_ptr(), ctypes.byref(acts[k - 1]),
                                                    ctypes.byref(out)), 'head_dgrad')
                elif self.input_grad:
                    out = hb_map(self.dz.data_ptr(), 256, 0, 0, 0)
                    _lib.check(lib.rtm3d_head_dgrad(st, B, H, W, 1, G, 6, 256, ctypes.byref(dy), wr[1].data_ptr(), None, ctypes.byref(out)),
                               'head_dgrad')


# --------------------------------------------------------------------------------------------------- through the model
# Gather tables.  An index is sent through a packer as three base-2048 digits: each digit is an integer below 2048 and survives the
# packer's rounding to fp16 exactly.
def perm_through(pack, src_index):
    """The gather table of a packer: ``pack`` (fp32 array(s) -> a flat fp16 array, e.g. plan.pack_mfma_weights) applied to the
    digits of ``src_index`` (an int array of the packer's input shape, or a list of them where the packer takes a list) and to a
    plane of ones -> int32 [packed size]: packed[i] comes from source element perm[i], or is padding (-1)."""
    many = isinstance(src_index, (list, tuple))
    srcs = [np.asarray(s, np.int64) for s in (src_index if many else [src_index])]
    run = lambda planes: np.asarray(pack(planes if many else planes[0]), np.float32)
    digits = [run([((s >> (11 * i)) & 2047).astype(np.float32) for s in srcs]).astype(np.int64) for i in range(3)]
    valid = run([np.ones(s.shape, np.float32) for s in srcs])
    return np.where(valid != 0, digits[0] + (digits[1] << 11) + (digits[2] << 22), -1).astype(np.int32)


class TrainableHeads(object):
    """The head convs of ``model`` (an rtm3d_amd.Model on a GPU) as trainable fp32 CUDA leaves under the reference's state-dict
    keys; see the module docstring.  ``named_parameters`` / ``parameters`` / ``state_dict(keep_vars=)`` (the BN tensors as
    buffers) are what ``optim.Solver``, ``param_groups`` and ``ModelEMA`` need.

    ``heads(x)`` / ``heads(None, preloaded=(B, H, W))`` refreshes the plan's packed weights from the parameters (one launch,
    EVERY call: the optimiser writes the parameters through raw pointers, so their torch version does not move), runs the
    model's dense fp16 plan and returns the logit maps with a grad_fn.  The backward of a forward whose plan has since run
    again or was rebuilt is refused.  Refused by name: head_precision='mxfp8', peaks-only plans, graph-replayed plans
    (set ``model.use_graph = False``: a captured graph's kernel nodes and blobs rewritten in place have not been shown to
    coexist), HEADER_NUM_CONV > 2 (the plan's d1 convs ping-pong between two tensors, so h1 is overwritten), a grad_scale that is
    no power of two.  (Peaks-only plans never come here: the forward always takes the model's dense plan.)"""

    def __init__(self, model, grad_scale=DEFAULT_GRAD_SCALE, input_grad=False, want_slices=None):
        import torch
        if model._precision(None) != 'fp16':
            raise NotImplementedError("TrainableHeads: head_precision='mxfp8' has no backward pass (fp16 heads only)")
        if not _is_pow2(grad_scale):
            raise ValueError('TrainableHeads: grad_scale = %r is no power of two' % (grad_scale,))
        if model._num_conv > 2:
            raise NotImplementedError('TrainableHeads: HEADER_NUM_CONV = %d: the plan keeps two head activations (ping-pong), the '
                                      'backward needs all %d' % (model._num_conv, model._num_conv))
        if model._device is None:
            raise RuntimeError('TrainableHeads: call model.to("cuda") first')
        self.model, self.S, self._want_dz, self.want_slices = model, float(grad_scale), bool(input_grad), want_slices
        self.device = model._device
        self.table = head_table(model._head_variant, model._num_classes)
        self.G, self.num_conv = len(self.table), model._num_conv
        self.K = [c for _, _, c in self.table]
        sd = model.state_dict()
        # the parameter arena: conv k (1 .. num_conv) of every branch, then the final convs; weights and biases
        self._names, sizes = [], []
        self._conv_keys = {}                                    # (k, g) -> (conv key, bn key or None); k = num_conv + 1: the final conv
        for g, (seq, last, _) in enumerate(self.table):
            for k in range(1, self.num_conv + 1):
                self._conv_keys[(k, g)] = ('detect_header.%s.%d' % (seq, 3 * (k - 1)), 'detect_header.%s.%d' % (seq, 3 * (k - 1) + 1))
            self._conv_keys[(self.num_conv + 1, g)] = ('detect_header.%s.%s' % (seq, last), None)
        order = [(k, g) for k in range(1, self.num_conv + 2) for g in range(self.G)]
        for kg in order:
            conv, _ = self._conv_keys[kg]
            for leaf in ('weight', 'bias'):
                if conv + '.' + leaf in sd:
                    self._names.append(conv + '.' + leaf)
                    sizes.append(int(sd[conv + '.' + leaf].numel()))
        offs = np.concatenate([[0], np.cumsum([-(-n // 4) * 4 for n in sizes])]).astype(np.int64)      # 16-byte aligned
        self._off = dict(zip(self._names, offs[:-1].tolist()))
        self._arena = torch.zeros(int(offs[-1]), dtype=torch.float32, device=self.device)
        self._params = {}
        for name, n in zip(self._names, sizes):
            v = self._arena[self._off[name]:self._off[name] + n].view(sd[name].shape)
            v.copy_(sd[name])
            self._params[name] = v.requires_grad_()
        # BN rows {s, mean, beta} in fp64 as plan.fold_bn forms them; row 0: no BN
        rows, self._bn_row, self._buffers = [[1.0, 0.0, 0.0]], {}, {}
        scale_of = np.zeros(int(offs[-1]), np.int32)
        self._scale = {}
        for kg in order:
            conv, bn = self._conv_keys[kg]
            if bn is None:
                continue
            for leaf in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'):
                if bn + '.' + leaf in sd:
                    self._buffers[bn + '.' + leaf] = sd[bn + '.' + leaf].to(self.device)
            s = plan_mod._np(sd, bn + '.weight') / np.sqrt(plan_mod._np(sd, bn + '.running_var') + plan_mod.BN_EPS)
            first = len(rows)
            rows += np.stack([s, plan_mod._np(sd, bn + '.running_mean'), plan_mod._np(sd, bn + '.bias')], 1).tolist()
            self._scale[kg] = torch.from_numpy(s.astype(np.float32)).to(self.device)
            cout = len(s)
            w0 = self._off[conv + '.weight']
            per = sizes[self._names.index(conv + '.weight')] // cout
            scale_of[w0:w0 + cout * per] = first + np.repeat(np.arange(cout), per)
            if conv + '.bias' in self._off:
                scale_of[self._off[conv + '.bias']:self._off[conv + '.bias'] + cout] = first + np.arange(cout)
        self._bn = torch.from_numpy(np.asarray(rows, np.float64)).to(self.device)
        self._scale_of = torch.from_numpy(scale_of).to(self.device)
        self._scale_of_host = scale_of
        # the rotated dgrad operands: refreshed by the same launch as the plan's blobs
        self._wr = [None] + [torch.zeros(self.G, 9, 256, 256, dtype=torch.float16, device=self.device) for _ in range(self.num_conv)]
        self._wr_out = torch.zeros(self.G, 9, 256, 16, dtype=torch.float16, device=self.device)
        self._rot_perm = self._upload_rot_perms()
        self._plans = {}                                         # id(plan) -> per-plan state (jobs, HeadBackward, maps)
        self._last = None

    # ---- nn.Module-like surface
    def named_parameters(self):
        return iter(self._params.items())

    def parameters(self):
        return iter(self._params.values())

    def state_dict(self, keep_vars=False):
        from collections import OrderedDict
        out = OrderedDict()
        for k, v in list(self._params.items()) + list(self._buffers.items()):
            out[k] = v if keep_vars else v.detach()
        return out

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def export_to(self, model=None):
        """Write the parameters back through ``model.load_state_dict`` (the model's plans are rebuilt on their next use)."""
        model = self.model if model is None else model
        sd = model.state_dict()
        for k, v in self._params.items():
            sd[k] = v.detach().cpu()
        model.load_state_dict(sd)
        if model is self.model:
            self._plans = {}
        return model

    def nonfinite(self):
        """Non-finite parameter-gradient elements produced so far (reads the device counters: one synchronisation)."""
        return sum(int(st['hb'].nonfinite.item()) for st in self._plans.values())

    # ---- gather tables
    def _wsrc(self, k, g):
        """Arena index of every element of conv (k, g)'s weight, shaped (cout, 256, 3, 3)."""
        name = self._conv_keys[(k, g)][0] + '.weight'
        shape = tuple(self._params[name].shape)
        return self._off[name] + np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)

    def _rot_src(self, k):
        """int32 [G][tap][ci][kc]: the arena index behind every element of the rotated operand of conv k (-1: padding)."""
        kc = 16 if k == self.num_conv + 1 else 256
        out = np.full((self.G, 9, 256, kc), -1, np.int64)
        for g in range(self.G):
            src = self._wsrc(k, g)
            out[g, :, :, :src.shape[0]] = src.reshape(src.shape[0], 256, 9).transpose(2, 1, 0)
        return out.astype(np.int32)

    def _upload_rot_perms(self):
        import torch
        return [torch.from_numpy(self._rot_src(k).reshape(-1)).to(self.device) for k in range(1, self.num_conv + 2)]

    def forward_perms(self, rplan):
        """[(blob id, kind, int32 perm)] of every packed array of the head ops of a realized plan: the perm built by sending the
        arena indices through the packer the recorder used for that blob."""
        jobs = []
        names = {self._op_name(k): k for k in range(1, self.num_conv + 2)}
        for rec in rplan.param_blobs:
            k = names.get(rec['name'])
            if k is None:
                continue
            op = rec['op']
            if k == self.num_conv + 1:                                     # the final convs: plan.pack_headout_weights
                pack = lambda planes: plan_mod.pack_headout_weights(planes, [np.zeros(p.shape[0], np.float32) for p in planes])[0]
                wperm = perm_through(pack, [self._wsrc(k, g) for g in range(self.G)])
                bperm = np.full((self.G, 16), -1, np.int32)
                for g in range(self.G):
                    b = self._off.get(self._conv_keys[(k, g)][0] + '.bias')
                    if b is not None:
                        bperm[g, :self.K[g]] = b + np.arange(self.K[g])
                jobs += [(rec['w_blob'], 0, wperm), (rec['bias_blob'], 1, bperm.reshape(-1))]
                continue
            # op['w']: (groups, taps, cout, cin); conv 1 is ONE group whose cout stacks the branches, the others one group per branch
            groups = op['w'].shape[0]
            per = op['cout'] // 256
            wperm, bperm = [], []
            for gg in range(groups):
                branches = range(per) if groups == 1 else [gg]
                src = np.concatenate([self._wsrc(k, g).reshape(256, 256, 9).transpose(2, 0, 1) for g in branches], 1)      # (taps, cout, cin)
                wperm.append(perm_through(rec['pack'], src))
                bp = np.full(rec['cout_pad'], -1, np.int32)
                for i, g in enumerate(branches):
                    bp[i * 256:(i + 1) * 256] = self._off[self._conv_keys[(k, g)][0] + '.bias'] + np.arange(256)      # (_state refuses a conv without a bias)
                bperm.append(bp)
            jobs += [(rec['w_blob'], 0, np.concatenate(wperm)), (rec['bias_blob'], 1, np.concatenate(bperm))]
        return jobs

    def _op_name(self, k):
        if k == self.num_conv + 1:
            return 'heads.out_convs'
        return 'heads.conv_d6' if k == 1 else ('heads.conv_d1' if k == 2 else 'heads.conv_d1_%d' % (k - 1))

    # ---- per-plan state
    def _state(self, rplan, B, H, W):
        import torch
        st = self._plans.get(id(rplan))
        if st is not None and st['plan'] is rplan:
            return st
        if rplan.graph_stats()[2]:
            raise NotImplementedError('TrainableHeads: the plan for batch %d replays a captured graph; set model.use_graph = False '
                                      '(graph replay and in-place weight refresh have not been shown to coexist)' % B)
        if any(self._conv_keys[(k, g)][0] + '.bias' not in self._off for k in range(1, self.num_conv + 1) for g in range(self.G)):
            raise NotImplementedError('TrainableHeads: a head conv without a bias parameter')
        Hm, Wm = H // 4, W // 4
        named = rplan.plan.named
        acts = []
        for k, nm in enumerate(['z', 'h1', 'h2'][:self.num_conv + 1]):
            s = named[nm]
            if (s.tid, s.coff, s.C) in rplan.lowering['s2d_only'] or s.tid in rplan.lowering.get('widen', {}):
                raise NotImplementedError('TrainableHeads: the plan does not keep %s as a plain tensor' % nm)
            addr, b, h, w, C, P = rplan.tensor_info(s)
            if (b, h, w) != (B, Hm, Wm) or C != (256 if k == 0 else self.G * 256) or P < (6 if k == 0 else 1):
                raise RuntimeError('TrainableHeads: %s is %s with border %d, not the head geometry' % (nm, (b, h, w, C), P))
            acts.append(hb_map(addr, C, P, s.coff, 0 if k == 0 else 256))
        jobs = self.forward_perms(rplan)
        if len(jobs) != 2 * (self.num_conv + 1):
            raise RuntimeError('TrainableHeads: found %d of %d packed head arrays in the plan' % (len(jobs), 2 * (self.num_conv + 1)))
        table, keep = [], []
        for bid, kind, perm in jobs:
            if perm.size * (2 if kind == 0 else 4) != rplan.blob_bytes(bid) or perm.max() >= self._arena.numel():
                raise RuntimeError('TrainableHeads: a gather table does not match its blob (%d elements, %d bytes)' % (perm.size, rplan.blob_bytes(bid)))
            d = torch.from_numpy(perm).to(self.device)
            keep.append(d)
            table.append((rplan.blob_address(bid), d.data_ptr(), perm.size, kind, 0))
        for k in range(1, self.num_conv + 2):
            t = self._wr[k] if k <= self.num_conv else self._wr_out
            table.append((t.data_ptr(), self._rot_perm[k - 1].data_ptr(), t.numel(), 0, 0))
        c_jobs = (_lib.HbRefreshJobC * len(table))(*[_lib.HbRefreshJobC(*j) for j in table])
        _lib.check(_lib.load().rtm3d_head_refresh_check(len(table), c_jobs), 'head_refresh_check')
        d_jobs = torch.frombuffer(bytearray(ctypes.string_at(c_jobs, ctypes.sizeof(c_jobs))), dtype=torch.uint8).to(self.device)
        hb = HeadBackward(B, Hm, Wm, self.K, self.num_conv, self.device, self.S, self._want_dz, self.want_slices)
        st = {'plan': rplan, 'acts': acts, 'jobs': c_jobs, 'd_jobs': d_jobs, 'keep': keep, 'hb': hb, 'shape': (B, H, W)}
        self._plans = {k: v for k, v in self._plans.items() if v['plan'].ctx}          # (closed plans: dropped)
        self._plans[id(rplan)] = st
        return st

    def refresh(self, st=None):
        """Rebuild, on the device and in one launch per plan, every packed array derived from the head parameters: the forward
        blobs of conv_d6 / conv_d1* / out_convs, their fp32 biases, and the rotated dgrad copies."""
        import torch
        for s in ([st] if st is not None else list(self._plans.values())):
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().rtm3d_head_refresh(_lib.stream_ptr(self.device), len(s['jobs']), s['jobs'], s['d_jobs'].data_ptr(),
                                                          self._arena.data_ptr(), self._scale_of.data_ptr(), self._bn.data_ptr()), 'head_refresh')

    # ---- forward / backward
    def __call__(self, x, preloaded=None):
        import torch
        m = self.model
        if preloaded is not None:
            B, H, W = (int(v) for v in preloaded)
        else:
            B, _, H, W = x.shape
        rplan = m._plan_for(B, H, W, self.device, 'dense', 'fp16')
        st = self._state(rplan, B, H, W)
        self.refresh(st)
        names = list(self._params)
        return _head_function().apply(self, st, x, preloaded, *[self._params[n] for n in names])

    def input_grad(self, fp32=False):
        """dz of the last backward: the fp16 NHWC (B, H, W, 256) tensor still scaled by grad_scale (for a device consumer), or with
        ``fp32=True`` a fresh fp32 NCHW tensor, unscaled."""
        if not self._want_dz or self._last is None:
            raise RuntimeError('TrainableHeads.input_grad: construct with input_grad=True and run a backward first')
        dz = self._last['hb'].dz
        return dz.permute(0, 3, 1, 2).float().div_(self.S).contiguous() if fp32 else dz

    def backward_explicit(self, st, dlogits, out=None):
        """The chain for the forward that left ``st``: -> {parameter name: fp32 gradient}.  ``out``: tensors to write into."""
        import torch
        rplan = st['plan']
        if not rplan.ctx or self._plans.get(id(rplan)) is not st:
            raise RuntimeError('TrainableHeads: stale plan - the plan of this forward was rebuilt since (load_state_dict, export_to or eviction)')
        n = self.num_conv
        grads = {}

        def outs(k, leaf):
            res = []
            for g in range(self.G):
                name = self._conv_keys[(k, g)][0] + '.' + leaf
                if name not in self._params:
                    res.append(None)
                    continue
                t = out[name] if out is not None else torch.empty_like(self._params[name].detach())
                grads[name] = t
                res.append(t)
            return res
        dw = [None] + [outs(k, 'weight') for k in range(1, n + 1)]
        db = [None] + [outs(k, 'bias') for k in range(1, n + 1)]
        scales = [None] + [[self._scale[(k, g)] for g in range(self.G)] for k in range(1, n + 1)]
        st['hb'].run(list(dlogits), st['acts'], self._wr, self._wr_out, scales, dw, db, outs(n + 1, 'weight'), outs(n + 1, 'bias'))
        self._last = st
        return grads


_HeadFunction = None


def _head_function():
    """The autograd node of TrainableHeads.__call__ (made on first use: this module imports without torch)."""
    global _HeadFunction
    if _HeadFunction is None:
        import torch
        from torch.autograd.function import once_differentiable

        class _HeadFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, heads, st, x, preloaded, *params):
                logits = heads.model.forward_logits(x, preloaded=preloaded, heads='dense', head_precision='fp16')
                ctx.heads, ctx.st, ctx.stamp = heads, st, st['plan'].z_stamp
                ctx.shapes = [tuple(t.shape) for t in logits]
                return tuple(logits)

            @staticmethod
            @once_differentiable
            def backward(ctx, *grads):
                heads, st = ctx.heads, ctx.st
                if getattr(st['plan'], 'z_stamp', None) != ctx.stamp:
                    raise RuntimeError('TrainableHeads: stale plan - another forward of this shape has overwritten the saved activations')
                dl = [g.contiguous().float() if g is not None else torch.zeros(sh, dtype=torch.float32, device=heads.device)
                      for g, sh in zip(grads, ctx.shapes)]
                got = heads.backward_explicit(st, dl)
                return (None, None, None, None) + tuple(got[n] for n in heads._params)

    return _HeadFunction
