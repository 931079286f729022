"""Engine files: a realized plan written to disk, so that a C or C++ process runs the model without Python.

``save_engine`` has ``plan.PlanRecorder`` - the recording half of ``plan.RealizedPlan`` - issue the plan of ``plan.build_plan``
on a recorder of its own instead of librtm3d_hip.so (no GPU, no library, no context needed) and writes the state-changing C ABI
calls it made - tensor and blob creation, every ``rtm3d_op_*`` launch with its descriptor - plus the packed weight blobs and the
metadata of a detect step.
``rtm3d_engine_load`` (csrc/engine.cpp) replays those calls inside the library; ``rtm3d_engine_detect`` then runs
forward -> decode2d -> decode3d_slots -> pack_records on one stream.  The format is documented in DESIGN.md section 10 and
above the prototypes in include/rtm3d_hip.h; ``read_engine`` is a pure-Python parser of it (inspection and tests).

    rtm3d_amd.engine.save_engine(model, 'dla34_b32.rtm3d', 32, 384, 1280)      # or model.save_engine(...)
    eng = rtm3d_amd.engine.Engine('dla34_b32.rtm3d', 'cuda:0')                  # no plan building, no weight packing
    records = eng.detect(x, K)                                                  # (B, topk, 32) fp32, the pipeline's records
"""
import ctypes
import hashlib
import struct

import numpy as np

from . import _lib

MAGIC = b'RTM3DENG'
FORMAT_VERSION = 1
ARCH = 'gfx950'
HEADER_BYTES = 256
ALIGN = 256
MAX_CLASSES = 16
FUN_ACCEPT = 0.1        # model_utils.FUN_ACCEPT (utils/model_utils.py:298); repeated here so that export needs no torch import

# header: magic, format version, ABI version, arch, state-dict digest (hex), sha256 of the body, body bytes; zero-padded to 256
_HEADER = struct.Struct('<8sII16s64s32sQ')
# metadata of a detect step (the first bytes of the body)
_META = struct.Struct('<3i16s3i4iiffi%dd3diid' % (MAX_CLASSES * 3))
_COUNTS = struct.Struct('<IIQ')          # n_records, n_blobs, records_bytes
_BLOBS = struct.Struct('<QQ')            # blob area offset (from the body start, a multiple of ALIGN), blob area bytes
_REC = struct.Struct('<II')              # opcode, payload bytes
_BLOB_REC = struct.Struct('<QQii')       # bytes, offset in the blob area, id handed out, 0

HEAD_PRECISION_IDS = {'fp16': 0, 'mxfp8': 1}

# the allowlist: C ABI entry -> (opcode, int32 arguments after the context; 'desc' = descriptor struct)
OPCODES = {
    'rtm3d_tensor_create': (1, 6),            # B, H, W, C, pad, id
    'rtm3d_tensor_create_mx8': (2, 6),
    'rtm3d_blob_create': (3, None),           # _BLOB_REC
    'rtm3d_op_input_nhwc4': (16, 1),
    'rtm3d_op_conv': (17, 'desc'),
    'rtm3d_op_stem_fused': (18, 9),
    'rtm3d_op_conv32s2_fused': (19, 10),
    'rtm3d_op_conv64_root': (20, 16),
    'rtm3d_op_headout': (21, 8),              # in, w, bias, nheads, cout4[4]
    'rtm3d_op_maxpool': (22, 8),
    'rtm3d_op_maxpool_s2d': (23, 5),
    'rtm3d_op_softmax_fuse': (24, 6),         # z_in, z_out, n_u, u[3] (unused entries 0)
    'rtm3d_op_quant_mx8': (25, 5),
    'rtm3d_op_conv_mx8': (26, 'desc'),
}
NAMES = {v[0]: k for k, v in OPCODES.items()}
DESCS = {'rtm3d_op_conv': _lib.ConvDesc, 'rtm3d_op_conv_mx8': _lib.ConvMx8Desc}


class EngineInfo(ctypes.Structure):
    """Mirror of struct rtm3d_engine_info (include/rtm3d_hip.h)."""
    _fields_ = [
        ('format_version', ctypes.c_int), ('abi_version', ctypes.c_int),
        ('arch', ctypes.c_char * 16), ('state_digest', ctypes.c_char * 72),
        ('B', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
        ('backbone', ctypes.c_char * 16),
        ('head_precision', ctypes.c_int), ('header_num_conv', ctypes.c_int), ('num_classes', ctypes.c_int),
        ('head_channels', ctypes.c_int * 4),
        ('topk', ctypes.c_int), ('down_sample', ctypes.c_float), ('score_thresh', ctypes.c_float),
        ('n_dim_ref', ctypes.c_int), ('dim_ref', (ctypes.c_double * 3) * MAX_CLASSES), ('ref_loc', ctypes.c_double * 3),
        ('solver_form', ctypes.c_int), ('use_graph', ctypes.c_int), ('fun_accept', ctypes.c_double),
        ('n_records', ctypes.c_int), ('n_tensors', ctypes.c_int), ('n_mx8_tensors', ctypes.c_int), ('n_blobs', ctypes.c_int),
        ('n_launches', ctypes.c_int), ('reserved', ctypes.c_int),
        ('blob_bytes', ctypes.c_uint64), ('file_bytes', ctypes.c_uint64),
    ]


def info_dict(info):
    """An EngineInfo as plain Python values."""
    d = {}
    for name, _ in EngineInfo._fields_:
        v = getattr(info, name)
        if isinstance(v, bytes):
            v = v.decode()
        elif isinstance(v, ctypes.Array):
            v = [list(r) if isinstance(r, ctypes.Array) else r for r in v]
        d[name] = v
    d['dim_ref'] = d['dim_ref'][:d['n_dim_ref']]
    return d


# ---------------------------------------------------------------------------------------------------------- export
class _Recorder(object):
    """The `lib` plan.PlanRecorder issues an exported plan on: keeps the allowlisted calls with their arguments and the blob
    bytes, hands out ids per namespace the way the runtime does (0, 1, 2 ... in creation order), returns 0."""

    def __init__(self):
        self.records = []          # (name, tuple of ints | descriptor bytes | (nbytes, blob index))
        self.blobs = []
        self._next = {}

    def __getattr__(self, name):
        if not name.startswith('rtm3d_'):
            raise AttributeError(name)
        if name == 'rtm3d_op_patch_mask':
            raise NotImplementedError('engine files hold one dense realized plan: the peaks-only regression heads (sparse_heads) '
                                      'are a second plan fed by rtm3d_gather_peak_patches and are not exported')
        if name not in OPCODES:
            raise NotImplementedError('engine export: %s is not a recordable call (allowlist: %s)' % (name, ', '.join(sorted(OPCODES))))

        def call(ctx, *args):
            return self._record(name, args)
        return call

    def _new_id(self, kind, out):
        out._obj.value = self._next.get(kind, 0)
        self._next[kind] = out._obj.value + 1
        return out._obj.value

    def _record(self, name, args):
        if name == 'rtm3d_blob_create':
            ptr, nbytes, out = args
            data = ctypes.string_at(ptr.value if isinstance(ptr, ctypes.c_void_p) else ptr, int(nbytes))
            self.blobs.append(data)
            self.records.append((name, (len(data), len(self.blobs) - 1, self._new_id('blob', out))))
        elif name in ('rtm3d_tensor_create', 'rtm3d_tensor_create_mx8'):
            vals = tuple(int(a) for a in args[:-1])
            self.records.append((name, vals + (self._new_id(name, args[-1]),)))
        elif name in DESCS:
            d = args[0]._obj
            self.records.append((name, bytes(d)))
        elif name == 'rtm3d_op_headout':
            self.records.append((name, tuple(int(a) for a in args[:4]) + tuple(int(c) for c in args[4])))
        elif name == 'rtm3d_op_softmax_fuse':
            us = [int(u) for u in args[3]][:int(args[2])]
            self.records.append((name, tuple(int(a) for a in args[:3]) + tuple(us + [0] * (3 - len(us)))))
        else:
            self.records.append((name, tuple(int(a) for a in args)))
        return 0


def record_plan(ir):
    """(records, blobs) of the plan IR as plan.PlanRecorder issues it: on a _Recorder, with no context (nothing shared is
    touched: neither the library nor its loader)."""
    from . import plan as plan_mod
    rec = _Recorder()
    plan_mod.PlanRecorder(ir, rec, None)
    return rec.records, rec.blobs


def _align(n):
    return -(-n // ALIGN) * ALIGN


def _payload(name, v):
    if name == 'rtm3d_blob_create':
        raise AssertionError('blob records are written by _serialize')
    if name in DESCS:
        return struct.pack('<I', len(v)) + v
    return struct.pack('<%di' % len(v), *v)


def _serialize(meta, digest, records, blobs):
    offsets, pos = [], 0
    for b in blobs:
        offsets.append(pos)
        pos = _align(pos + len(b))
    blob_area = pos
    body = [_META.pack(*meta)]
    recs = []
    for name, v in records:
        if name == 'rtm3d_blob_create':
            nbytes, k, bid = v
            p = _BLOB_REC.pack(nbytes, offsets[k], bid, 0)
        else:
            p = _payload(name, v)
        recs.append(_REC.pack(OPCODES[name][0], len(p)) + p)
    recs = b''.join(recs)
    body.append(_COUNTS.pack(len(records), len(blobs), len(recs)))
    body.append(recs)
    n = sum(len(x) for x in body) + _BLOBS.size
    blob_off = _align(n)
    body.append(_BLOBS.pack(blob_off, blob_area))
    body.append(b'\0' * (blob_off - n))
    for b, o in zip(blobs, offsets):
        body.append(b)
        body.append(b'\0' * (_align(o + len(b)) - o - len(b)))
    body = b''.join(body)
    assert len(body) == blob_off + blob_area
    head = _HEADER.pack(MAGIC, FORMAT_VERSION, _lib.ABI_VERSION, ARCH.encode(), digest.encode(), hashlib.sha256(body).digest(), len(body))
    return head + b'\0' * (HEADER_BYTES - len(head)) + body


def save_engine(model, path, B, H, W, head_precision=None, dim_ref=None, ref_loc=(0.0, -0.5, 20.0), solver_form=None, use_graph=None,
                sparse_heads=False):
    """Write the engine file of ``model`` (its current state dict) for input batches of (B, 3, H, W) to ``path``.
    head_precision: 'fp16' | 'mxfp8' (None: the model's).  dim_ref / ref_loc / solver_form: the 3D decode of the detect step
    (None: cfg.DETECTOR.dim_ref and the default solver form, as Model.detect3d).  use_graph: replay as one hipGraph
    (None: B <= model.GRAPH_MAX_BATCH, the Model's rule).  Needs neither a GPU nor the library.  Returns the metadata dict.
    The peaks-only regression heads (sparse_heads=True) are a second plan fed between two decode kernels: not exported."""
    from . import plan as plan_mod
    from .model import GRAPH_MAX_BATCH
    from .model_utils import solver_form_id
    from .weight_cache import WeightCache, state_dict_digest
    if sparse_heads:
        raise NotImplementedError('engine files hold one dense realized plan; the peaks-only regression heads (sparse_heads) are not exported')
    if model._head_variant not in (None, 'rtm3d'):
        raise NotImplementedError('engine files run the rtm3d head table (forward -> decode2d -> decode3d); head variant %r is not exported'
                                  % model._head_variant)
    prec = model._precision(head_precision)
    B, H, W = int(B), int(H), int(W)
    dim_ref = np.asarray(model.config.DETECTOR.dim_ref if dim_ref is None else dim_ref, np.float64).reshape(-1, 3)
    if len(dim_ref) < model._num_classes:
        raise IndexError('dim_ref has %d rows for %d classes' % (len(dim_ref), model._num_classes))
    if len(dim_ref) > MAX_CLASSES:
        raise ValueError('dim_ref has %d rows; an engine file holds at most %d' % (len(dim_ref), MAX_CLASSES))
    ref_loc = [float(v) for v in np.asarray(ref_loc, np.float64).reshape(3)]
    form = solver_form_id(solver_form)
    use_graph = model.use_graph if use_graph is None else use_graph
    graph = B <= GRAPH_MAX_BATCH if use_graph is None else bool(use_graph)
    if model._wcache is None:
        model._wcache = WeightCache(model._sd)
    ir = plan_mod.build_plan(model._sd, model._backbone_name, B, H, W, model._head_variant, cache=model._wcache,
                             num_classes=model._num_classes, header_num_conv=model._num_conv, head_precision=prec)
    records, blobs = record_plan(ir)
    hc = list(model._head_channels) + [0] * (4 - len(model._head_channels))
    dims = np.zeros((MAX_CLASSES, 3), np.float64)
    dims[:len(dim_ref)] = dim_ref
    meta = (B, H, W, model._backbone_name.encode(), HEAD_PRECISION_IDS[prec], model._num_conv, model._num_classes) + tuple(hc) + \
        (int(model.config.DETECTOR.TOPK_CANDIDATES), float(model.config.MODEL.DOWN_SAMPLE), float(model.config.DETECTOR.SCORE_THRESH),
         len(dim_ref)) + tuple(dims.reshape(-1)) + tuple(ref_loc) + (form, 1 if graph else 0, FUN_ACCEPT)
    data = _serialize(meta, state_dict_digest(model._sd), records, blobs)
    with open(path, 'wb') as f:
        f.write(data)
    return read_engine(path)['meta']


# ---------------------------------------------------------------------------------------------------------- inspection
class EngineFormatError(ValueError):
    pass


def read_engine(path):
    """Parse and check an engine file in Python: {'format_version', 'abi_version', 'arch', 'state_digest', 'meta',
    'records': [(name, values)], 'blobs': [bytes]} - values as written (ints, descriptor bytes; blob records (bytes, index,
    id)).  Raises EngineFormatError on anything the C loader would refuse for its format."""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < HEADER_BYTES:
        raise EngineFormatError('truncated header')
    magic, fv, abi, arch, digest, sha, nbody = _HEADER.unpack_from(data, 0)
    if magic != MAGIC:
        raise EngineFormatError('bad magic')
    if fv != FORMAT_VERSION or abi != _lib.ABI_VERSION:
        raise EngineFormatError('format version %d / ABI %d (this build reads %d / %d)' % (fv, abi, FORMAT_VERSION, _lib.ABI_VERSION))
    body = data[HEADER_BYTES:]
    if len(body) != nbody:
        raise EngineFormatError('body is %d bytes, the header says %d' % (len(body), nbody))
    if hashlib.sha256(body).digest() != sha:
        raise EngineFormatError('sha256 mismatch')
    if len(body) < _META.size + _COUNTS.size:
        raise EngineFormatError('truncated metadata')
    m = _META.unpack_from(body, 0)
    keys = ['B', 'H', 'W', 'backbone', 'head_precision', 'header_num_conv', 'num_classes']
    meta = dict(zip(keys, m[:7]))
    meta['backbone'] = meta['backbone'].rstrip(b'\0').decode()
    meta['head_precision'] = {v: k for k, v in HEAD_PRECISION_IDS.items()}[meta['head_precision']]
    meta['head_channels'] = list(m[7:11])
    meta['topk'], meta['down_sample'], meta['score_thresh'], nd = m[11:15]
    dims = np.asarray(m[15:15 + 3 * MAX_CLASSES]).reshape(MAX_CLASSES, 3)
    meta['dim_ref'] = dims[:nd].tolist()
    r = m[15 + 3 * MAX_CLASSES:]
    meta['ref_loc'], meta['solver_form'], meta['use_graph'], meta['fun_accept'] = list(r[:3]), r[3], r[4], r[5]
    nrec, nblob, rbytes = _COUNTS.unpack_from(body, _META.size)
    pos = _META.size + _COUNTS.size
    if pos + rbytes + _BLOBS.size > len(body):
        raise EngineFormatError('records section past end of file')
    boff, bbytes = _BLOBS.unpack_from(body, pos + rbytes)
    if boff + bbytes != len(body):
        raise EngineFormatError('blob area does not end at the end of the file')
    records, blobs, end = [], [], pos + rbytes
    for i in range(nrec):
        if pos + _REC.size > end:
            raise EngineFormatError('record %d: past the records section' % i)
        op, n = _REC.unpack_from(body, pos)
        pos += _REC.size
        if op not in NAMES or pos + n > end:
            raise EngineFormatError('record %d: unknown opcode %d or payload past the section' % (i, op))
        name, p = NAMES[op], body[pos:pos + n]
        pos += n
        if name == 'rtm3d_blob_create':
            nb, off, bid, _ = _BLOB_REC.unpack(p)
            if off + nb > bbytes:
                raise EngineFormatError('record %d: blob past end of file' % i)
            blobs.append(body[boff + off:boff + off + nb])
            records.append((name, (nb, len(blobs) - 1, bid)))
        elif name in DESCS:
            size, = struct.unpack_from('<I', p)
            if size != ctypes.sizeof(DESCS[name]) or len(p) != 4 + size:
                raise EngineFormatError('record %d: descriptor size %d' % (i, size))
            records.append((name, p[4:]))
        else:
            records.append((name, struct.unpack('<%di' % (len(p) // 4), p)))
    if nblob != len(blobs):
        raise EngineFormatError('%d blob records, the counts say %d' % (len(blobs), nblob))
    return {'format_version': fv, 'abi_version': abi, 'arch': arch.rstrip(b'\0').decode(), 'state_digest': digest.decode(),
            'meta': meta, 'records': records, 'blobs': blobs}


def replay(parsed, lib, ctx=None):
    """Issue the recorded calls of ``read_engine(path)`` against ``lib`` (an object with the rtm3d_* entry points, e.g. the
    ctypes library or a recorder) - the Python statement of what rtm3d_engine_load does; checks the ids handed out."""
    keep = []
    for i, (name, v) in enumerate(parsed['records']):
        fn = getattr(lib, name)
        if name == 'rtm3d_blob_create':
            nb, k, want = v
            buf = ctypes.create_string_buffer(parsed['blobs'][k], nb)
            keep.append(buf)
            out = ctypes.c_int()
            rc = fn(ctx, ctypes.c_void_p(ctypes.addressof(buf)), nb, ctypes.byref(out))
        elif name in ('rtm3d_tensor_create', 'rtm3d_tensor_create_mx8'):
            want, out = v[-1], ctypes.c_int()
            rc = fn(ctx, *v[:-1], ctypes.byref(out))
        elif name in DESCS:
            rc = fn(ctx, ctypes.byref(DESCS[name].from_buffer_copy(v)))
        elif name == 'rtm3d_op_headout':
            rc = fn(ctx, *v[:4], (ctypes.c_int * 4)(*v[4:8]))
        elif name == 'rtm3d_op_softmax_fuse':
            rc = fn(ctx, *v[:3], (ctypes.c_int * v[2])(*v[3:3 + v[2]]))
        else:
            rc = fn(ctx, *v)
        if rc != 0:
            raise RuntimeError('replay: record %d (%s) failed' % (i, name))
        if name in ('rtm3d_blob_create', 'rtm3d_tensor_create', 'rtm3d_tensor_create_mx8') and out.value != want:
            raise RuntimeError('replay: record %d (%s) got id %d, the file says %d' % (i, name, out.value, want))


def inspect_engine(path):
    """rtm3d_engine_inspect through the library: the metadata dict, or RuntimeError with the loader's reason."""
    lib = _lib.load()
    info = EngineInfo()
    _lib.check(lib.rtm3d_engine_inspect(str(path).encode(), ctypes.byref(info)), 'engine_inspect')
    return info_dict(info)


# ---------------------------------------------------------------------------------------------------------- execution
class Engine(object):
    """An engine file loaded by the C loader (rtm3d_engine_load): no plan building, no weight packing in Python.
    use_graph: None = the file's default, True / False overrides it."""

    def __init__(self, path, device='cuda', use_graph=None):
        import torch
        lib = _lib.load()
        d = torch.device(device)
        self.device = torch.device('cuda', d.index if d.index is not None else torch.cuda.current_device())
        info = EngineInfo()
        ctx = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.rtm3d_engine_load(str(path).encode(), self.device.index, ctypes.byref(ctx), ctypes.byref(info)), 'engine_load')
        self.lib, self.ctx = lib, ctx
        self.info = info_dict(info)
        if use_graph is not None:
            self.set_graph(use_graph)
        B, H, W = self.info['B'], self.info['H'], self.info['W']
        self.shapes = [(B, c, H // 4, W // 4) for c in self.info['head_channels'] if c]
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(int(lib.rtm3d_engine_workspace_bytes(ctx)), dtype=torch.uint8, device=self.device)

    def set_graph(self, enable):
        _lib.check(self.lib.rtm3d_ctx_set_graph(self.ctx, 1 if enable else 0), 'ctx_set_graph')

    def _input(self, x):
        import torch
        B, H, W = self.info['B'], self.info['H'], self.info['W']
        if not isinstance(x, torch.Tensor) or tuple(x.shape) != (B, 3, H, W) or not x.is_cuda or x.dtype != torch.float32:
            raise ValueError('this engine runs fp32 CUDA batches of shape %s' % ((B, 3, H, W),))
        return x.contiguous()

    def forward_logits(self, x, out=None):
        """The four fp32 NCHW logit maps of Model.forward_logits (rtm3d_forward of the loaded plan)."""
        import torch
        x = self._input(x)
        with torch.cuda.device(self.device):
            outs = [torch.empty(sh, dtype=torch.float32, device=self.device) for sh in self.shapes] if out is None else list(out)
            ptrs = (ctypes.c_void_p * 4)(*([o.data_ptr() for o in outs] + [0] * (4 - len(outs))))
            _lib.check(self.lib.rtm3d_forward(self.ctx, _lib.stream_ptr(self.device), ctypes.c_void_p(x.data_ptr()), ptrs), 'forward')
        return tuple(outs)

    # ---- what detect and the detect_frames* share: the refusals in front of the step, its outputs, and what follows it
    def _frames_ready(self, who, frames, *maps):
        """Engine.<who> has its workspace and a full batch of frames (and of maps, where it takes them); returns them as lists."""
        B = self.info['B']
        if getattr(self, 'frames_workspace', None) is None:
            raise RuntimeError('Engine.%s: call set_frame_params(mean, std, resize_to) first' % who)
        batches = [list(b) for b in (frames,) + maps]
        if any(len(b) != B for b in batches):
            got = ('%d frames and %d maps' if maps else '%d') % tuple(len(b) for b in batches)
            raise ValueError('this engine runs batches of %d frames, got %s' % (B, got))
        return batches if maps else batches[0]

    @staticmethod
    def _check_draw(who, draw, tracker):
        """Before anything is launched: a TrackDrawParams paints the ids only a tracker hands out."""
        if draw is not None and tracker is None:
            from . import draw as _draw
            if isinstance(draw, _draw.TrackDrawParams):
                raise ValueError('Engine.%s: draw=TrackDrawParams paints track ids and needs tracker=' % who)

    def _intrinsics(self, K):
        import torch
        return torch.as_tensor(K, dtype=torch.float64, device=self.device).reshape(self.info['B'], 9).contiguous()

    def _outputs(self, out, kitti=False):
        """(records, KITTI rows or None) of one step; out: the caller's records."""
        import torch
        B, topk = self.info['B'], self.info['topk']
        rec = torch.empty(B, topk, 32, dtype=torch.float32, device=self.device) if out is None else out
        return rec, torch.empty(B, topk, 16, dtype=torch.float64, device=self.device) if kitti else None

    @staticmethod
    def _after_step(rec, rows, K, paint, draw, tracker, nms3d):
        """Behind a step, in this order: nms3d on the records (and rows), one more frame for the tracker, the drawing into the
        frames ``paint``.  Returns (panels, ids), None where there are none."""
        if nms3d is not None:
            from . import box_overlap
            box_overlap.nms3d_records(rec, kitti_rows=rows, **nms3d)
        ids = None if tracker is None else tracker.update(rec, dt=tracker.dt, ego=tracker.ego)
        panels = None
        if draw is not None:
            from . import draw as _draw
            if isinstance(draw, _draw.TrackDrawParams):
                panels = _draw.draw_tracks(paint, rec, ids, K, draw, tracker=tracker, check_classes=False)
            else:
                panels = _draw.draw_records(paint, rec, K, draw, check_classes=False)
        return panels, ids

    @staticmethod
    def _result(rec, rows, panels, ids, extra=None):
        """(records[, rows][, panels][, ids]): alone, the records themselves; with ``extra`` appended, always a tuple."""
        res = tuple(v for v in (rec, rows, panels, ids) if v is not None)
        if extra is not None:
            return res + extra
        return res if len(res) > 1 else res[0]

    def _frames_step(self, who, front, K, kitti, out, draw, tracker, nms3d, queued=None):
        """The body of every detect_frames*: rtm3d_engine_<who> and what follows it.  front(), called on the engine's device
        once the draw is checked, returns (the entry's own leading arguments, the frames draw= paints, the attributes to
        remember: last_packed, last_rect); queued() is called right behind the library call.  Returns _result's arguments."""
        import torch
        K = self._intrinsics(K)
        with torch.cuda.device(self.device):
            self._check_draw(who, draw, tracker)
            args, paint, remember = front()
            rec, rows = self._outputs(out, kitti)
            _lib.check(getattr(self.lib, 'rtm3d_engine_' + who)(
                self.ctx, _lib.stream_ptr(self.device), *args, ctypes.c_void_p(K.data_ptr()), ctypes.c_void_p(rec.data_ptr()),
                ctypes.c_void_p(rows.data_ptr()) if kitti else None, ctypes.c_void_p(self.frames_workspace.data_ptr())), 'engine_' + who)
            if queued is not None:
                queued()
            for name, frames in remember.items():
                setattr(self, name, frames)
            panels, ids = self._after_step(rec, rows, K, paint, draw, tracker, nms3d)
        return rec, rows, panels, ids

    # (nms3d stays the LAST parameter of detect and detect_frames - tests/test_box_overlap_cpu.py pins it - so tracker, which runs
    # after nms3d, stands before it in the signatures; pass both by keyword)
    def detect(self, x, K_per_image, out=None, tracker=None, nms3d=None):
        """One detect step (rtm3d_engine_detect): (B, topk, 32) fp32 records, the layout of Detect3DPipeline.results.
        K_per_image: (B, 9) intrinsics (fp64 on the device).  nms3d: None | IoU threshold | dict of
        box_overlap.nms3d_records' keywords: 3D NMS of the returned records (one more launch behind the step).
        tracker: None (nothing is launched, the records alone are returned) or a track.Tracker of B streams: the records, after
        nms3d, are one more frame of its streams (tracker.update with tracker.dt / tracker.ego); returns (records, ids)."""
        from . import box_overlap
        nms3d = box_overlap.nms3d_options(nms3d)
        import torch
        x = self._input(x)
        K = self._intrinsics(K_per_image)
        with torch.cuda.device(self.device):
            rec, _ = self._outputs(out)
            _lib.check(self.lib.rtm3d_engine_detect(self.ctx, _lib.stream_ptr(self.device), ctypes.c_void_p(x.data_ptr()),
                                                    ctypes.c_void_p(K.data_ptr()), ctypes.c_void_p(rec.data_ptr()),
                                                    ctypes.c_void_p(self.workspace.data_ptr())), 'engine_detect')
            _, ids = self._after_step(rec, None, K, None, None, tracker, nms3d)
        return self._result(rec, None, None, ids)

    def set_frame_params(self, mean, std, resize_to=None):
        """Once, before detect_frames (rtm3d_engine_set_frame_params): the Normalize mean / std of the frames (cfg.DATASET.MEAN /
        STD) and the longest side after Resize (None: the frames are fed at their own size)."""
        import torch
        p = _lib.FrameParams((ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std]),
                             int(resize_to or 0))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rtm3d_engine_set_frame_params(self.ctx, ctypes.byref(p)), 'engine_set_frame_params')
            self.frames_workspace = torch.empty(int(self.lib.rtm3d_engine_frames_workspace_bytes(self.ctx)), dtype=torch.uint8,
                                                device=self.device)

    def detect_frames(self, images, K_camera, kitti=False, out=None, draw=None, tracker=None, nms3d=None):
        """One detect step fed by camera frames (rtm3d_engine_detect_frames): images = list of B uint8 (h, w, 3) CUDA tensors of
        any sizes that fit the canvas after Resize, K_camera = the cameras' own (B, 9) intrinsics.  Returns the (B, topk, 32)
        records with their 2D fields in the pixels of each frame; kitti=True: (records, (B, topk, 16) float64 KITTI rows).
        nms3d: as for detect; applied to the records and, with kitti=True, to the rows (a suppressed slot's row is zeroed).
        draw: None (nothing is painted, nothing is launched) or a draw.DrawParams: the records, after nms3d, are painted into
        ``images`` in place (draw.draw_records, one more launch behind the step; the frames must be contiguous); with the BEV
        layer set the new (B, bev_h, bev_w, 3) panels are appended to what is returned.  A draw.TrackDrawParams needs ``tracker``
        (ValueError without one) and paints with the ids of this step and the tracker's table (draw.draw_tracks) instead.
        tracker: as for detect; it runs after nms3d and before draw, and the (B, topk) int32 ids are the last element of what is
        returned.  None launches nothing and returns what is returned without it."""
        from . import _frames, box_overlap
        nms3d = box_overlap.nms3d_options(nms3d)
        images = self._frames_ready('detect_frames', images)
        imgs = _frames.packed_frames(images)
        # (draw= paints the caller's tensors, not their contiguous copies: the drawing refuses a frame it could not paint in place)
        front = lambda: ((_lib.ptr_array(imgs), _lib.hw_array(imgs)), images, {})
        return self._result(*self._frames_step('detect_frames', front, K_camera, kitti, out, draw, tracker, nms3d))

    def detect_frames_rig(self, images, K_camera, rig, kitti=False, nms3d=None, tracker=None, out=None):
        """detect_frames on the R * C frames of a rig.Rig (frame r * C + c = camera c of rig r; the engine's batch is R * C), then
        the fusion of the cameras' records into the rig frame (rig.fuse, three more launches).  nms3d: as for detect_frames, per
        camera, before the fusion.  tracker: None or a track.Tracker of R streams: ONE update on the fused records - an object
        keeps its id from one camera's view into the next - then the ids taken back to every camera's record slots
        (rig.camera_ids).  Returns (records[, rows], fused) and, with a tracker, (..., ids_rig (R, cap), ids_cam (R * C, topk)):
        records / rows per camera as detect_frames returns them, fused a rig.Fused.  Nothing synchronises; wrong sizes raise
        before anything is launched."""
        B, topk = self.info['B'], self.info['topk']
        if rig.R * rig.C != B:
            raise ValueError('Engine.detect_frames_rig: the rig holds %d x %d cameras, this engine runs batches of %d' % (rig.R, rig.C, B))
        if rig.device != self.device:
            raise ValueError('Engine.detect_frames_rig: the rig lives on %s, the engine on %s' % (rig.device, self.device))
        cap = rig.check_sizes(topk)
        if tracker is not None and tracker.B != rig.R:
            raise ValueError('Engine.detect_frames_rig: the tracker follows %d streams, the rig has %d (one stream per rig)' % (tracker.B, rig.R))
        res = self.detect_frames(images, K_camera, kitti=kitti, out=out, nms3d=nms3d)
        rec = res[0] if kitti else res
        import torch
        with torch.cuda.device(self.device):
            fused = rig.fuse(rec)
            assert fused.records.shape[1] == cap
            res = (res if kitti else (rec,)) + (fused,)
            if tracker is not None:
                ids_rig = tracker.update(fused.records, dt=tracker.dt, ego=tracker.ego)
                res = res + (ids_rig, rig.camera_ids(ids_rig, fused))
        return res

    def detect_frames_src(self, sources, K_camera, order='rgb', packed=None, kitti=False, out=None, draw=None, tracker=None, nms3d=None):
        """detect_frames fed by decoder / camera surfaces (rtm3d_engine_detect_frames_src): sources = list of B
        pixfmt.FrameSource (NV12, P010, YUYV, I420, pitched RGB / BGRA ... of any sizes that fit the canvas after Resize).  One
        more launch in front of the step converts them into ``packed`` - B contiguous uint8 (h, w, 3) CUDA tensors, allocated
        when None and reachable afterwards as ``engine.last_packed`` - and the step reads those; nothing synchronises.
        order: 'rgb' | 'bgr', the byte order of the packed pixels = the channel order the checkpoint was trained on; the
        library cannot know it (the reference's loader hands the network B G R).
        Every other keyword is detect_frames' and what is returned is what it returns; draw= paints into ``packed``."""
        from . import box_overlap, pixfmt
        nms3d = box_overlap.nms3d_options(nms3d)
        sources = self._frames_ready('detect_frames_src', sources)
        src = pixfmt.c_sources(sources)

        def front():
            dst = pixfmt.packed_buffers(sources, packed)
            return (src, _lib.ptr_array(dst), pixfmt._lookup(pixfmt.ORDERS, order, 'order')), dst, dict(last_packed=dst)
        return self._result(*self._frames_step('detect_frames_src', front, K_camera, kitti, out, draw, tracker, nms3d))

    def detect_frames_raw(self, sources, K_camera, method='mhc', order='rgb', packed=None, kitti=False, out=None, draw=None, tracker=None,
                          nms3d=None):
        """detect_frames fed by raw sensor frames (rtm3d_engine_detect_frames_raw), the twin of detect_frames_src: sources = list
        of B raw.RawSource (Bayer mosaics as bytes, uint16 or MIPI RAW10 / RAW12, of any sizes that fit the canvas after Resize).
        One more launch in front of the step - black level, white balance, demosaic, colour matrix, tone table - writes them
        into ``packed``: B contiguous uint8 (h, w, 3) CUDA tensors, allocated when None and reachable afterwards as
        ``engine.last_packed``; the step reads those and nothing synchronises.
        method: 'mhc' | 'bilinear'.  order: 'rgb' | 'bgr', the byte order of the packed pixels = the channel order the
        checkpoint was trained on.  Every other keyword is detect_frames' and what is returned is what it returns; draw= paints
        into ``packed``.  For a real lens chain the stages yourself: raw.demosaic(sources) gives the packed frames that
        detect_frames_lens(frames, maps) takes."""
        from . import box_overlap, raw
        nms3d = box_overlap.nms3d_options(nms3d)
        sources = self._frames_ready('detect_frames_raw', sources)
        src = raw.c_sources(sources)

        def front():
            dst = raw.packed_buffers(sources, packed)
            return (src, _lib.ptr_array(dst), raw._lookup(raw.METHODS, method, 'method'), raw._lookup(raw.ORDERS, order, 'order')), dst, \
                dict(last_packed=dst)
        return self._result(*self._frames_step('detect_frames_raw', front, K_camera, kitti, out, draw, tracker, nms3d))

    def detect_frames_jpeg(self, datas, K_camera, order='rgb', packed=None, kitti=False, out=None, draw=None, tracker=None, nms3d=None):
        """detect_frames fed by JPEG streams (rtm3d_engine_detect_frames_jpeg), the twin of detect_frames_raw: datas = list of B
        baseline JPEG streams (bytes objects or 1-D uint8 arrays: jpeg.read_files, an MJPEG camera's frames) of any sizes that fit
        the canvas after Resize.  The host entropy-decodes them on a few threads, one copy and one launch in front of the step
        write the frames into ``packed`` - B contiguous uint8 (h, w, 3) CUDA tensors, allocated when None and reachable afterwards
        as ``engine.last_packed`` - and the step reads those; the device is never waited for.
        order: 'rgb' | 'bgr', the byte order of the packed pixels = the channel order the checkpoint was trained on.  Every other
        keyword is detect_frames' and what is returned is what it returns; draw= paints into ``packed``."""
        from . import box_overlap, jpeg
        nms3d = box_overlap.nms3d_options(nms3d)
        datas = self._frames_ready('detect_frames_jpeg', datas)
        arrs, ptrs, sizes = jpeg._streams(datas)
        infos = jpeg.batch_info(arrs, 'engine_detect_frames_jpeg')
        s = None                                 # the staging set of this call

        def front():
            nonlocal s
            dst = jpeg._destinations([(i['h'], i['w']) for i in infos], packed, self.device)
            s, cap = jpeg.staging(self.device, sum(i['coef_count'] for i in infos) * 2)
            nbytes = (ctypes.c_size_t * len(dst))(*[p.numel() for p in dst])
            return (ptrs, sizes, s.host.data_ptr(), s.dev.data_ptr(), cap, _lib.ptr_array(dst), nbytes, jpeg._order(order), 0), dst, \
                dict(last_packed=dst)
        return self._result(*self._frames_step('detect_frames_jpeg', front, K_camera, kitti, out, draw, tracker, nms3d,
                                               queued=lambda: s.mark(self.device)))

    def detect_frames_lens(self, frames_or_sources, maps, order='rgb', fill=(0, 0, 0), K_rect=None, packed=None, rect=None, kitti=False,
                           out=None, draw=None, tracker=None, nms3d=None):
        """detect_frames fed by frames of a real lens (rtm3d_engine_detect_frames_lens): frames_or_sources = list of B raw
        frames, either all uint8 (h, w, 3) CUDA tensors or all pixfmt.FrameSource (converted into ``packed`` first, as by
        detect_frames_src, in ``order``); maps = list of B lens.LensMap (frames may share one).  One more launch resamples the
        raw frames through the maps into ``rect`` - B contiguous uint8 (ho, wo, 3) CUDA tensors, allocated when None - and the
        step reads those with K_rect, the (B, 9) intrinsics of the RECTIFIED cameras (None: each map's own K_rect); nothing
        synchronises.  Records and KITTI rows are in the pixels and the camera of the rectified frames; draw= paints into them.
        fill: the bytes of a pixel without a source.  Every other keyword is detect_frames'.  Returns what detect_frames
        returns, as a tuple, with the list of rectified frames appended: (records[, rows][, panels][, ids], rect)."""
        from . import box_overlap, lens, pixfmt
        nms3d = box_overlap.nms3d_options(nms3d)
        raw, maps = self._frames_ready('detect_frames_lens', frames_or_sources, maps)
        cm = lens.c_maps(maps)
        from_src = all(isinstance(r, pixfmt.FrameSource) for r in raw)
        if not from_src and any(isinstance(r, pixfmt.FrameSource) for r in raw):
            raise ValueError('Engine.detect_frames_lens: either all frames are FrameSource or none is')
        if K_rect is None:
            if any(m.K_rect is None for m in maps):
                raise ValueError('Engine.detect_frames_lens: a map without K_rect needs K_rect=')
            K_rect = np.stack([m.K_rect for m in maps])

        def front():
            if from_src:
                src, hw = pixfmt.c_sources(raw), None
                mid = pixfmt.packed_buffers(raw, packed)
            else:
                src = None
                mid = lens.packed_frames(raw)
                hw = _lib.hw_array(mid)
            dst = lens.rect_buffers(maps, rect)
            return (src, _lib.ptr_array(mid), hw, pixfmt._lookup(pixfmt.ORDERS, order, 'order'), cm, _lib.ptr_array(dst), lens.c_fill(fill)), \
                dst, dict(last_packed=mid, last_rect=dst)
        res = self._frames_step('detect_frames_lens', front, K_rect, kitti, out, draw, tracker, nms3d)
        return self._result(*res, extra=(self.last_rect,))

    def close(self):
        if self.ctx:
            self.lib.rtm3d_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
