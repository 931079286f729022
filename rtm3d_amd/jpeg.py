"""JPEG frames (include/rtm3d_hip.h, "JPEG frames"): baseline JPEG byte streams - what USB / IP cameras deliver as MJPEG and
what recorded driving sets ship as files - become the tightly packed uint8 (h, w, 3) frames that Engine.detect_frames,
lens.remap, preprocess_batch and the drawing entry points read.  The Huffman decoding runs on the host, threaded over the
frames of a batch (rtm3d_jpeg_entropy_decode); dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB run on the
device, one launch per 32 frames (rtm3d_frames_jpeg_idct).  No image library is involved.  The integer rule - libjpeg's default
decode, bit for bit - is written out in the header; tests/jpeg_ref.py restates it in numpy.

JPEG encoding (the header's "JPEG encoding") is the way back: packed frames - painted ones, bird's-eye panels - become baseline
streams byte for byte as libjpeg writes them.  Colour conversion, downsampling, forward DCT and quantisation run on the device
(rtm3d_frames_jpeg_fdct), the Huffman coding on host threads (rtm3d_jpeg_entropy_encode); encode() is the chain, Encoder its
two halves for pipelines; tests/jpeg_enc_ref.py restates the rule in numpy."""
import ctypes

import numpy as np

from . import _frames, _lib
from ._frames import CHUNK  # noqa: F401  (a name the tests use)

MODES = {'grey': 0, '444': 1, '422': 2, '420': 3}
MODE_NAMES = {v: k for k, v in MODES.items()}
ORDERS = {'rgb': 0, 'bgr': 1}
TABLE_WORDS = 192                        # int16 in front of the planes of a coefficient buffer: three tables of 64


def _order(order):
    if isinstance(order, str):
        if order.lower() not in ORDERS:
            raise ValueError("unknown order %r ('rgb' or 'bgr')" % (order,))
        return ORDERS[order.lower()]
    return int(order)                    # a number is passed on: the library refuses what it does not know


def _stream(data):
    """bytes | bytearray | memoryview | 1-D uint8 array -> a contiguous 1-D uint8 numpy array that shares or copies the bytes."""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError('a stream is bytes or a 1-D uint8 array, got %s %s' % (data.dtype, data.shape))
        return np.ascontiguousarray(data)
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    raise ValueError('a stream is bytes or a 1-D uint8 array, got %s' % type(data).__name__)


def _streams(datas):
    arrs = [_stream(d) for d in datas]
    if not arrs:
        raise ValueError('expected a non-empty list of JPEG streams')
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    sizes = (ctypes.c_size_t * len(arrs))(*[a.size for a in arrs])
    return arrs, ptrs, sizes


def info(data):
    """rtm3d_jpeg_info (host only): dict with h, w, components, mode ('grey' '444' '422' '420'), restart_interval, mcus_x, mcus_y,
    bw / bh (the block grid of each component), table_offset / plane_offset (in int16) and coef_count of the stream's coefficient
    buffer.  RuntimeError with the reason for a stream that is refused."""
    a = _stream(data)
    out = _lib.JpegInfo()
    _lib.check(_lib.load().rtm3d_jpeg_info(a.ctypes.data, a.size, ctypes.byref(out)), 'jpeg_info')
    n = out.components
    return dict(h=out.h, w=out.w, components=n, mode=MODE_NAMES[out.mode], restart_interval=out.restart_interval, mcus_x=out.mcus_x,
                mcus_y=out.mcus_y, bw=list(out.bw)[:n], bh=list(out.bh)[:n], table_offset=list(out.table_offset)[:n],
                plane_offset=list(out.plane_offset)[:n], coef_count=out.coef_count)


def batch_info(arrs, who):
    """info of every stream of a batch; a refusal names the frame, as the library's batch entry points do."""
    out = []
    for b, a in enumerate(arrs):
        try:
            out.append(info(a))
        except RuntimeError as e:
            raise RuntimeError('rtm3d_hip %s failed: %s: frame %d: %s' % (who, who, b, str(e).split('jpeg_info: ', 1)[-1]))
    return out


def entropy_decode(data):
    """rtm3d_jpeg_entropy_decode (host only): the stream's coefficient buffer as an int16 numpy array of info(data)['coef_count']."""
    a = _stream(data)
    buf = np.empty(info(a)['coef_count'], np.int16)
    _lib.check(_lib.load().rtm3d_jpeg_entropy_decode(a.ctypes.data, a.size, buf.ctypes.data, buf.size), 'jpeg_entropy_decode')
    return buf


def c_frames(frames):
    """[(int16 CUDA tensor holding a coefficient buffer, h, w, mode)] -> ctypes array of rtm3d_jpeg_frame."""
    arr = (_lib.JpegFrame * len(frames))()
    for i, (coef, h, w, mode) in enumerate(frames):
        arr[i].d_coef = coef if isinstance(coef, int) else coef.data_ptr()
        arr[i].h, arr[i].w, arr[i].reserved = int(h), int(w), 0
        arr[i].mode = MODES[mode] if isinstance(mode, str) else int(mode)
    return arr


def plan(frames):
    """rtm3d_frames_jpeg_plan: the launch schedule of idct(frames), one JpegPlan per chunk of 32 frames (host only; ``frames``:
    what c_frames takes, or its result)."""
    arr = frames if isinstance(frames, ctypes.Array) else c_frames(frames)
    return _frames.chunk_plans('frames_jpeg_plan', _lib.JpegPlan, arr)


def _destinations(sizes, out, dev):
    return _frames.packed_buffers(sizes, [dev] * len(sizes), out, 'stream')


def idct(frames, order='rgb', out=None):
    """rtm3d_frames_jpeg_idct, the device stage alone: frames = [(int16 CUDA tensor holding a coefficient buffer, h, w, mode)] ->
    list of packed uint8 (h, w, 3) CUDA tensors (``out``, or new ones)."""
    import torch
    frames = list(frames)
    dev = frames[0][0].device
    with torch.cuda.device(dev):
        out = _destinations([(f[1], f[2]) for f in frames], out, dev)
        _lib.check(_lib.load().rtm3d_frames_jpeg_idct(_lib.stream_ptr(dev), len(frames), c_frames(frames), _lib.ptr_array(out), _order(order)),
                   'frames_jpeg_idct')
    return out


class _Staging(object):
    """One set of buffers of the chain: pinned host memory for the coefficients, the device buffer they are copied to, and the
    event behind the last call that used them."""

    def __init__(self):
        self.host = self.dev = self.event = None

    def ready(self, nbytes, device):
        import torch
        if self.event is not None:
            self.event.synchronize()                 # the copy and the kernels of the call before last have left these buffers
        if self.host is None or self.host.numel() * 2 < nbytes:
            self.host = torch.empty(max(nbytes // 2, 1), dtype=torch.int16).pin_memory()
        if self.dev is None or self.dev.numel() * 2 < nbytes or self.dev.device != device:
            self.dev = torch.empty(max(nbytes // 2, 1), dtype=torch.int16, device=device)
        return min(self.host.numel(), self.dev.numel()) * 2

    def mark(self, device):
        """Behind the call that uses the buffers: the event ready() waits for."""
        import torch
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(device))


_sets = {}                               # device -> [two _Staging, the index of the next]


def staging(device, nbytes):
    """The staging set of the next call on ``device``, grown to ``nbytes``: (set, capacity in bytes).  Two sets alternate, so the
    host decodes batch n + 1 while the copy of batch n is still under way; a set is reused only after the event recorded behind
    its last call has completed."""
    entry = _sets.setdefault(str(device), [[_Staging(), _Staging()], 0])
    s = entry[0][entry[1]]
    entry[1] ^= 1
    return s, s.ready(nbytes, device)


def workspace_bytes(datas):
    """rtm3d_jpeg_workspace_bytes: the bytes of staging memory (and of device coefficients) the batch needs."""
    _, ptrs, sizes = _streams(datas)
    n = ctypes.c_size_t()
    _lib.check(_lib.load().rtm3d_jpeg_workspace_bytes(len(ptrs), ptrs, sizes, ctypes.byref(n)), 'jpeg_workspace_bytes')
    return n.value


def decode(datas, order='rgb', out=None, threads=0, device=None):
    """rtm3d_frames_jpeg: list of JPEG streams (bytes objects or 1-D uint8 arrays) -> list of packed uint8 (h, w, 3) CUDA tensors
    (``out``, or new ones) on ``device`` (None: the current one).  order: 'rgb' | 'bgr', the byte order of a written pixel - the
    channel order the checkpoint was trained on.  threads: host threads of the entropy decode, 0 = min(B, 8).  The call returns
    when the streams are entropy-decoded and the copies and launches are queued on the current stream; one refused stream
    refuses the batch (RuntimeError naming the frame and the reason) and nothing is launched."""
    import torch
    arrs, ptrs, sizes = _streams(datas)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    infos = batch_info(arrs, 'frames_jpeg')
    with torch.cuda.device(dev):
        out = _destinations([(i['h'], i['w']) for i in infos], out, dev)
        s, cap = staging(dev, sum(i['coef_count'] for i in infos) * 2)
        nbytes = (ctypes.c_size_t * len(out))(*[o.numel() for o in out])
        _lib.check(_lib.load().rtm3d_frames_jpeg(_lib.stream_ptr(dev), len(arrs), ptrs, sizes, s.host.data_ptr(), s.dev.data_ptr(), cap,
                                                 _lib.ptr_array(out), nbytes, _order(order), int(threads)), 'frames_jpeg')
        s.mark(dev)
    return out


def read_files(paths):
    """The bytes of the files, as decode takes them."""
    out = []
    for p in paths:
        with open(p, 'rb') as f:
            out.append(f.read())
    return out


# ---------------------------------------------------------------------------------------------------- encoding
def _mode(mode):
    if isinstance(mode, str):
        if mode.lower() not in MODES:
            raise ValueError("unknown mode %r ('grey', '444', '422' or '420')" % (mode,))
        return MODES[mode.lower()]
    return int(mode)                     # a number is passed on: the library refuses what it does not know


def quality_tables(quality):
    """rtm3d_jpeg_quality_tables (host only): (luma, chroma), two uint16 arrays of 64 in natural order, for quality 1..100."""
    luma, chroma = np.empty(64, np.uint16), np.empty(64, np.uint16)
    _lib.check(_lib.load().rtm3d_jpeg_quality_tables(int(quality), luma.ctypes.data, chroma.ctypes.data), 'jpeg_quality_tables')
    return luma, chroma


def _tables(quality, tables):
    if tables is None:
        return quality_tables(quality)
    luma, chroma = [np.ascontiguousarray(np.asarray(t).reshape(-1)) for t in tables]
    for t in (luma, chroma):
        if t.size != 64 or t.dtype.kind not in 'iu' or t.min() < 0 or t.max() > 65535:
            raise ValueError('a quantisation table is 64 integers in natural order (the library accepts 1..255)')
    return luma.astype(np.uint16), chroma.astype(np.uint16)


def frame_layout(h, w, mode):
    """rtm3d_jpeg_frame_layout (host only): the dict info() gives for a stream of an (h, w, mode) frame."""
    out = _lib.JpegInfo()
    _lib.check(_lib.load().rtm3d_jpeg_frame_layout(int(h), int(w), _mode(mode), ctypes.byref(out)), 'jpeg_frame_layout')
    n = out.components
    return dict(h=out.h, w=out.w, components=n, mode=MODE_NAMES[out.mode], restart_interval=0, mcus_x=out.mcus_x, mcus_y=out.mcus_y,
                bw=list(out.bw)[:n], bh=list(out.bh)[:n], table_offset=list(out.table_offset)[:n], plane_offset=list(out.plane_offset)[:n],
                coef_count=out.coef_count)


def encode_bound(h, w, mode, restart=0):
    """rtm3d_jpeg_encode_bound (host only): an upper bound of the bytes of the stream of an (h, w, mode) frame."""
    n = ctypes.c_size_t()
    _lib.check(_lib.load().rtm3d_jpeg_encode_bound(int(h), int(w), _mode(mode), int(restart), ctypes.byref(n)), 'jpeg_encode_bound')
    return n.value


def entropy_encode(coef, h, w, mode, restart=0):
    """rtm3d_jpeg_entropy_encode (host only): a coefficient buffer (int16 numpy array, its tables included) -> the stream as bytes."""
    coef = np.ascontiguousarray(coef)
    if coef.dtype != np.int16 or coef.ndim != 1 or coef.size < frame_layout(h, w, mode)['coef_count']:
        raise ValueError('a coefficient buffer is an int16 array of at least frame_layout(h, w, mode)["coef_count"]')
    out = np.empty(encode_bound(h, w, mode, restart), np.uint8)
    n = ctypes.c_size_t()
    _lib.check(_lib.load().rtm3d_jpeg_entropy_encode(coef.ctypes.data, int(h), int(w), _mode(mode), int(restart), out.ctypes.data, out.size,
                                                     ctypes.byref(n)), 'jpeg_entropy_encode')
    return out[:n.value].tobytes()


def c_enc_frames(frames):
    """[(uint8 CUDA tensor (h, w, 3) or its address, int16 CUDA tensor for the coefficient buffer or its address, h, w, mode)] ->
    ctypes array of rtm3d_jpeg_enc_frame."""
    arr = (_lib.JpegEncFrame * len(frames))()
    for i, (src, coef, h, w, mode) in enumerate(frames):
        arr[i].d_src = src if isinstance(src, int) else src.data_ptr()
        arr[i].d_coef = coef if isinstance(coef, int) else coef.data_ptr()
        arr[i].h, arr[i].w, arr[i].reserved = int(h), int(w), 0
        arr[i].mode = _mode(mode)
    return arr


def fdct_plan(frames):
    """rtm3d_frames_jpeg_fdct_plan: the launch schedule of fdct, one JpegEncPlan per chunk of 32 frames (host only; ``frames``: what
    c_enc_frames takes, or its result)."""
    arr = frames if isinstance(frames, ctypes.Array) else c_enc_frames(frames)
    return _frames.chunk_plans('frames_jpeg_fdct_plan', _lib.JpegEncPlan, arr)


def _frame_list(frames):
    """A list of contiguous uint8 (h, w, 3) CUDA tensors, or one (B, h, w, 3) tensor -> the list of its frames (views)."""
    import torch
    if isinstance(frames, torch.Tensor):
        if frames.dim() == 3:
            frames = [frames]
        elif frames.dim() == 4:
            frames = [frames[b] for b in range(frames.shape[0])]
    frames = list(frames)
    if not frames:
        raise ValueError('expected a non-empty list of frames')
    if not all(_frames.is_packed_frame(f) for f in frames):
        raise ValueError('a frame is a contiguous uint8 (h, w, 3) CUDA tensor')
    return frames


def fdct(frames, modes='420', quality=90, tables=None, order='rgb'):
    """rtm3d_frames_jpeg_fdct, the device stage alone: frames (what encode takes) -> list of int16 CUDA tensors, one coefficient
    buffer per frame.  modes: one mode, or one per frame."""
    import torch
    frames = _frame_list(frames)
    modes = [modes] * len(frames) if isinstance(modes, (str, int)) else list(modes)
    luma, chroma = _tables(quality, tables)
    dev = frames[0].device
    with torch.cuda.device(dev):
        out = [torch.empty(frame_layout(f.shape[0], f.shape[1], m)['coef_count'], dtype=torch.int16, device=dev) for f, m in zip(frames, modes)]
        arr = c_enc_frames([(f, o, f.shape[0], f.shape[1], m) for f, o, m in zip(frames, out, modes)])
        _lib.check(_lib.load().rtm3d_frames_jpeg_fdct(_lib.stream_ptr(dev), len(frames), arr, luma.ctypes.data, chroma.ctypes.data, _order(order)),
                   'frames_jpeg_fdct')
    return out


_enc_sets = {}                           # device -> [two _Staging, the index of the next]


def _enc_staging(device, nbytes):
    entry = _enc_sets.setdefault(str(device), [[_Staging(), _Staging()], 0])
    s = entry[0][entry[1]]
    entry[1] ^= 1
    return s, s.ready(nbytes, device)


class Encoder(object):
    """The chain in its two halves: submit(frames) queues the device stage and the copies of a batch behind the current stream
    and returns at once (rtm3d_frames_jpeg_encode_queue, then an event); collect() waits on the OLDEST submitted batch's event
    and on nothing else and Huffman-encodes it on the host (rtm3d_frames_jpeg_encode_finish) -> list of bytes.  Two staging sets
    alternate, so one batch may be in flight while the one before it is collected: at most two batches are pending."""

    def __init__(self, quality=90, mode='420', order='rgb', restart=0, tables=None, threads=0):
        self.mode, self.order, self.restart, self.threads = _mode(mode), _order(order), int(restart), int(threads)
        self.luma, self.chroma = _tables(quality, tables)
        self.sets, self.next, self.pending = [_Staging(), _Staging()], 0, []

    def submit(self, frames):
        import torch
        if len(self.pending) >= 2:
            raise RuntimeError('jpeg.Encoder: two batches are pending; collect() one first')
        frames = _frame_list(frames)
        dev = frames[0].device
        hw = _lib.hw_array(frames)
        lib = _lib.load()
        n = ctypes.c_size_t()
        _lib.check(lib.rtm3d_jpeg_encode_workspace_bytes(len(frames), hw, self.mode, ctypes.byref(n)), 'jpeg_encode_workspace_bytes')
        bounds = [encode_bound(f.shape[0], f.shape[1], self.mode, self.restart) for f in frames]     # refuses a bad restart before any launch
        s = self.sets[self.next]
        self.next ^= 1
        with torch.cuda.device(dev):
            cap = s.ready(n.value, dev)
            _lib.check(lib.rtm3d_frames_jpeg_encode_queue(_lib.stream_ptr(dev), len(frames), _lib.ptr_array(frames), hw, self.mode, self.luma.ctypes.data,
                                                          self.chroma.ctypes.data, self.order, s.dev.data_ptr(), s.host.data_ptr(), cap), 'frames_jpeg_encode')
            s.mark(dev)
        self.pending.append((s, len(frames), hw, bounds, frames))          # (the frames stay alive until their kernels have run)

    def collect(self):
        if not self.pending:
            raise RuntimeError('jpeg.Encoder: nothing was submitted')
        s, B, hw, bounds, _ = self.pending.pop(0)
        s.event.synchronize()                                              # the one wait: the result is host bytes
        outs = [np.empty(b, np.uint8) for b in bounds]
        ptrs = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs])
        caps = (ctypes.c_size_t * B)(*bounds)
        lens = (ctypes.c_size_t * B)()
        _lib.check(_lib.load().rtm3d_frames_jpeg_encode_finish(B, hw, self.mode, self.restart, s.host.data_ptr(), ptrs, caps, lens, self.threads),
                   'frames_jpeg_encode')
        return [o[:n].tobytes() for o, n in zip(outs, lens)]


def encode(frames, quality=90, mode='420', order='rgb', restart=0, tables=None, threads=0):
    """rtm3d_frames_jpeg_encode: contiguous uint8 (h, w, 3) CUDA tensors - a list, or one (B, h, w, 3) tensor such as the bird's-eye
    panels - -> list of bytes, one baseline JPEG stream per frame, byte for byte what libjpeg writes for these pixels, tables and
    sampling (Huffman tables not optimised).  quality 1..100 or ``tables`` = (luma, chroma), 64 entries of 1..255 in natural order;
    mode 'grey' | '444' | '422' | '420'; order: the byte order of a pixel in the frames, 'rgb' | 'bgr'; restart: MCUs between
    restart markers, 0 = none; threads: host threads of the Huffman coding, 0 = min(B, 8).  The call waits for its own copies
    (the result is host bytes); one refused frame refuses the batch before anything is launched."""
    import torch
    frames = _frame_list(frames)
    dev = frames[0].device
    mode_, hw, lib = _mode(mode), _lib.hw_array(frames), _lib.load()
    luma, chroma = _tables(quality, tables)
    B = len(frames)
    n = ctypes.c_size_t()
    _lib.check(lib.rtm3d_jpeg_encode_workspace_bytes(B, hw, mode_, ctypes.byref(n)), 'jpeg_encode_workspace_bytes')
    bounds = [encode_bound(f.shape[0], f.shape[1], mode_, restart) for f in frames]
    outs = [np.empty(b, np.uint8) for b in bounds]
    ptrs = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs])
    caps = (ctypes.c_size_t * B)(*bounds)
    lens = (ctypes.c_size_t * B)()
    with torch.cuda.device(dev):
        s, cap = _enc_staging(dev, n.value)
        _lib.check(lib.rtm3d_frames_jpeg_encode(_lib.stream_ptr(dev), B, _lib.ptr_array(frames), hw, mode_, luma.ctypes.data, chroma.ctypes.data,
                                                _order(order), int(restart), s.dev.data_ptr(), s.host.data_ptr(), cap, ptrs, caps, lens, int(threads)),
                   'frames_jpeg_encode')
        s.event = None                                                     # the call has waited for its copies already
    return [o[:k].tobytes() for o, k in zip(outs, lens)]


def write_files(paths, streams):
    """Write every stream to its path."""
    paths, streams = list(paths), list(streams)
    if len(paths) != len(streams):
        raise ValueError('%d paths for %d streams' % (len(paths), len(streams)))
    for p, s in zip(paths, streams):
        with open(p, 'wb') as f:
            f.write(s)
