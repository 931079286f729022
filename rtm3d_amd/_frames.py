"""What the wrappers of the frame stages (pixfmt, raw, jpeg, lens, augment) and the callers of packed frames (engine, draw,
preprocess) share: the chunk size, names -> numbers, lists -> ctypes arrays, the chunked ``*_plan`` call, the check of a packed
uint8 (h, w, 3) frame and the two checks of a pitched plane.  The host side of the same stages shares csrc/frame_chunks.h."""
from . import _lib

CHUNK = 32                               # frames per launch (csrc/frame_chunks.h: FRAME_CHUNK)


def lookup(table, v, what, aliases=None):
    """A name of ``table`` (or of ``aliases``) in any letter case -> its number; ValueError for another name."""
    if isinstance(v, str):
        name = v.lower()
        name = (aliases or {}).get(name, name)
        if name not in table:
            raise ValueError('unknown %s %r (one of %s)' % (what, v, ', '.join(sorted(table))))
        return table[name]
    return int(v)                        # a number is passed on: the library refuses what it does not know


def struct_array(ctype, items, cls):
    """list of ``cls`` -> ctypes array of ``ctype``, one ``c_struct()`` each."""
    items = list(items)
    if not items or not all(isinstance(i, cls) for i in items):
        raise ValueError('expected a non-empty list of %s' % cls.__name__)
    arr = (ctype * len(items))()
    for i, s in enumerate(items):
        arr[i] = s.c_struct()
    return arr


def chunk_plans(entry, plan_type, arr, *args):
    """rtm3d_<entry>(len(arr), arr, *args, out): the launch schedule of a batch, one ``plan_type`` per chunk of CHUNK frames."""
    out = (plan_type * ((len(arr) + CHUNK - 1) // CHUNK))()
    _lib.check(getattr(_lib.load(), 'rtm3d_' + entry)(len(arr), arr, *(args + (out,))), entry)
    return list(out)


def is_packed_frame(t, hw=None, contiguous=True, device=None):
    """``t`` is a uint8 (h, w, 3) CUDA tensor - of (h, w) = ``hw``, contiguous, on ``device`` where these are asked for."""
    import torch
    return isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_cuda and t.dim() == 3 and t.shape[2] == 3 \
        and (hw is None or tuple(t.shape[:2]) == tuple(hw)) and (not contiguous or t.is_contiguous()) and (device is None or t.device == device)


def packed_frames(frames, what='expected uint8 (h, w, 3) CUDA frames', device=None):
    """The frames a stage reads: checked (uint8 (h, w, 3) CUDA, ValueError(``what``) otherwise), made contiguous."""
    frames = list(frames)
    if not all(is_packed_frame(f, contiguous=False, device=device) for f in frames):
        raise ValueError(what)
    return [f.contiguous() for f in frames]


def packed_buffers(sizes, devices, out, owner, dims='(h, w, 3)'):
    """The destination frames of a stage: new uint8 (h, w, 3) tensors of ``sizes`` on ``devices``, or ``out`` checked against
    the sizes.  owner: what a destination belongs to in the messages ('source', 'map', 'stream')."""
    import torch
    if out is None:
        return [torch.empty(h, w, 3, dtype=torch.uint8, device=d) for (h, w), d in zip(sizes, devices)]
    out = list(out)
    if len(out) != len(sizes):
        raise ValueError('%d destinations for %d %ss' % (len(out), len(sizes), owner))
    for (h, w), o in zip(sizes, out):
        if not is_packed_frame(o, (h, w)):
            raise ValueError('a destination is a contiguous uint8 CUDA tensor of its %s\'s %s = %s' % (owner, dims, (h, w, 3)))
    return out


def plane_row_bytes(t):
    """Bytes of a row of a 2- or 3-D plane tensor."""
    return int(t.shape[1] * (t.shape[2] if t.dim() == 3 else 1)) * t.element_size()


def plane_pitch(t, what):
    """The pitch a plane tensor gives by itself: ``stride(0)`` in bytes; None for a 1-D tensor, a raw buffer.  ValueError unless
    the bytes of a row are contiguous."""
    if t.dim() == 1:
        return None
    inner = list(zip(t.shape[1:], t.stride()[1:]))
    if inner[-1][1] != 1 or (len(inner) == 2 and inner[0][1] != inner[1][0]):
        raise ValueError('%s: the bytes of a row must be contiguous (strides %s)' % (what, tuple(t.stride())))
    return int(t.stride(0)) * t.element_size() if t.shape[0] > 1 else plane_row_bytes(t)


def check_plane_covers(t, pitch, row, rows, what, owner):
    """What the tensor holds must cover what the kernel reads: ``rows`` x ``row`` bytes at ``pitch`` (the library cannot see
    sizes).  owner: 'format' | 'layout', whose need the message states."""
    if t.dim() == 1:
        have, need = t.numel() * t.element_size(), (rows - 1) * pitch + row
        if pitch >= row and have < need:
            raise ValueError('%s holds %d bytes, %d rows of %d at pitch %d need %d' % (what, have, rows, row, pitch, need))
    elif t.shape[0] < rows or plane_row_bytes(t) < row:
        raise ValueError('%s is %d rows of %d bytes, the %s needs %d rows of %d' % (what, t.shape[0], plane_row_bytes(t), owner, rows, row))
