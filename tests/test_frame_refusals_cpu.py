"""The refusals and the chunking that the six frame stages share (csrc/frame_chunks.h), pinned through every stage's host-only
``_plan`` and ``_check`` entry: the texts below were recorded from the library before the stages shared that header, so a stage
that words a shared refusal by hand again, or cuts its chunks differently, fails here.  No GPU: nothing is launched and the
fake addresses are never read."""
import ctypes
from ctypes import c_int, c_void_p

import pytest

from rtm3d_amd import _lib

P = 0x10000                              # stands for a device address (aligned for every stage)
Q = (ctypes.c_uint16 * 64)(*[16] * 64)  # a quantisation table


def _fill(s, **fields):
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _raw():
    s = _fill(_lib.RawSrc(), plane=P, pitch=8, h=6, w=8, layout=0, bits=8, pattern=0)
    s.gain[:], s.ccm[:] = [1024] * 4, [1024, 0, 0, 0, 1024, 0, 0, 0, 1024]
    return s


def _src():
    s = _fill(_lib.FrameSrc(), h=6, w=8, format=0)
    s.plane[0], s.pitch[0] = P, 24
    return s


# stage -> (frame struct, plan struct, a valid frame, the two side fields, plan(lib, B, arr, out), check(lib, B, arr, dst, order))
STAGES = {
    'convert': (_lib.FrameSrc, _lib.ConvertPlan, _src, 'hw', lambda L, B, a, o: L.rtm3d_frames_convert_plan(B, a, o),
                lambda L, B, a, d, r: L.rtm3d_frames_convert_check(B, a, d, r)),
    'demosaic': (_lib.RawSrc, _lib.DemosaicPlan, _raw, 'hw', lambda L, B, a, o: L.rtm3d_frames_demosaic_plan(B, a, 0, o),
                 lambda L, B, a, d, r: L.rtm3d_frames_demosaic_check(B, a, d, 0, r)),
    'jpeg': (_lib.JpegFrame, _lib.JpegPlan, lambda: _lib.JpegFrame(P, 6, 8, 1, 0), 'hw', lambda L, B, a, o: L.rtm3d_frames_jpeg_plan(B, a, o),
             lambda L, B, a, d, r: L.rtm3d_frames_jpeg_check(B, a, d, r)),
    'jpeg_enc': (_lib.JpegEncFrame, _lib.JpegEncPlan, lambda: _lib.JpegEncFrame(P, P, 6, 8, 1, 0), 'hw',
                 lambda L, B, a, o: L.rtm3d_frames_jpeg_fdct_plan(B, a, o), lambda L, B, a, d, r: L.rtm3d_frames_jpeg_fdct_check(B, a, Q, Q, r)),
    'lens': (_lib.LensMapC, _lib.RemapPlan, lambda: _lib.LensMapC(P, 6, 8, 0), ('ho', 'wo'), lambda L, B, a, o: L.rtm3d_frames_remap_plan(B, a, o),
             lambda L, B, a, d, r: L.rtm3d_frames_remap_check(B, (c_void_p * 2)(2 * P, 2 * P), (c_int * 4)(6, 8, 6, 8), a, d, (ctypes.c_uint8 * 3)())),
    'augment': (_lib.AugmentFrameC, _lib.AugmentPlan, lambda: _fill(_lib.AugmentFrameC(), h=6, w=8, rw=8, rh=6, alpha_q=65536), 'hw',
                lambda L, B, a, o: L.rtm3d_frames_augment_plan(B, a, 2, 6, 8, 0, o),
                lambda L, B, a, d, r: L.rtm3d_frames_augment_check(B, (c_void_p * 2)(2 * P, 2 * P), a, d[1], 2, 6, 8, 0, P, None, None, P)),
}
CONDITIONS = ('B = 0', 'null array', 'order 2', 'side 0', 'side 16385', 'reserved 1', 'NULL destination of frame 1')


def refusal(stage, entry, cond):
    """The last-error text of the stage's ``entry`` ('plan' | 'check') for a batch of two frames under ``cond``; None: accepted."""
    frame, plan_t, good, sides, plan, check = STAGES[stage]
    lib = _lib.load()
    B, order, arr, dst = 2, 0, (frame * 2)(good(), good()), (c_void_p * 2)(P, P)
    if cond == 'B = 0':
        B = 0
    elif cond == 'null array':
        arr = None
    elif cond == 'order 2':
        order = 2
    elif cond == 'side 0':
        setattr(arr[1], sides[0], 0)
    elif cond == 'side 16385':
        setattr(arr[1], sides[1], 16385)
    elif cond == 'reserved 1':
        arr[1].reserved = 1
    else:
        dst[1] = None
    rc = plan(lib, B, arr, (plan_t * 1)()) if entry == 'plan' else check(lib, B, arr, dst, order)
    return lib.rtm3d_last_error().decode() if rc else None


# condition -> text, in the words of the stage: who (the plan's, the check's), the name of its order argument (None: it takes none),
# the least side, how it words a bad side, how a missing destination (None: it has none)
TEXTS = {'B = 0': '{who}: B = 0', 'null array': '{who}: null pointer', 'order 2': '{who}: {order} 2 (0 R G B, 1 B G R)',
         'side 0': '{who}: frame 1{side} 0 x 8; a side must lie in {lo}..16384',
         'side 16385': '{who}: frame 1{side} 6 x 16385; a side must lie in {lo}..16384', 'reserved 1': '{who}: frame 1: reserved = 1, not 0',
         'NULL destination of frame 1': '{who}: {dst}the destination is a NULL pointer'}
WORDS = {'convert': (('frames_convert_plan', 'frames_convert'), 'dst_order', 1, ' is', 'frame 1: '),
         'demosaic': (('frames_demosaic_plan', 'frames_demosaic'), 'dst_order', 2, ' is', 'frame 1: '),
         'jpeg': (('frames_jpeg_plan', 'frames_jpeg_idct'), 'dst_order', 1, ' is', 'frame 1: '),
         'jpeg_enc': (('frames_jpeg_fdct_plan', 'frames_jpeg_fdct'), 'src_order', 1, ' is', None),
         'lens': (('frames_remap_plan', 'frames_remap'), None, 1, ': a map of', 'frame 1: '),
         'augment': (('frames_augment_plan', 'frames_augment'), None, 1, ' is', '')}      # (one destination for the batch)


def expected(stage, entry, cond):
    who, order, lo, side, dst = WORDS[stage]
    accepted = (cond == 'order 2' and (entry == 'plan' or order is None)) or (cond.startswith('NULL') and (entry == 'plan' or dst is None))
    return None if accepted else TEXTS[cond].format(who=who[entry == 'check'], order=order, lo=lo, side=side, dst=dst)


@pytest.mark.parametrize('stage', sorted(STAGES))
@pytest.mark.parametrize('entry', ['plan', 'check'])
def test_shared_refusals_keep_their_text(stage, entry):
    for cond in CONDITIONS:
        assert refusal(stage, entry, cond) == expected(stage, entry, cond), (stage, entry, cond)


@pytest.mark.parametrize('stage', sorted(STAGES))
def test_chunks_of_a_plan(stage):
    frame, plan_t, good, _, plan, _ = STAGES[stage]
    want = {31: [(0, 31)], 32: [(0, 32)], 33: [(0, 32), (32, 1)], 65: [(0, 32), (32, 32), (64, 1)]}
    for B, chunks in want.items():
        out = (plan_t * 3)()
        assert plan(_lib.load(), B, (frame * B)(*[good() for _ in range(B)]), out) == 0, _lib.load().rtm3d_last_error()
        assert [(p.first, p.count) for p in out[:len(chunks)]] == chunks and all(p.count == 0 for p in out[len(chunks):]), B
