"""CPU: the host helpers of the camera-frame entry points (csrc/frames_host.cpp) against the Python statements of the same
bookkeeping in rtm3d_amd/preprocess.py - the normalisation tables bit for bit, the Resize / letterbox geometry of every frame
size up to 160 x 160 - and the refusals of rtm3d_engine_detect_frames that need no device."""
import ctypes
import re

import numpy as np
import pytest

import rtm3d_amd
from rtm3d_amd import _lib, preprocess


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _err(lib):
    return lib.rtm3d_last_error().decode()


def test_normalize_luts_equal_the_python_tables(lib):
    cfg = rtm3d_amd.kitti_config('DLA-34')
    triples = [(cfg.DATASET.MEAN, cfg.DATASET.STD),
               ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
               ((0.0, 0.5, 1.0), (1.0, 1e-6, 3e4))]       # incl. results beyond fp16's range and inside its subnormals
    for mean, std in triples:
        want = preprocess.normalize_lut(mean, std)
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        s = (ctypes.c_float * 3)(*[float(v) for v in std])
        lut32 = np.full((3, 256), np.nan, np.float32)
        lut16 = np.zeros((3, 256), np.uint16)
        assert lib.rtm3d_normalize_luts(m, s, lut32.ctypes.data_as(ctypes.c_void_p), lut16.ctypes.data_as(ctypes.c_void_p)) == 0
        np.testing.assert_array_equal(lut32, want)
        with np.errstate(over='ignore'):
            np.testing.assert_array_equal(lut16, want.astype(np.float16).view(np.uint16))
    # the third triple does reach both ends of the fp16 range
    assert np.abs(want).max() > 65520 and np.abs(want[np.nonzero(want)]).min() < 6.2e-5
    # either table alone
    only16 = np.zeros((3, 256), np.uint16)
    assert lib.rtm3d_normalize_luts(m, s, None, only16.ctypes.data_as(ctypes.c_void_p)) == 0
    np.testing.assert_array_equal(only16, lut16)
    assert lib.rtm3d_normalize_luts(m, s, None, None) != 0 and 'normalize_luts' in _err(lib)


SIDES = np.arange(1, 161)
CANVASES = [(64, 128), (128, 160)]
RESIZES = [0, 96, 128, 160]


def _reference_sizes(resize_to):
    """(160, 160, 2) int: preprocess.resized_size for every (h, w) in 1..160 x 1..160."""
    out = np.empty((160, 160, 2), np.int64)
    for h in SIDES:
        for w in SIDES:
            out[h - 1, w - 1] = preprocess.resized_size(np.int32(h), np.int32(w), resize_to) if resize_to else (h, w)
    return out


@pytest.mark.parametrize('resize_to', RESIZES)
def test_frame_geometry_equals_resized_size_and_the_pad_rule(lib, resize_to):
    ref = _reference_sizes(resize_to)
    hh, ww = np.meshgrid(SIDES, SIDES, indexing='ij')
    for H, W in CANVASES:
        fits = (ref[..., 0] >= 1) & (ref[..., 1] >= 1) & (ref[..., 0] <= H) & (ref[..., 1] <= W)
        assert not fits.all()
        if not fits.any():                               # (Resize to 160 on the 64 x 128 canvas: no frame fits)
            assert (resize_to, H, W) == (160, 64, 128)
        # every frame that fits, in one call
        hw = np.ascontiguousarray(np.stack([hh[fits], ww[fits]], 1), np.int32)
        if len(hw):
            geom = (_lib.FrameGeom * len(hw))()
            assert lib.rtm3d_frame_geometry(len(hw), hw.ctypes.data_as(ctypes.c_void_p), resize_to, H, W, geom) == 0, _err(lib)
            got = np.frombuffer(geom, np.int32).reshape(-1, 6)
            rhw = ref[fits]
            want = np.stack([hw[:, 0], hw[:, 1], rhw[:, 0], rhw[:, 1], (W - rhw[:, 1]) // 2, (H - rhw[:, 0]) // 2], 1)
            np.testing.assert_array_equal(got, want)
            # the Python wrapper hands out the same array
            g2 = preprocess.frame_geometry(hw[:7], (H, W), resize_to or None)
            np.testing.assert_array_equal(np.frombuffer(g2, np.int32).reshape(-1, 6), want[:7])
        # every frame that does not fit is refused by name, wherever it stands in a batch of frames that do
        filler = hw[len(hw) // 2] if len(hw) else None
        batch = np.ones((3, 2), np.int32)
        out3 = (_lib.FrameGeom * 3)()
        p = batch.ctypes.data_as(ctypes.c_void_p)
        for k, (h, w) in enumerate(zip(hh[~fits], ww[~fits])):
            at = k % 3 if filler is not None else 0
            batch[:] = filler if filler is not None else (h, w)
            batch[at] = (h, w)
            assert lib.rtm3d_frame_geometry(3, p, resize_to, H, W, out3) != 0, (h, w)
            assert re.match(r'frame_geometry: frame %d \(' % at, _err(lib)), (h, w, at, _err(lib))
        with pytest.raises(ValueError, match=r'frame 0 '):
            preprocess.frame_geometry([(H + 1, 1), (1, 1)] if not resize_to else [(0, 5), (1, 1)], (H, W), resize_to or None)


def test_frame_geometry_refuses_empty_frames_and_bad_arguments(lib):
    out = (_lib.FrameGeom * 2)()
    for hw, idx in (([4, 4, 0, 4], 1), ([-3, 4, 4, 4], 0), ([4, 4, 4, 0], 1)):
        a = np.array(hw, np.int32)
        for resize_to in (0, 64):
            assert lib.rtm3d_frame_geometry(2, a.ctypes.data_as(ctypes.c_void_p), resize_to, 64, 128, out) != 0
            assert 'frame %d ' % idx in _err(lib)
    a = np.array([4, 4], np.int32)
    assert lib.rtm3d_frame_geometry(0, a.ctypes.data_as(ctypes.c_void_p), 0, 64, 128, out) != 0
    assert lib.rtm3d_frame_geometry(1, None, 0, 64, 128, out) != 0
    assert lib.rtm3d_frame_geometry(1, a.ctypes.data_as(ctypes.c_void_p), -1, 64, 128, out) != 0
    assert lib.rtm3d_frame_geometry(1, a.ctypes.data_as(ctypes.c_void_p), 0, 64, 128, None) != 0


def test_engine_frames_entries_refuse_a_missing_context_without_a_device(lib):
    """No context can be made on a machine without a GPU, so what is reachable here is the null context: every engine entry
    of the frames path names itself and says what is wrong (a live context that is not an engine: tests/test_gpu_frames.py)."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rtm3d_engine_detect_frames(None, None, p, p, p, p, None, p) != 0
    assert _err(lib) == 'engine_detect_frames: the context was not made by rtm3d_engine_load'
    assert lib.rtm3d_engine_detect_frames(None, None, None, None, None, None, None, None) != 0
    assert _err(lib).startswith('engine_detect_frames: ')
    params = _lib.FrameParams((ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(1, 1, 1), 0)
    assert lib.rtm3d_engine_set_frame_params(None, ctypes.byref(params)) != 0
    assert _err(lib) == 'engine_set_frame_params: the context was not made by rtm3d_engine_load'
    assert lib.rtm3d_engine_frames_workspace_bytes(None) == 0


def test_frame_structs_have_the_c_layout(lib, tmp_path):
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s/include/rtm3d_hip.h"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu", '
           'sizeof(rtm3d_frame_geom), offsetof(rtm3d_frame_geom, pad_h), sizeof(rtm3d_frame_params), '
           'offsetof(rtm3d_frame_params, std), offsetof(rtm3d_frame_params, resize_to));return 0;}' % repo)
    c, exe = str(tmp_path / 'l.c'), str(tmp_path / 'l')
    open(c, 'w').write(src)
    subprocess.run(['gcc', '-std=c99', '-Werror', '-o', exe, c], check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(_lib.FrameGeom), _lib.FrameGeom.pad_h.offset, ctypes.sizeof(_lib.FrameParams),
                   _lib.FrameParams.std.offset, _lib.FrameParams.resize_to.offset]
