"""GPU: the uint8 input path (csrc/preprocess.hip) in every regime of tests/preprocess_cases.py, bit for bit against the CPU oracle
(oracle/preprocess_ref.py: resize_bilinear_u8 -> apply_padding -> normalize_to_nchw; the fp16 table is the fp32 one rounded, as
rtm3d_amd.preprocess.device_luts builds it).  rtm3d_preprocess_batch is called through ctypes, so the resized sizes, the border
and the output buffer are the test's own: outputs are pre-filled (NaN / a sentinel bit pattern), so a pixel the kernels skip and a
byte they write outside the interior both show.  That each case runs in the regime it names is tests/test_preprocess_regimes.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import preprocess_ref
from tests import preprocess_cases as pc

pytestmark = pytest.mark.gpu

SUMS_JUNK = 0x5A5A5A5A5A5A            # d_sums before a call: the launcher resets it, a refused call leaves it


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from rtm3d_amd import _lib
    ge.build()
    return _lib.load()


@pytest.fixture(scope='module')
def luts():
    """(device fp32 table, device fp16 table, host fp32 [3][256], host fp16 [3][256] as uint16 bits)"""
    from rtm3d_amd import preprocess
    d32, d16 = preprocess.device_luts(pc.MEAN, pc.STD, torch.device('cuda', 0))
    h32 = preprocess.normalize_lut(pc.MEAN, pc.STD)
    return d32, d16, h32, np.ascontiguousarray(h32.astype(np.float16)).view(np.uint16)


_ORACLE = {}


def oracle(name, call=0):
    """[(uint8 canvas (H, W, 3), integer channel sums)] of a case, computed once and shared by both output modes."""
    key = (name, call)
    if key not in _ORACLE:
        case = pc.CASES[name]
        imgs = pc.make_images(case, call)
        got = pc.oracle_canvases(case, imgs, call)
        for canvas, _ in got:
            canvas.setflags(write=False)
        _ORACLE[key] = (imgs, got)
    return _ORACLE[key]


def upload(case, imgs):
    """The images as views of ONE device buffer at the case's byte offsets: (buffer, [view])."""
    buf, pos = pc.pack(case, imgs)
    d = torch.from_numpy(buf).cuda()
    assert d.data_ptr() % 256 == 0
    views = [d[p:p + im.size].view(im.shape) for im, p in zip(imgs, pos)]
    for v, o in zip(views, pc.offsets(case)):
        assert v.is_contiguous() and v.data_ptr() % 16 == o % 16
    return d, views


def launch(lib, ptrs, hw, rhw, canvas, mode, border, out, sums, luts, B=None, lut16=True):
    B = len(ptrs) if B is None else B
    arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    hw = np.ascontiguousarray(hw, np.int32)
    rhw = None if rhw is None else np.ascontiguousarray(rhw, np.int32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.rtm3d_preprocess_batch(stream, B, arr, hw.ctypes.data_as(ctypes.c_void_p),
                                      None if rhw is None else rhw.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()), mode,
                                      canvas[0], canvas[1], border, luts[0].data_ptr(), luts[1].data_ptr() if lut16 else None,
                                      sums.data_ptr())


def check_fp32(out, canvases, where):
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), '%s: pixels left unwritten' % where
    for b, (canvas, _) in enumerate(canvases):
        want = preprocess_ref.normalize_to_nchw(canvas, pc.MEAN, pc.STD)
        np.testing.assert_array_equal(got[b].view(np.uint32), want.view(np.uint32), err_msg='%s image %d' % (where, b))


def check_nhwc4(out, canvases, P, lut16_bits, where):
    got = out.cpu().numpy().view(np.uint16)                                  # (B, H + 2P, W + 2P, 4)
    H, W = canvases[0][0].shape[:2]
    inner = got[:, P:P + H, P:P + W]
    for b, (canvas, _) in enumerate(canvases):
        for c in range(3):
            np.testing.assert_array_equal(inner[b, :, :, c], lut16_bits[c][canvas[:, :, c]], err_msg='%s image %d channel %d' % (where, b, c))
    assert (inner[..., 3] == 0).all(), '%s: fourth channel is not +0' % where
    ring = np.ones(got.shape[1:3], bool)
    ring[P:P + H, P:P + W] = False
    assert (got[:, ring] == pc.SENTINEL16).all(), '%s: the border ring was written' % where


def check_sums(sums, canvases, where):
    np.testing.assert_array_equal(sums.cpu().numpy(), np.stack([s for _, s in canvases]), err_msg=where)


LIVE = [n for n in pc.CASES if 'refused' not in pc.CASES[n]['expect']]


@pytest.mark.parametrize('mode', ['fp32_nchw', 'fp16_nhwc4'])
@pytest.mark.parametrize('name', LIVE)
def test_case_bit_exact(lib, luts, name, mode):
    case = pc.CASES[name]
    H, W = case['canvas']
    B = len(case['images'])
    P = case['border'] if mode == 'fp16_nhwc4' else 0
    if mode == 'fp32_nchw':
        out = torch.full((B, 3, H, W), float('nan'), dtype=torch.float32, device='cuda')
    else:
        out = torch.full((B, H + 2 * P, W + 2 * P, 4), pc.SENTINEL16, dtype=torch.int16, device='cuda')
    sums = torch.full((B, 3), SUMS_JUNK, dtype=torch.int64, device='cuda')
    for call in range(2 if 'second' in case else 1):           # (replay: the same output and sums, other images)
        imgs, canvases = oracle(name, call)
        shapes = np.array(case['second'] if call else case['images'], np.int32)
        buf, views = upload(case, imgs)
        rc = launch(lib, [v.data_ptr() for v in views], shapes[:, :2], shapes[:, 2:], (H, W), 1 if mode == 'fp16_nhwc4' else 0, P, out,
                    sums, luts)
        assert rc == 0, lib.rtm3d_last_error().decode()
        torch.cuda.synchronize()
        where = '%s %s call %d' % (name, mode, call)
        if mode == 'fp32_nchw':
            check_fp32(out, canvases, where)
        else:
            check_nhwc4(out, canvases, P, luts[3], where)
        check_sums(sums, canvases, where)
        del buf


def test_single_image_kernel_and_the_no_resize_batch(lib, luts):
    """rtm3d_preprocess on 270 400 pixels (channel_sum_kernel's grid stops at 1024 blocks = 262 144 pixels: its grid-stride loop
    runs) and on an image at an odd address, against the oracle; the batched call without resized sizes equals it bit for bit."""
    rng = np.random.Generator(np.random.PCG64(111))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (h, w), (H, W), off in (((520, 520), (523, 524), 0), ((33, 47), (40, 64), 5)):
        assert (h, w) != (520, 520) or h * w > 1024 * 256
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        case = dict(offsets=[off], images=[(h, w, h, w)])
        buf, (view,) = upload(case, [img])
        assert view.data_ptr() % 16 == off
        want, _, _ = preprocess_ref.letterbox_normalize(img, (H, W), pc.MEAN, pc.STD)
        out = torch.full((1, 3, H, W), float('nan'), dtype=torch.float32, device='cuda')
        sums = torch.full((1, 3), SUMS_JUNK, dtype=torch.int64, device='cuda')
        rc = lib.rtm3d_preprocess(stream, view.data_ptr(), h, w, out.data_ptr(), H, W, luts[0].data_ptr(), sums.data_ptr())
        assert rc == 0, lib.rtm3d_last_error().decode()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(sums[0].cpu().numpy(), img.reshape(-1, 3).astype(np.int64).sum(0))
        out2 = torch.full((1, 3, H, W), float('nan'), dtype=torch.float32, device='cuda')
        sums2 = torch.full((1, 3), SUMS_JUNK, dtype=torch.int64, device='cuda')
        assert launch(lib, [view.data_ptr()], [[h, w]], None, (H, W), 0, 0, out2, sums2, luts) == 0, lib.rtm3d_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(sums2, sums)


def _refusals():
    """name -> (keyword overrides of a good two-image call on a 16 x 24 canvas, what the error must name)"""
    good_hw, big = [[8, 10], [5, 7]], [[4, 4]] * 70
    bad70 = [list(s) for s in big]
    bad70[66] = [17, 4]
    return {
        'resized_height_over_canvas': (dict(rhw=[[17, 10], [5, 7]]), 'image 0 (8x10 -> 17x10) does not fit the 16x24 canvas'),
        'resized_width_over_canvas': (dict(rhw=[[8, 10], [5, 25]]), 'image 1 (5x7 -> 5x25) does not fit the 16x24 canvas'),
        'empty_image': (dict(hw=[[8, 10], [0, 7]], rhw=None), 'image 1 (0x7 -> 0x7) does not fit'),
        'null_image_pointer': (dict(null=1), 'image 1 is a null pointer'),
        'empty_batch': (dict(B=0), 'bad arguments'),
        'unknown_out_mode': (dict(mode=2), 'out_mode must be 0 (fp32 NCHW) or 1 (fp16 NHWC4)'),
        'nhwc4_without_fp16_table': (dict(mode=1, lut16=False), 'needs the fp16 table'),
        'negative_border': (dict(mode=1, border=-1), 'border >= 0, not -1'),
        'table_refused': (dict(hw=[[1, 7501]], rhw=None, canvas=(2, 7504)), 'resized width 7501 exceeds'),
        'image_66_of_70_does_not_fit': (dict(hw=bad70, rhw=None), 'image 66 (17x4 -> 17x4) does not fit the 16x24 canvas'),
    }, good_hw


@pytest.mark.parametrize('which', list(_refusals()[0]))
def test_refused_call_launches_nothing(lib, luts, which):
    """Every refusal returns 1, names its cause, and has touched neither the output nor the sums - also when the bad image stands
    behind 64 good ones (the whole batch is validated before the first memset or launch)."""
    (kw, names), good_hw = _refusals()[0][which], _refusals()[1]
    hw = kw.get('hw', good_hw)
    rhw = kw.get('rhw', hw)
    canvas = kw.get('canvas', (16, 24))
    mode, border = kw.get('mode', 0), kw.get('border', 0)
    n = len(hw)
    src = torch.zeros(max(h * w for h, w in hw) * 3 + 16, dtype=torch.uint8, device='cuda')      # every pointer is a readable image
    ptrs = [src.data_ptr()] * n
    if 'null' in kw:
        ptrs[kw['null']] = None
    out = torch.full((n * 3 * (canvas[0] + 2) * (canvas[1] + 2) * 4,), 0xA5, dtype=torch.uint8, device='cuda')
    sums = torch.full((n, 3), SUMS_JUNK, dtype=torch.int64, device='cuda')
    rc = launch(lib, ptrs, hw, rhw, canvas, mode, border, out, sums, luts, B=kw.get('B'), lut16=kw.get('lut16', True))
    err = lib.rtm3d_last_error().decode()
    torch.cuda.synchronize()
    assert rc == 1 and names in err, (rc, err)
    assert bool((out == 0xA5).all()), 'a refused call wrote to the output'
    assert bool((sums == SUMS_JUNK).all()), 'a refused call reset the channel sums'


def test_product_wiring_many_bands_per_workgroup(lib, luts):
    """preprocess.preprocess_batch(..., model=m) at B = 64 with tall thin camera images: the launcher gives every workgroup four
    bands (asserted from the plan entry), and the plan's own input tensor, read back, is the oracle's fp16 canvas."""
    import rtm3d_amd
    from rtm3d_amd import _lib, preprocess, weights
    from tests.conv_harness import D2H, _hip_memcpy
    bb = 'RESNET-18'
    cfg = rtm3d_amd.kitti_config(bb)
    m = rtm3d_amd.create_model(cfg).to('cuda:0').eval()
    m.load_state_dict(weights.synth_state_dict(bb, 1, 'trained', heat_bias=-3.5))
    H, W, B = 128, 256, 64
    rng = np.random.Generator(np.random.PCG64(112))
    kinds = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in ((5120, 160), (4096, 100), (2560, 200), (1280, 90))]
    dev = [torch.from_numpy(k).cuda() for k in kinds]
    _, pads, rhw = preprocess.preprocess_batch([dev[i % 4] for i in range(B)], (H, W), pc.MEAN, pc.STD, resize_to=128, model=m)
    base, P = m.input_tensor(B, H, W)
    torch.cuda.synchronize()
    # the schedule this call had
    hw = np.array([kinds[i % 4].shape[:2] for i in range(B)], np.int32)
    r = np.array(rhw, np.int32)
    plan = (_lib.PreprocessPlan * 1)()
    assert lib.rtm3d_preprocess_batch_plan(B, hw.ctypes.data_as(ctypes.c_void_p), r.ctypes.data_as(ctypes.c_void_p), H, W, plan) == 0
    assert plan[0].count == 64 and plan[0].bands > plan[0].grid_x and plan[0].bands == 128 and plan[0].grid_x == 32
    got = np.empty((B, H + 2 * P, W + 2 * P, 4), np.uint16)
    _hip_memcpy(lib, got.ctypes.data, base, got.nbytes, D2H)
    inner = got[:, P:P + H, P:P + W]
    for k in range(4):
        small = preprocess_ref.resize_bilinear_u8(kinds[k], rhw[k])
        canvas, pw, ph = preprocess_ref.apply_padding(small, (W, H))
        want = np.stack([luts[3][c][canvas[:, :, c]] for c in range(3)], 2)
        for b in range(k, B, 4):
            assert pads[b] == (pw, ph)
            np.testing.assert_array_equal(inner[b, :, :, :3], want, err_msg='image %d' % b)
    assert (inner[..., 3] == 0).all()
