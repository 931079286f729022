"""GPU (-m gpu): the store layout of the 256 px x 256 ch conv family (conv_mfma256.hip, "Store layout": pixels as the MFMA's A
operand, four consecutive channels per lane, 8-byte stores of whole 128-byte lines, weights read from a row-permuted copy made
at admission) on the smallest shapes at which its addressing can go wrong: one tile and a few, one and two channel tiles, rows
past M, residuals with a channel offset and pitch of their own, channel slices of wider output tensors, the four interleaved
phases of a transposed conv with their softmax partials, the dilated lattice tiles.

Operands, references, poisoned outputs (NaN inside the slice, a sentinel outside it, a zero border) and tolerances are those of
tests/test_gpu_conv256.py: fp16 operands against a float64 conv of the same taps, rtol = atol = 2e-3.  The softmax partials have
no entry point that reads them back, so they are checked through the fusion that consumes them, against torch's softmax of the
stored fp16 values, at the tolerance of test_softmax_fuse_with_epilogue_partials (4e-3)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import rtm3d_amd                                                         # noqa: E402
from rtm3d_amd import plan as plan_mod, _lib, engine, weights           # noqa: E402
from tests.conv_harness import raw_write                                 # noqa: E402
from tests.test_gpu_conv256 import Conv, run_plan, spec, _forward        # noqa: E402

CASES = {
    # ---- generic persistent (1x1, cin 256: four K-tiles) and one-tile (cin 192: three) forms
    'persistent_one_tile_map': spec('persistent', 1, 8, 32, 256, 256, k=1),
    'persistent_b3_nt2_no_relu': spec('persistent', 3, 8, 64, 256, 512, k=1, relu=False),
    'persistent_res_nt2': spec('persistent', 3, 8, 64, 256, 512, k=1, res=True),
    'persistent_m200': spec('persistent', 1, 8, 25, 256, 256, k=1),                       # M = 200: rows 200..255 of the tile are past M
    'persistent_m200_res_no_relu': spec('persistent', 1, 8, 25, 256, 256, k=1, res=True, relu=False),
    'persistent_m1000_w5': spec('persistent', 5, 40, 5, 256, 256, k=1, res=True),         # a lane's four pixels cross rows and images
    'persistent_3x3_res': spec('persistent', 1, 8, 32, 64, 256, res=True),                # (a residual keeps a 3x3 off the halo kernel)
    '1tile_one_tile_map': spec('1tile', 1, 8, 32, 192, 256, k=1),
    '1tile_b3_nt2_res': spec('1tile', 3, 8, 64, 192, 512, k=1, res=True),
    '1tile_m200_no_relu': spec('1tile', 1, 8, 25, 192, 256, k=1, relu=False),
    '1tile_m200_res': spec('1tile', 1, 10, 20, 192, 256, k=1, res=True),
    # ---- output into a channel slice of a wider tensor (512 and 1024 channels per pixel)
    'persistent_slice_of_512': spec('persistent', 1, 8, 25, 256, 256, k=1, out_lo=128, out_hi=128),
    'persistent_slice_of_1024': spec('persistent', 3, 8, 64, 256, 256, k=1, out_lo=256, out_hi=512, out_P=2),
    'halo_slice_of_1024': spec('halo', 1, 8, 32, 64, 512, out_lo=448, out_hi=64),
    'lattice_slice_of_512': spec('lattice', 1, 48, 32, 64, 256, dil=6, out_lo=64, out_hi=192),
    # ---- halo <0, 9>: d1's shape class; halo <., 4>: the four phases of a 4x4 / stride-2 transposed conv
    'halo_groups4_256': spec('halo', 1, 16, 32, 256, 256, groups=4),
    'halo_deconv_8x32': spec('halo', 1, 8, 32, 256, 256, kind='deconv', k=4),
    'halo_deconv_b3_out_border0': spec('halo', 3, 8, 32, 64, 256, kind='deconv', k=4, out_P=0),
    # ---- lattice <6>
    'lattice_cin64': spec('lattice', 1, 48, 32, 64, 256, dil=6),
    'lattice_cin256_no_relu': spec('lattice', 1, 48, 32, 256, 256, dil=6, relu=False),
}


@pytest.mark.parametrize('name', list(CASES))
def test_store_layout_vs_reference(name):
    sp = CASES[name]
    P = plan_mod.Plan(sp['B'], sp['H'] * 4, sp['W'] * 4)
    run_plan(P, [Conv(P, sp, np.random.default_rng(sum(map(ord, name))))])


def test_transposed_conv_phases_and_softmax_partials():
    """Halo <1, 4>: three transposed convs 8x32 -> 16x64 whose epilogues emit the spatial-softmax partials (per channel and
    128-pixel run: max and sum of exp) that the fusion consumes instead of reducing the maps itself.  The maps themselves are
    checked phase by phase (a phase written to another phase's pixels cannot pass), then the fused result, after two forwards
    (the partial buffer is rewritten by every forward).
    What this indirect check cannot see: the fusion combines all chunks of an image, so partials written to the wrong CHUNK of
    their image and channel (a swapped wp, a wrong tile index) cancel; a wrong channel, a wrong image, a wrong max or sum do not."""
    B, H, W = 2, 8, 32
    rng = np.random.default_rng(23)
    P = plan_mod.Plan(B, H * 8, W * 8)
    z0 = P.tensor(2 * H, 2 * W, 256, 0)
    xs = [P.tensor(H, W, 256, 1) for _ in range(3)]
    us = [P.tensor(2 * H, 2 * W, 256, 0) for _ in range(3)]
    ws = [(rng.standard_normal((256, 256, 4, 4)) * sc / 32).astype(np.float32) for sc in (1.0, 2.5, 6.0)]
    for x, u, w in zip(xs, us, ws):
        P.deconv(x, u, w, name='up')
        P.ops[-1]['variant'] = _lib.CONV_MFMA256
    z = P.tensor(2 * H, 2 * W, 256, 6)
    P.softmax_fuse(z0, z, us, name='fuse')
    zin = rng.standard_normal((B, 256, 2 * H, 2 * W)).astype(np.float32)
    xin = [rng.standard_normal((B, 256, H, W)).astype(np.float32) for _ in range(3)]
    R = plan_mod.RealizedPlan(P, 0)
    try:
        assert sorted(R.lowering['stat_slots'].values()) == [0, 1, 2]
        assert [n for n in R.kernel_names() if 'deconv' in n] == ['deconv4x4_phase_mfma256_halo'] * 3, R.kernel_names()
        for s_, arr in [(z0, zin)] + list(zip(xs, xin)):
            _lib.check(R.lib.rtm3d_tensor_upload(R.ctx, R.tids[s_.tid], s_.coff, s_.C, np.ascontiguousarray(arr).ctypes.data_as(ctypes.c_void_p)))
        dummy = torch.zeros(16, device='cuda')
        outs = [torch.zeros(16, device='cuda') for _ in range(4)]
        for _ in range(2):
            R.forward(torch.cuda.current_stream().cuda_stream, dummy.data_ptr(), [o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        got_u = [R.download(u) for u in us]
        got = R.download(z)
    finally:
        R.close()
    half = lambda t: t.half().float()                                   # noqa: E731
    ref = half(torch.from_numpy(zin))
    for x, w, gu in zip(xin, ws, got_u):
        t = half(F.conv_transpose2d(half(torch.from_numpy(x)), half(torch.from_numpy(w)), None, 2, 1))
        tn = t.numpy()
        for py in range(2):
            for px in range(2):                                         # each sub-pixel phase on its own pixels
                np.testing.assert_allclose(gu[:, :, py::2, px::2], tn[:, :, py::2, px::2], rtol=2e-3, atol=2e-3 * max(1.0, float(np.abs(tn).max())))
        ref = ref + t * torch.softmax(t.view(B, 256, -1), -1).view(B, 256, 2 * H, 2 * W)
    ref = half(ref).numpy()
    np.testing.assert_allclose(got, ref, rtol=4e-3, atol=4e-3 * max(1.0, np.abs(ref).max()))


def test_weight_copy_is_per_op_and_deterministic():
    """The row-permuted weight copy is made per op, at admission: the same op built twice in one context, and once more in a
    second context, gives the same bits (one case per kernel of the family).  The engine-file leg is the test below."""
    for name in ('persistent_res_nt2', '1tile_b3_nt2_res', 'halo_groups4_256', 'lattice_cin64'):
        sp = CASES[name]
        images = []
        for ctx in range(2):
            P = plan_mod.Plan(sp['B'], sp['H'] * 4, sp['W'] * 4)
            a = Conv(P, sp, np.random.default_rng(7))
            b = Conv(P, sp, None, shared=a)
            R = plan_mod.RealizedPlan(P, 0)
            try:
                raw_write(R, a.xt, a.x_img)
                if a.rt is not None:
                    raw_write(R, a.rt, a.r_img)
                first, second = _forward(R, [a, b])
            finally:
                R.close()
            a.check(first)
            np.testing.assert_array_equal(first.view(np.uint16), second.view(np.uint16), err_msg=name)
            images.append(first)
        np.testing.assert_array_equal(images[0].view(np.uint16), images[1].view(np.uint16), err_msg=name)


def test_weight_copy_through_an_engine_file(tmp_path):
    """The same ops once more from an engine file: the C loader replays the recorded rtm3d_op_conv calls and makes its own
    permuted copies.  A DLA-34 plan at the smallest batch and map whose lowering puts ops on the generic persistent kernel
    (the folded up3 conv), the halo kernel with four taps and softmax partials (three transposed convs), the halo kernel with
    nine taps (d1) and the lattice kernel (d6): the engine's logits equal the plan's bit for bit.  (No layer of the model
    takes the one-tile form; its weights go through the same admission, before the route is chosen.)"""
    B, H, W = 17, 192, 256
    dev = torch.device('cuda', 0)
    m = rtm3d_amd.create_model(rtm3d_amd.kitti_config('DLA-34')).to(dev).eval()
    m.load_state_dict(weights.synth_state_dict('DLA-34', 5))
    m.use_graph = False
    x = weights.synth_images(B, H, W, seed=9).to(dev)
    want = [t.clone() for t in m.forward_logits(x)]
    names = m._plan_for(B, H, W, dev).kernel_names()
    for k in ('conv3x3_mfma256', 'conv3x3_mfma256_halo', 'conv3x3_mfma256_lattice'):
        assert k in names, (k, names)
    assert names.count('deconv4x4_phase_mfma256_halo') == 3, names
    path = str(tmp_path / 'e.rtm3d')
    m.save_engine(path, B, H, W)
    eng = engine.Engine(path, dev)
    try:
        eng.set_graph(False)
        got = eng.forward_logits(x)
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    finally:
        eng.close()
