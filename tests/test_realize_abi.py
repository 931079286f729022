"""CPU: the exact stream of C ABI calls ``plan.PlanRecorder`` makes for a fixed set of plans - tensors, packed weight blobs,
every launch with its descriptor - recorded through tests/abi_recorder.py instead of librtm3d_hip.so and compared with
digests recorded when the test was written: a change of the host-side lowering that means to keep the launches must keep
these digests.  The set covers every realize-level rewrite and
kernel choice: stem fusion, level entry and tail, project folds, neck up-folds, space-to-depth-only maps, the halo kernels,
the softmax-partials producers, MXFP8 heads, the peaks-only patch plan, and each A/B switch flipped."""
import numpy as np
import pytest

from rtm3d_amd import _lib, plan as plan_mod, weights
from tests.abi_recorder import pin_switches, record

_SD = {}


def _sd(bb):
    if bb not in _SD:
        _SD[bb] = weights.synth_state_dict(bb, 3, 'trained')
    return _SD[bb]


def _dense(bb, B, H, W, **kw):
    return lambda: plan_mod.build_plan(_sd(bb), bb, B, H, W, **kw)


def _softmax_partials_plan():
    """The hand-built plan of test_gpu_kernels.py::test_softmax_fuse_with_epilogue_partials."""
    B, H, W = 3, 8, 32
    rng = np.random.default_rng(11)
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
    return P


# case: (plan builder, switches other than abi_recorder.DEFAULTS, (calls, launches), sha256 of the call log)
CASES = {
    'dla34_b32_384x1280': (_dense('DLA-34', 32, 384, 1280), {}, (182, 47),
        'e8dcb993a5cd13d574f1c73a294ccfc0731b0c5d3fde3c087c7e32136233c469'),
    'dla34_b32_384x1280_mxfp8': (_dense('DLA-34', 32, 384, 1280, head_precision='mxfp8'), {}, (186, 48),
        'd10c509f6e9a873c40a8af406fc218cacc5d8831c0c863278574af0bea84b663'),
    'dla34_b32_416x1280': (_dense('DLA-34', 32, 416, 1280), {}, (182, 47),
        'ee5b0b40abc89a67422ab37704e7eb1b6f5f352fd9e752d432ce0ecb119df242'),
    'dla34_b2_64x128': (_dense('DLA-34', 2, 64, 128), {}, (191, 50),
        '07a39fbf619a7214ac06bf8c5bfbe9d162091706eeac92b35ff52ddfb575d028'),
    'dla34_b32_dense_heads1': (_dense('DLA-34', 32, 384, 1280, dense_heads=1), {}, (182, 47),
        '2f781a8a6abe2f000261a88a99ccfa89c46460d41750ffa3f7c42c9d307b2cb9'),
    'peak_plan_3200': (lambda: plan_mod.build_peak_plan(_sd('DLA-34'), 3200, (96, 320)), {}, (18, 6),
        'ca3a8cd79a23efe33687d8592cc8844100803eac717f98a4e53ce30c525f6b33'),
    'resnet18_b8_384x1280': (_dense('RESNET-18', 8, 384, 1280), {}, (140, 37),
        '29ce5ba61c81045150b221b6be56bf0e6e918766b233b9db423173cc7e53a204'),
    'resnet34_b8_384x1280': (_dense('RESNET-34', 8, 384, 1280), {}, (204, 53),
        'd2afc96b70eb1aff31e495315c4da39467af47cb355b0d4a84c881b51438e896'),
    'dla34_b32_fuse_stem2': (_dense('DLA-34', 32, 384, 1280), {'FUSE_STEM': 2}, (183, 48),
        '872b1a90df29835bbea613ba5928d840862e702014261324fc2ccbf4f0742751'),
    'dla34_b32_fuse_stem_off': (_dense('DLA-34', 32, 384, 1280), {'FUSE_STEM': False}, (184, 49),
        '04e9eef053e18b9067b3bfa1f01b1b5be4b6c2e964093c0db94779d25b6e465b'),
    'dla34_b32_level_entry_off': (_dense('DLA-34', 32, 384, 1280), {'FUSE_LEVEL_ENTRY': False}, (184, 49),
        'aecf8a7607577b5585cc48a877b23b4e7b242d2f37771f62fc99ce68e8937d87'),
    'dla34_b32_level_tail_off': (_dense('DLA-34', 32, 384, 1280), {'FUSE_LEVEL_TAIL': False}, (184, 49),
        '9367662284be8dba9b865cb40677821b28e9d7287129c85d2799d3c3488083c8'),
    'dla34_b32_fold_project_off': (_dense('DLA-34', 32, 384, 1280), {'FOLD_PROJECT': False}, (191, 50),
        'b962609e883f3bdfaa2dee6164653422179a0ef6f0ab866a0d24157dce7934e9'),
    'dla34_b32_fold_c128_off': (_dense('DLA-34', 32, 384, 1280), {'FOLD_PROJECT_C128': False}, (185, 48),
        '491d57ef17db754e9d86b5ee3b7f66482a60e78af8e9e980927eb77ec2d4620e'),
    'dla34_b32_fold_neck_up_off': (_dense('DLA-34', 32, 384, 1280), {'FOLD_NECK_UP': False}, (191, 50),
        '8e8d01dcb3ef9f30aab0480471b3c47765014d24b1681551e78dd99be078c44b'),
    'dla34_b32_s2d_only_off': (_dense('DLA-34', 32, 384, 1280), {'S2D_ONLY': False}, (182, 47),
        '211f72a0e7f4c1bb7acdf3af2120c66ff60eebe8b10e410adbf10c12e96c02d5'),
    'dla34_b32_conv128_off': (_dense('DLA-34', 32, 384, 1280), {'USE_CONV128': False}, (182, 47),
        '575ffaa740c9488d9db8c74feed8270778467417a888357405b26aa774aa0ac2'),
    'dla34_b32_conv64s2_off': (_dense('DLA-34', 32, 384, 1280), {'USE_CONV64S2': False}, (182, 47),
        'f6dc541aec6900703a1f43a32f6a49c96587332fabccee300ea6ff7f1f0c6e8f'),
    'dla34_b2_v2_min_tiles8': (_dense('DLA-34', 2, 384, 1280), {'V2_MIN_TILES': 8}, (182, 47),
        '2fb4689d11279700a8e71853e0d5eae8a2af8598f98ef66170de1aafc46b7bcb'),
    'softmax_epilogue_partials': (_softmax_partials_plan, {}, (18, 4),
        '08561886fd2a308175eb8b598041e5211b9f53879bffb3d5d38b269af3d59c0c'),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_realized_call_stream_is_pinned(case, monkeypatch):
    build, switches, counts, want = CASES[case]
    pin_switches(monkeypatch, **switches)
    rec = record(build())
    got = (len(rec.calls), len(rec.launches())), rec.digest()
    assert len(rec.recorded.op_names) == len(rec.launches())
    assert got == (counts, want), got
