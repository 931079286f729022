"""GPU: rtm3d_rig_fuse / rtm3d_rig_scatter_ids (csrc/rig.hip: rig_prepare_kernel, rig_link_kernel, rig_cluster_kernel) against the
numpy yardstick tests/rig_ref.py over the constructed cases of tests/rig_regimes.py - every regime of the three kernels that the
rendered scenes of tests/rig_cases.py leave out: the bitonic sort at every padded size M = 64 .. 2048 on both sides of each
power of two (one, two and four pairs per lane, nothing padded at n = 64, 256, 2048), keys of tied, negative, signed-zero,
denormal and infinite scores, min_score at its edges, link rows with bits in every word and at both ends of a word, NaN classes,
one-camera rigs under cross_only, invalid boxes and the reach bar under BEV IoU, settle loops of 63 and 64 rounds, pushes over 31
chunks, a cluster of 2048 members, dense graphs of 2048 and of 300 candidates, cap at, one under and far under the number of
clusters and above N.  tests/test_rig_regimes.py asserts on the CPU, from a host model of the schedule, that each case is in its
regime and that the cases tell wrong schedules from the right one.

Every case is compared by the rule of tests/test_gpu_rig.py (its ``equals_the_yardstick``): n, map, info, out[..., :24] and the
flags EQUAL, equal finite masks, the fused boxes within 1e-9, the fp32 boxes the bit-exact rounding of the device's own fp64 boxes.
Then: two runs bit-identical, a workspace holding the star's all-ones link words (and 0xff bytes) under a sparse case, d_box =
NULL, R = 3 against three calls of R = 1, and the id scatter over maps with -2 entries.

Measured on an MI355X (the figure each case prints; copied to profiles/rig.txt): between 0 and 4.44e-16 in the 29 cases - 0 in five of
the small cases (min_score_inf, class_nan, cap_exact, cap_one, cap_256_n4), 4.44e-16 in the two IoU cases with real extrinsics, 2.22e-16 in
star_dense_2048_mean, whose star is a weighted mean over 2048 terms (same order of the sums on both sides: the roundings are the
same, what differs is sin / cos / atan2).  The bar stays 1e-9."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib, rig                                               # noqa: E402
from tests import rig_ref as ref                                              # noqa: E402
from tests import rig_regimes as rr                                           # noqa: E402
from tests.test_gpu_rig import rig_for, run_device, same_bytes, equals_the_yardstick      # noqa: E402

KEYS = ('out', 'box', 'info', 'map', 'n')
_runs = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def refs():
    """name -> (case, the yardstick's result), from the cache of tests/rig_regimes.py; never modified."""
    return {n: rr.case(n) for n in rr.NAMES}


def first_run(name, dev):
    """The undisturbed run of a case, made once per module and shared by the tests that compare against it."""
    if name not in _runs:
        _runs[name] = run_device(rr.case(name)[0], dev)
    return _runs[name]


def host(f):
    return dict(out=f.records.cpu().numpy(), box=f.box.cpu().numpy(), info=f.info.cpu().numpy(), map=f.map.cpu().numpy(), n=f.n.cpu().numpy())


def rig_of(want, case, r):
    """Rig r of a whole-call result, as a result of R = 1."""
    C = case['C']
    return dict(out=want['out'][r:r + 1], box=want['box'][r:r + 1], info=want['info'][r:r + 1], map=want['map'][r * C:(r + 1) * C],
                n=want['n'][r:r + 1])


@pytest.mark.parametrize('name', rr.NAMES)
def test_regimes_equal_the_yardstick(dev, refs, name):
    case, want = refs[name]
    err = equals_the_yardstick(case, first_run(name, dev), want)
    assert err <= 1e-9


@pytest.mark.parametrize('name', ['star_dense_2048_mean', 'dense_2048_flags_on', 'chain_parity0', 'chain_parity1'])
def test_two_runs_are_bit_identical(dev, name):
    assert same_bytes(first_run(name, dev), run_device(rr.case(name)[0], dev))


def test_stale_link_words_change_nothing(dev, refs):
    """One Rig of C = 16, topk = 128: the star leaves every link word of every row set; the sparse rig of 300 candidates through
    the same workspace, and again through a workspace of 0xff bytes, gives the bytes of a fresh Rig and the yardstick's map."""
    case, want = refs['star_dense_2048_mean']
    C = case['C']
    fresh = run_device(case, dev, [3])
    rg = rig_for(case, dev, [0])
    star = host(rg.fuse(torch.from_numpy(case['rec'][:C]).to(dev)))
    assert tuple(star['n'][0]) == (1, 0) and star['info'][0, 0, 2] == 2048
    d_rec = torch.from_numpy(np.ascontiguousarray(case['rec'][3 * C:4 * C])).to(dev)
    ws = rg._ws
    after_star = host(rg.fuse(d_rec))
    again = host(rg.fuse(d_rec))
    rg._ws.fill_(0xff)
    after_ff = host(rg.fuse(d_rec))
    torch.cuda.synchronize()
    assert rg._ws is ws                                                       # one workspace throughout
    for got in (after_star, again, after_ff):
        assert same_bytes(got, fresh)
        assert np.array_equal(got['map'], want['map'][3 * C:4 * C]) and np.array_equal(got['n'], want['n'][3:4])


def test_d_box_may_be_null(dev, refs):
    case, want = refs['sizes_2_5_70_heading_fold']
    lib = _lib.load()
    R, C, topk, cap = case['R'], case['C'], case['topk'], case['cap']
    p = rig.RigParams(**case['params']).to_c()
    d_rec = torch.from_numpy(case['rec']).to(dev)
    d_ext = torch.from_numpy(case['ext'].reshape(R * C, 12)).to(dev)
    ws = torch.zeros(int(lib.rtm3d_rig_workspace_bytes(R, C, topk)), dtype=torch.uint8, device=dev)
    res = []
    for with_box in (True, False):
        out = torch.full((R, cap, 32), 7.0, dtype=torch.float32, device=dev)
        box = torch.full((R, cap, 7), 7.0, dtype=torch.float64, device=dev)
        info = torch.full((R, cap, 4), 7, dtype=torch.int32, device=dev)
        omap = torch.full((R * C, topk), 7, dtype=torch.int32, device=dev)
        n = torch.full((R, 2), 7, dtype=torch.int32, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(lib.rtm3d_rig_fuse(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), R, C, topk, cap, P(d_rec), P(d_ext),
                                      ctypes.byref(p), P(out), P(box) if with_box else None, P(info), P(omap), P(n), P(ws)), 'rig_fuse')
        torch.cuda.synchronize()
        res.append(dict(out=out.cpu().numpy(), box=box.cpu().numpy(), info=info.cpu().numpy(), map=omap.cpu().numpy(), n=n.cpu().numpy()))
    a, b = res
    assert same_bytes(a, first_run(case['name'], dev))
    assert all(a[k].tobytes() == b[k].tobytes() for k in KEYS if k != 'box') and (b['box'] == 7.0).all()      # d_box untouched, the rest equal
    assert np.array_equal(b['map'], want['map'])


def test_three_rigs_equal_three_calls_of_one(dev, refs):
    case, want = refs['odd_n_three_rigs']
    assert case['R'] == 3 and (case['C'] * case['topk']) % 2 == 1
    both = first_run(case['name'], dev)
    for r in range(3):
        assert same_bytes(run_device(case, dev, [r]), rig_of(both, case, r)), r


@pytest.mark.parametrize('name', ['cap_one', 'cap_plus_one'])
def test_scatter_ids_over_dropped_clusters(dev, refs, name):
    case, want = refs[name]
    rg = rig_for(case, dev)
    f = rg.fuse(torch.from_numpy(case['rec']).to(dev))
    m = f.map.cpu().numpy()
    assert np.array_equal(m, want['map']) and (m == -1).any() and (m == -2).any() and (m >= 0).any()
    rng = np.random.Generator(np.random.PCG64(11))
    ids_rig = rng.integers(1, 400, (case['R'], case['cap'])).astype(np.int32) * np.where(rng.random((case['R'], case['cap'])) < 0.5, -1, 1).astype(np.int32)
    got = rg.camera_ids(torch.from_numpy(ids_rig).to(dev), f).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, ref.scatter_ids(m, ids_rig, case['R'], case['C']))
    assert not got[m < 0].any() and (got[m >= 0] != 0).all()
