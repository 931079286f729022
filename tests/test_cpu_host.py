"""CPU (-m "not gpu"): host logic of the product that needs no GPU - the L-BFGS-B header compiled
for the host against SciPy's results, the C-ABI library's exported symbols, config / checkpoint /
ParamList surface, distributed sharding + all-gather over gloo."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rtm3d_amd
from rtm3d_amd import _lib, weights, distributed as rdist
from tests.util import load_golden, solver_tail_stats

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    return True


@pytest.mark.parametrize('form', ['lb_solve_batch', 'lb_solve_batch_direct'])
def test_lbfgsb_header_host_build_matches_scipy(built, form):
    """Both forms of the solver's search direction against the reference's SciPy results: lb_solve_batch = the published
    subspace step (formk / subsm), lb_solve_batch_direct = the product form (two-loop recursion over the same pairs)."""
    lib = ctypes.CDLL(os.path.join(REPO, 'tests', '_build', 'libhost_lbfgsb.so'))
    g = load_golden('decode3d_cases.npz')
    N = len(g['clses'])
    cls = np.ascontiguousarray(g['clses'], np.int64); uv = np.ascontiguousarray(g['uv'], np.float32)
    K = np.ascontiguousarray(np.tile(g['K'], (N, 1))); dim = np.ascontiguousarray(g['dim_ref']); loc = np.ascontiguousarray(g['ref_loc'])
    x = np.zeros((N, 8)); f = np.zeros(N); nit = np.zeros(N, np.int32); st = np.zeros(N, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    getattr(lib, form)(N, P(cls), P(uv), P(K), P(dim), P(loc), P(x), P(f), P(nit), P(st))
    kept = g['raw_fun'] < 0.1
    np.testing.assert_array_equal(f < 0.1, kept)
    # (published form: 63 of 64 objects agree with SciPy to 1e-11; one stops an iteration apart from it at 1.3e-8: the solver's
    # reciprocal-diagonal Cholesky rounds differently from LAPACK's, and the factr test then fires one step earlier or later.
    # Direct form: kept objects within 5e-12, rejected ones within 5e-7)
    np.testing.assert_allclose(x[kept], g['raw_x'][kept], rtol=0, atol=1e-7)
    np.testing.assert_allclose(x, g['raw_x'], rtol=0, atol=1e-4)
    assert np.abs(nit - g['raw_nit']).max() <= (1 if form == 'lb_solve_batch' else 3)


@pytest.mark.parametrize('form', ['lb_solve_batch', 'lb_solve_batch_direct'])
def test_lbfgsb_header_tail_on_large_reference_fixture(built, form):
    """VERDICT r03 item 3a (host build; the device kernels: tests/test_gpu_parity.py::test_decode3d_large_fixture): 1536 objects
    the REFERENCE solved (SciPy through its own aimFun / jac, tests/golden/make_golden.py::gen_decode3d_large; 876 kept): keep /
    reject decisions identical, >= 99.5 % of the kept boxes within 1e-4, p99 <= 1e-5 - for the published form and the product form
    (measured here: all 876 within 2.7e-5, p99 1-2e-6 for both)."""
    lib = ctypes.CDLL(os.path.join(REPO, 'tests', '_build', 'libhost_lbfgsb.so'))
    g = load_golden('decode3d_large.npz')
    N = len(g['clses'])
    assert N >= 1500
    cls = np.ascontiguousarray(g['clses'], np.int64); uv = np.ascontiguousarray(g['uv'], np.float32)
    K = np.ascontiguousarray(np.tile(g['K'], (N, 1))); dim = np.ascontiguousarray(g['dim_ref']); loc = np.ascontiguousarray(g['ref_loc'])
    x = np.zeros((N, 8)); f = np.zeros(N); nit = np.zeros(N, np.int32); st = np.zeros(N, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    getattr(lib, form)(N, P(cls), P(uv), P(K), P(dim), P(loc), P(x), P(f), P(nit), P(st))
    s = solver_tail_stats(x, f, g)
    assert s['keep_mismatch'] == 0 and s['kept'] >= 800, s
    assert s['within_1e-4'] >= 0.995 and s['p99'] <= 1e-5, s


def test_lbfgsb_direct_form_on_reference_kept_objects(built):
    """The product form on every e2e / planted fixture (286 further objects the reference solved): identical keep / reject
    decisions, kept boxes within 1e-6 of the reference's (bar 1e-4), objective values within 1e-2 relative."""
    from tests.golden.cases import DIM_REF
    lib = ctypes.CDLL(os.path.join(REPO, 'tests', '_build', 'libhost_lbfgsb.so'))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n_kept = n_all = 0
    for name in ('planted_small', 'planted_full', 'e2e_dla34_small', 'e2e_resnet18_small', 'e2e_resnet34_small'):
        g = load_golden(name + '.npz')
        for b in range(len(g['det_n'])):
            if g['det_n'][b] == 0:
                continue
            cls = np.ascontiguousarray(g['det_cls_%d' % b], np.int64)
            N = len(cls)
            uv = np.ascontiguousarray(g['det_verts_%d' % b], np.float32).reshape(N, 16)
            K = np.ascontiguousarray(np.tile(np.asarray(g['K'], np.float64).reshape(1, 9), (N, 1)))
            dim = np.ascontiguousarray(DIM_REF, np.float64); loc = np.array([0, -0.5, 20.0])
            x = np.zeros((N, 8)); f = np.zeros(N); nit = np.zeros(N, np.int32); st = np.zeros(N, np.int32)
            lib.lb_solve_batch_direct(N, P(cls), P(uv), P(K), P(dim), P(loc), P(x), P(f), P(nit), P(st))
            rx, rf = g['d3_raw_x_%d' % b], g['d3_raw_fun_%d' % b]
            kept = rf < 0.1
            np.testing.assert_array_equal(f < 0.1, kept)
            np.testing.assert_allclose(x[kept], rx[kept], rtol=0, atol=1e-6)
            np.testing.assert_allclose(f, rf, rtol=1e-2, atol=1e-6)
            n_kept += int(kept.sum()); n_all += N
    assert n_kept >= 50 and n_all >= 200


@pytest.mark.parametrize('form', ['lb_solve_batch', 'lb_solve_batch_direct'])
def test_lbfgsb_nonfinite_vertices_follow_scipy(built, form):
    """NaN / Inf key points (non-finite logits upstream): the reference's SciPy call returns x0, fun = nan, nit = 0 and the
    object is rejected (nan < 0.1 is False); the product solver does the same with status 3 and no iterations, instead of
    walking a NaN line search up to the iteration limit.  Finite neighbours in the same batch are unaffected."""
    from oracle import decode3d_ref
    from tests.golden.cases import DIM_REF
    lib = ctypes.CDLL(os.path.join(REPO, 'tests', '_build', 'libhost_lbfgsb.so'))
    g = load_golden('decode3d_cases.npz')
    N = 6
    cls = np.ascontiguousarray(g['clses'][:N], np.int64); uv = np.ascontiguousarray(g['uv'][:N], np.float32).copy()
    uv[1, 3] = np.nan; uv[3, 0] = np.inf; uv[4, :] = -np.inf
    K = np.ascontiguousarray(np.tile(g['K'], (N, 1))); dim = np.ascontiguousarray(g['dim_ref']); loc = np.ascontiguousarray(g['ref_loc'])
    x = np.zeros((N, 8)); f = np.zeros(N); nit = np.full(N, -7, np.int32); st = np.full(N, -7, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    getattr(lib, form)(N, P(cls), P(uv), P(K), P(dim), P(loc), P(x), P(f), P(nit), P(st))
    _, raw = decode3d_ref.optim_decode_bbox3d(cls, uv.reshape(N, 8, 2), g['K'].reshape(3, 3), g['dim_ref'], g['ref_loc'], return_raw=True)
    bad = np.array([False, True, False, True, True, False])
    assert (st[bad] == 3).all() and (nit[bad] == 0).all() and not np.isfinite(f[bad]).any()
    assert (raw['nit'][bad] == 0).all() and np.isnan(raw['fun'][bad]).all() and not raw['kept'][bad].any()
    np.testing.assert_array_equal(x[bad], raw['x'][bad])                       # x0, like the reference
    assert (st[~bad] != 3).all()
    np.testing.assert_allclose(x[~bad], g['raw_x'][:N][~bad], rtol=0, atol=1e-4)


def test_library_exports_every_declared_symbol(built):
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    declared = set(re.findall(r'\b(rtm3d_[a-z0-9_]+)\s*\(', hdr))
    declared -= {'rtm3d_conv_desc'}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), 'missing export ' + name
    assert declared == set(_lib.SIGNATURES.keys()), declared ^ set(_lib.SIGNATURES.keys())
    assert _lib.load().rtm3d_abi_version() == _lib.ABI_VERSION
    # the struct mirrored in Python has the C size (checked through a tiny C program)
    src = '#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\nint main(){printf("%%zu", sizeof(rtm3d_conv_desc));return 0;}' % REPO
    exe = os.path.join(REPO, 'tests', '_build', 'sizeof_desc')
    subprocess.run(['gcc', '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    assert int(subprocess.check_output([exe])) == ctypes.sizeof(_lib.ConvDesc)


def test_abi9_solver_form_surface(built):
    """Round 6 (ABI 9): the SciPy-faithful `published` form is what every facade entry passes unless told otherwise, both decode
    entries carry the `form` argument in the header and in the binding (argument counts agree with the C prototypes), unknown forms
    are refused on the host, and the retired side-lane replay is gone from the header, the binding and the library."""
    from rtm3d_amd import model_utils
    assert model_utils.DEFAULT_SOLVER_FORM == 'published' and model_utils.solver_form_id(None) == 1
    assert model_utils.solver_form_id('direct') == 0 and model_utils.solver_form_id('published') == 1
    with pytest.raises(ValueError, match='solver form'):
        model_utils.solver_form_id('scipy')
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert '#define RTM3D_ABI_VERSION 9' in hdr and '#define RTM3D_SOLVER_PUBLISHED 1' in hdr and '#define RTM3D_SOLVER_DIRECT 0' in hdr
    for name in ('rtm3d_decode3d', 'rtm3d_decode3d_slots'):
        proto = re.search(r'int %s\(([^;]*)\);' % name, hdr).group(1)
        assert proto.rstrip().endswith('int form'), name
        assert len(proto.split(',')) == len(_lib.SIGNATURES[name][1]), name
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for gone in ('rtm3d_op_schedule', 'rtm3d_ctx_set_lanes'):
        assert gone not in hdr.replace('rtm3d_op_schedule / rtm3d_ctx_set_lanes', '') and gone not in _lib.SIGNATURES and not hasattr(lib, gone), gone


def test_no_cpu_fallback():
    cfg = rtm3d_amd.kitti_config('DLA-34')
    m = rtm3d_amd.create_model(cfg)
    with pytest.raises(RuntimeError):
        m.to('cpu')
    with pytest.raises(RuntimeError):
        m.eval()(torch.zeros(1, 3, 64, 64))
    with pytest.raises(AssertionError):
        rtm3d_amd.create_model(rtm3d_amd.CfgNode(MODEL=rtm3d_amd.CfgNode(BACKBONE='VGG')))
    # the product never imports the oracle
    for root, _, files in os.walk(os.path.join(REPO, 'rtm3d_amd')):
        for f in files:
            if f.endswith('.py'):
                assert 'oracle' not in open(os.path.join(root, f)).read().replace('CPU oracle', ''), f


def test_unsupported_config_is_refused_loudly():
    """Keys the reference reads that the HIP plan is not built for raise at construction, naming the key - none is ignored
    (MODEL.KFNs: models/nets/keypoint_fpn_fusion.py:11-17; OUT_CHANNELS / HEADER_NUM_CONV: models/nets/header.py:9-13)."""
    for bb, good in (('DLA-34', ['level2', 'level3', 'level4', 'level5']), ('RESNET-18', ['layer1', 'layer2', 'layer3', 'layer4'])):
        cfg = rtm3d_amd.kitti_config(bb)
        assert list(cfg.MODEL.KFNs) == good
        rtm3d_amd.create_model(cfg)                                    # the shipped lists build
        for bad in (good[1:], good[::-1], good[:2], ['level3', 'level4', 'level5', 'level6']):
            c = rtm3d_amd.kitti_config(bb)
            c.MODEL.KFNs = bad
            with pytest.raises(NotImplementedError, match='KFNs'):
                rtm3d_amd.create_model(c)
    # the DLA list on a ResNet (a yaml that overrides BACKBONE but keeps detault.py's KFNs) is refused too
    c = rtm3d_amd.kitti_config('DLA-34')
    c.MODEL.BACKBONE = 'RESNET-18'
    with pytest.raises(NotImplementedError, match='KFNs'):
        rtm3d_amd.create_model(c)
    c = rtm3d_amd.kitti_config('DLA-34')
    c.MODEL.OUT_CHANNELS = 128
    with pytest.raises(NotImplementedError, match='OUT_CHANNELS'):
        rtm3d_amd.create_model(c)
    # HEADER_NUM_CONV is a real parameter since round 5 (one dilation-6 conv + n - 1 dilation-1 convs per branch, header.py:12-13):
    # the state-dict surface follows it under the reference's Sequential indices 3k / 3k + 1; 0 is refused
    for n, keys in ((1, 321 - 4 * 7), (2, 321), (3, 321 + 4 * 7)):       # conv weight + bias, BN weight / bias / mean / var / count
        c = rtm3d_amd.kitti_config('DLA-34')
        c.MODEL.HEADER_NUM_CONV = n
        sd = rtm3d_amd.create_model(c).state_dict()
        assert len(sd) == keys, (n, len(sd))
        assert ('detect_header.main_offset_header.%d.weight' % (3 * (n - 1))) in sd
        assert ('detect_header.main_offset_header.%d.weight' % (3 * n)) not in sd
        assert tuple(sd['detect_header.main_offset_header.main_offset_head.weight'].shape) == (2, 256, 3, 3)
    c = rtm3d_amd.kitti_config('DLA-34')
    c.MODEL.HEADER_NUM_CONV = 0
    with pytest.raises(ValueError, match='HEADER_NUM_CONV'):
        rtm3d_amd.create_model(c)


def test_state_dict_surface_and_checkpoint(tmp_path):
    cfg = rtm3d_amd.kitti_config('RESNET-18')
    m = rtm3d_amd.create_model(cfg)
    sd = m.state_dict()
    assert len(sd) == 207 and 'backbone.layer4.1.bn2.running_var' in sd and 'detect_header.main_kf_header.main_kf_head.bias' in sd
    assert float(sd['backbone.bn1.running_var'].mean()) == 1.0          # reference-style init
    new = weights.synth_state_dict('RESNET-18', 5, 'trained')
    # checkpoint as the reference saves it ({"model": state_dict, ...}), keys nested one level deeper
    path = str(tmp_path / 'model_best.pt')
    torch.save({'model': {('module.' + k): v for k, v in new.items()}, 'epoch': 3}, path)
    from rtm3d_amd.check_point import CheckPointer
    # keys with an extra prefix in the MODEL are matched by suffix, not the other way round: emulate a
    # backbone-only checkpoint (ImageNet style) instead
    torch.save({k[len('backbone.'):]: v for k, v in new.items() if k.startswith('backbone.')}, path)
    CheckPointer(m, mode='state-dict').load(path, use_latest=False)
    assert torch.equal(m.state_dict()['backbone.layer1.0.conv1.weight'], new['backbone.layer1.0.conv1.weight'])
    assert not torch.equal(m.state_dict()['detect_header.main_kf_header.0.weight'], new['detect_header.main_kf_header.0.weight'])
    # a mode='full' file of the reference pickles the module object (utils/check_point.py:123): refused, nothing is unpickled
    full = str(tmp_path / 'model_full.pt')
    torch.save({'model': torch.nn.Linear(2, 2)}, full)
    with pytest.raises(RuntimeError, match='tensors-only'):
        CheckPointer(m, mode='full').load(full, use_latest=False)
    with pytest.raises(RuntimeError):
        m.load_state_dict({'backbone.conv1.weight': torch.zeros(1)})
    bad = dict(new); bad['backbone.conv1.weight'] = torch.zeros(64, 3, 3, 3)
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)


def test_config_merges_reference_yaml(tmp_path):
    y = tmp_path / 'cfg.yaml'
    y.write_text("INPUT_SIZE: (1280, 1280)\nMODEL:\n  BACKBONE: 'RESNET-18'\n  KFNs: ['layer1', 'layer2', 'layer3', 'layer4']\n"
                 "DETECTOR:\n  SCORE_THRESH: 0.4\n  TOPK_CANDIDATES: 100\n  dim_ref:\n    [[1.5, 1.6, 3.9], [1.7, 0.6, 0.8], [1.7, 0.6, 1.7]]\n")
    c = rtm3d_amd.CONFIGS.clone()
    c.merge_from_file(str(y))
    assert c.INPUT_SIZE == (1280, 1280) and c.MODEL.BACKBONE == 'RESNET-18' and c.MODEL.OUT_CHANNELS == 256
    assert c.DETECTOR.TOPK_CANDIDATES == 100 and len(c.DETECTOR.dim_ref) == 3
    assert rtm3d_amd.CONFIGS.DETECTOR.TOPK_CANDIDATES == 30          # defaults untouched (clone)


def test_paramlist():
    p = rtm3d_amd.ParamList((640, 640))
    p.add_field('class', [0, 2]); p.add_field('Ry', np.array([0.1, 0.2])); p.add_field('t', torch.ones(2))
    q = p.numpy()
    assert q.get_field('class') == [0, 2] and isinstance(q.get_field('t'), np.ndarray) and p.has_field('Ry') and 'Ry' in p.fields()


def test_checkpoint_key_alignment_matches_reference():
    """n2: suffix matching of checkpoint keys against vectors produced by running the reference's own
    align_and_update_state_dicts (tests/golden/make_golden_checkpoint.py): identical keys, an ImageNet-style backbone
    file, a DataParallel-wrapped file (nothing matches), deeper nesting, ambiguous suffixes, partial overlap."""
    import json
    from rtm3d_amd.check_point import align_and_update_state_dicts
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'checkpoint_align_cases.json')) as f:
        cases = json.load(f)
    assert len(cases) >= 6
    for name, c in cases.items():
        msd = {k: torch.tensor(-1) for k in c['model_keys']}
        lsd = {k: torch.tensor(i) for i, k in enumerate(c['loaded_keys'])}
        align_and_update_state_dicts(msd, lsd)
        assert [int(msd[k]) for k in c['model_keys']] == c['chosen'], name


def test_shard_ranges():
    for total, world in [(256, 8), (10, 3), (5, 8), (32, 1)]:
        r = [rdist.shard_range(total, k, world) for k in range(world)]
        assert r[0][0] == 0 and r[-1][1] == total and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert max(h - l for l, h in r) - min(h - l for l, h in r) <= 1


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    topk, b = 5, 3
    lo, hi = rdist.shard_range(world * b, rank, world)
    gen = torch.Generator().manual_seed(100 + rank)
    n = torch.tensor([2, 0, 5], dtype=torch.int32)
    cls = torch.randint(0, 3, (b * topk,), generator=gen)
    score = torch.rand(b * topk, generator=gen); mproj = torch.rand(b * topk, 2, generator=gen)
    verts = torch.rand(b * topk, 8, 2, generator=gen); bbox = torch.rand(b * topk, 4, generator=gen)
    from tests.util import pack_records_reference
    rec = pack_records_reference(n, cls, score, mproj, verts, bbox, topk)      # CPU tensors: the product packer is HIP-only
    allrec = rdist.all_gather_records(rec, check_shapes=True)
    assert allrec.shape == (world * b, topk, rdist.RECORD)
    assert torch.equal(allrec[lo:hi], rec)
    un = rdist.unpack_records(allrec[lo:hi])
    assert un[1] is None and len(un[0]['cls']) == 2 and len(un[2]['cls']) == 5
    assert torch.equal(un[0]['cls'], cls[:2]) and torch.equal(un[2]['verts'], verts[2 * topk:3 * topk])
    q.put((rank, float(allrec.sum())))
    dist.destroy_process_group()


def test_all_gather_records_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 1000)
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    res = dict(q.get() for _ in range(2))
    assert res[0] == res[1]           # every rank holds the same gathered batch


def _gloo_uneven_worker(rank, world, port, q):
    """10 images over 3 ranks: padded equal shards (4, 4, 2 + 2 padding), gathered, trimmed, unpacked."""
    import torch.distributed as dist
    from tests.util import pack_records_reference
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    total, topk = 10, 4
    lo, hi, per = rdist.padded_shard(total, rank, world)
    assert per == 4 and hi - lo == (4, 4, 2)[rank]
    # global, rank-independent synthetic detections: image g has (g % 5) objects of class g % 3
    def image(gidx):
        gen = torch.Generator().manual_seed(1000 + gidx)
        return gidx % 5, torch.full((topk,), gidx % 3, dtype=torch.int64), torch.rand(topk, generator=gen)
    n, cls, score = [], [], []
    for slot in range(per):
        gidx = lo + slot
        cnt, c, sc = image(min(gidx, total - 1))            # padding slots repeat the last image
        n.append(cnt); cls.append(c); score.append(sc)
    n = torch.tensor(n, dtype=torch.int32); cls = torch.cat(cls); score = torch.cat(score)
    z2, z16, z4 = torch.zeros(per * topk, 2), torch.zeros(per * topk, 8, 2), torch.zeros(per * topk, 4)
    rec = pack_records_reference(n, cls, score, z2, z16, z4, topk)
    allrec = rdist.trim_gathered(rdist.all_gather_records(rec, check_shapes=True), total)
    assert allrec.shape == (total, topk, rdist.RECORD)
    un = rdist.unpack_records(allrec)
    for gidx in range(total):
        cnt, c, sc = image(gidx)
        if cnt == 0:
            assert un[gidx] is None
        else:
            assert len(un[gidx]['cls']) == cnt and torch.equal(un[gidx]['cls'], c[:cnt]) and torch.equal(un[gidx]['score'], sc[:cnt])
    # uneven shapes handed to the collective are caught by the guard, on every rank
    bad = rec[: per - (1 if rank == 2 else 0)]
    try:
        rdist.all_gather_records(bad, check_shapes=True)
        ok = False
    except ValueError:
        ok = True
    q.put((rank, ok, float(allrec.sum())))
    dist.destroy_process_group()


def test_all_gather_records_gloo_world3_uneven_shards():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 200)
    ps = [ctx.Process(target=_gloo_uneven_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(180)
        assert p.exitcode == 0
    res = [q.get() for _ in range(3)]
    assert all(ok for _, ok, _ in res) and len(set(s for _, _, s in res)) == 1


def _gloo_config3_worker(rank, world, port, q):
    """BASELINE config[3] geometry: 256 images = 8 ranks x 32, top-100 records of 32 floats (410 KB per rank, 3.3 MB gathered);
    image g carries (g * 7) % 101 detections whose score encodes (g, slot), so any mis-ordered block shows."""
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    total, topk = 256, 100
    lo, hi, per = rdist.padded_shard(total, rank, world)
    assert (lo, hi, per) == (rank * 32, rank * 32 + 32, 32) == rdist.shard_range(total, rank, world) + (32,)
    rec = torch.zeros(per, topk, rdist.RECORD)
    for slot in range(per):
        g = lo + slot
        cnt = (g * 7) % 101
        rec[slot, :cnt, 0] = g % 3
        rec[slot, :cnt, 1] = (g * 128 + torch.arange(cnt)).float() / 65536.0           # exact in fp32
        rec[slot, :cnt, 31] = 1.0
    assert rec.numel() * 4 == 409600
    allrec = rdist.trim_gathered(rdist.all_gather_records(rec, check_shapes=True), total)
    assert allrec.shape == (total, topk, rdist.RECORD) and torch.equal(allrec[lo:hi], rec)
    un = rdist.unpack_records(allrec)
    for g in range(total):
        cnt = (g * 7) % 101
        if cnt == 0:
            assert un[g] is None
            continue
        assert len(un[g]['cls']) == cnt and int(un[g]['cls'][0]) == g % 3
        assert torch.equal(un[g]['score'], (g * 128 + torch.arange(cnt)).float() / 65536.0)
    q.put((rank, float(allrec.double().sum())))
    dist.destroy_process_group()


def test_all_gather_records_gloo_world8_config3_geometry():
    """The collective of the 8-GPU configuration (bs = 256 sharded 8 x 32), rehearsed on CPU ranks over gloo: contiguous
    shards, ONE all_gather_into_tensor of (32, 100, 32) fp32 per rank, results ordered by global image index on every rank."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29900 + (os.getpid() % 90)
    ps = [ctx.Process(target=_gloo_config3_worker, args=(r, 8, port, q)) for r in range(8)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(240)
        assert p.exitcode == 0
    res = dict(q.get() for _ in range(8))
    assert len(res) == 8 and len(set(res.values())) == 1


def test_box_projection_matches_reference_golden_vectors():
    """n3: rotation_matrix / create_corners / calc_proj_corners against the vectors produced by running the
    reference (tests/golden/make_golden_project.py), incl. yaw values inside its 1e-3 snapping window."""
    from rtm3d_amd import kitti_results as kr
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'project_cases.npz'))
    for i in range(len(g['Ry'])):
        c = kr.create_corners(g['dimension'][i], g['location'][i], kr.rotation_matrix(g['Ry'][i]))
        np.testing.assert_array_equal(c, g['corners'][i])
        p = kr.calc_proj_corners(g['dimension'][i], g['location'][i], g['Ry'][i], g['K'])
        np.testing.assert_array_equal(p, g['proj'][i])


def test_kitti_label_lines(tmp_path):
    from rtm3d_amd import kitti_results as kr
    from rtm3d_amd.ParamList import ParamList
    K = np.array([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]])
    pl = ParamList((1280, 384))
    pl.add_field('class', [0, 2]); pl.add_field('Ry', [0.3, -1.2])
    pl.add_field('dimension', [[1.5, 1.6, 3.9], [1.7, 0.6, 1.8]]); pl.add_field('location', [[2.0, 1.0, 20.0], [-60.0, 1.0, 10.0]])
    pl.add_field('K', [K.reshape(-1), K.reshape(-1)])
    lines = kr.kitti_label_lines(pl, image_size=(1280, 384))
    assert len(lines) == 2
    a = lines[0].split()
    assert a[0] == 'Car' and len(a) == 16
    assert abs(float(a[12]) - (1.0 + 0.75)) < 1e-9            # bottom-face y = centre y + h/2
    assert abs(float(a[3]) - (0.3 - np.arctan2(2.0, 20.0))) < 5e-3
    assert [float(v) for v in a[8:11]] == [1.5, 1.6, 3.9]
    proj, boxes = kr.project_boxes(pl)
    assert proj.shape == (2, 9, 2) and abs(float(a[4]) - boxes[0, 0]) < 5e-3
    b = lines[1].split()
    assert b[0] == 'Cyclist' and float(b[4]) == 0.0           # clipped to the image
    n = kr.write_kitti_label_file(str(tmp_path / 'data' / '000001.txt'), pl)
    assert n == 2 and len(open(str(tmp_path / 'data' / '000001.txt')).read().splitlines()) == 2
    assert kr.write_kitti_label_file(str(tmp_path / 'data' / '000002.txt'), None) == 0


def test_float_estimate_division_is_exact_for_small_quotients():
    """csrc/common.h div_small_q: q = int(float(m) * (1/d)), fixed up by +-1 from the remainder, is exact for
    0 <= m < 2^31 whenever the quotient is below 2^21 (pixel -> image / row index).  Same arithmetic in numpy."""
    rng = np.random.default_rng(5)
    for d in (1, 2, 3, 7, 20, 80, 160, 320, 1280, 1920, 30720, 491520, 2 ** 20 + 1, 2 ** 24 + 3):
        qmax = min(2 ** 21 - 1, (2 ** 31 - 1) // d)
        q_true = np.concatenate([rng.integers(0, qmax + 1, 20000), [0, 1, qmax]]).astype(np.int64)
        r_true = np.concatenate([rng.integers(0, d, 20000), [0, d - 1, d - 1]]).astype(np.int64)
        m = q_true * d + r_true
        m = m[m < 2 ** 31]
        rcp = np.float32(1.0) / np.float32(d)
        q = (m.astype(np.float32) * rcp).astype(np.int64)
        r = m - q * d
        q = q + (r >= d).astype(np.int64) - (r < 0).astype(np.int64)
        np.testing.assert_array_equal(q, m // d)


# ------------------------------------------------------------------ bench.py rank launcher
def _run_bench(argv, env_extra=None, timeout=300):
    import subprocess
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(env_extra or {})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, os.path.join(root, 'bench.py')] + argv, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize('n', [2, 8])
def test_bench_launcher_dry_launch(n):
    """`python bench.py --gpus N` must start N ranks ITSELF (the reference: mp.spawn, train_multi_gpu.py:239-245).  Rehearsed
    without GPUs: --dry-launch runs the launcher, the shard plumbing and the preallocated all-gather over gloo and prints the
    JSON line with n_gpus = N and every rank's record block seen intact; the line is marked INVALID (no hot path ran)."""
    import json
    r = _run_bench(['--gpus', str(n), '--dry-launch', '--steps', '2', '--warmup', '1', '--batch', '32' if n == 8 else '4'])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout                       # ONE line, from rank 0
    out = json.loads(lines[0])
    assert out['n_gpus'] == n and out['multi_gpu']['ranks_seen'] == n
    assert out['multi_gpu']['block_ranks'] == list(range(n))           # ordered by global image index
    assert len(out['multi_gpu']['per_rank_ms_per_step']) == n
    assert out['config']['global_batch'] == n * (32 if n == 8 else 4)
    assert 'INVALID' in out and out['value'] is None


def test_bench_dump_outputs_dry_launch(tmp_path):
    """`--dump-outputs DIR` writes the last timed step's gathered records as DIR/records.npy (float32), identical from run to
    run with the same arguments; `--steps` is echoed and ms_per_step reported."""
    import json
    outs = []
    for k in range(2):
        d = str(tmp_path / ('run%d' % k))
        r = _run_bench(['--gpus', '2', '--dry-launch', '--steps', '3', '--warmup', '1', '--batch', '4', '--dump-outputs', d])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][0])
        assert line['steps'] == 3 and line['ms_per_step'] > 0
        assert sorted(os.listdir(d)) == ['records.npy']
        outs.append(np.load(os.path.join(d, 'records.npy')))
    assert outs[0].dtype == np.float32 and outs[0].shape == (8, 100, rdist.RECORD)
    np.testing.assert_array_equal(outs[0], outs[1])
    assert outs[0][:, 0, 0].tolist() == [0.0] * 4 + [1.0] * 4          # both ranks' blocks, in rank order


def test_bench_dump_outputs_budget(tmp_path):
    """Outputs over the 64 MB budget keep a fixed seeded sample of rows, and say which rows."""
    import bench
    big = torch.arange(96 * 2 ** 18, dtype=torch.float32).reshape(96, 2 ** 18)          # 96 MB
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), {'records': big, 'n': torch.arange(96, dtype=torch.int32)})
    a, rows = np.load(str(tmp_path / '0' / 'records.npy')), np.load(str(tmp_path / '0' / 'records_rows.npy'))
    assert a.dtype == np.float32 and rows.dtype == np.float64 and np.load(str(tmp_path / '0' / 'n.npy')).dtype == np.float32
    assert sum(os.path.getsize(str(tmp_path / '0' / f)) for f in os.listdir(str(tmp_path / '0'))) <= bench.DUMP_BUDGET_BYTES
    np.testing.assert_array_equal(a, big.numpy()[rows.astype(np.int64)])
    np.testing.assert_array_equal(a, np.load(str(tmp_path / '1' / 'records.npy')))


def test_bench_refuses_world_size_mismatch():
    """Under a launcher that started a different number of ranks than --gpus claims, bench.py exits non-zero (it used to
    print a note and measure WORLD_SIZE ranks silently)."""
    r = _run_bench(['--gpus', '4', '--dry-launch'], {'RANK': '0', 'WORLD_SIZE': '2', 'LOCAL_RANK': '0'})
    assert r.returncode != 0 and 'WORLD_SIZE=2' in r.stderr
    if torch.cuda.device_count() < 2:
        r = _run_bench(['--gpus', '2'])                      # fewer GPUs than ranks: the launcher refuses before starting anything
        assert r.returncode != 0 and 'GPUs' in r.stderr


def test_all_gather_records_out_buffer_checks():
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(29700 + os.getpid() % 200)
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        rec = torch.rand(3, 100, rdist.RECORD)
        buf = rdist.gathered_buffer(rec)
        out = rdist.all_gather_records(rec, always=True, out=buf)
        assert out is buf and torch.equal(buf, rec)
        with pytest.raises(ValueError):
            rdist.all_gather_records(rec, always=True, out=torch.zeros(2, 100, rdist.RECORD))
    finally:
        dist.destroy_process_group()
