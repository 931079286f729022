"""Host side of the head backward: the two CPU yardsticks against each other, the parameter chain rule, the gather tables of the
refresh, the K-slice table and every refusal of the host check functions.  No GPU."""
import ctypes

import numpy as np
import pytest

from rtm3d_amd import _lib
from rtm3d_amd import plan as plan_mod
from tests import head_backward_cases as cases
from tests import head_backward_ref as ref


def test_module_and_exports():
    import rtm3d_amd
    from rtm3d_amd import head_train
    assert rtm3d_amd.TrainableHeads is head_train.TrainableHeads and rtm3d_amd.HeadBackward is head_train.HeadBackward
    for name in ('rtm3d_head_backward_check', 'rtm3d_head_backward_slices', 'rtm3d_head_backward_workspace_bytes', 'rtm3d_head_go',
                 'rtm3d_head_wgrad', 'rtm3d_head_dgrad', 'rtm3d_head_refresh', 'rtm3d_head_refresh_check'):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


@pytest.mark.parametrize('cid', sorted(cases.INT_CASES))
def test_integer_cases_are_exact_in_both_yardsticks(cid):
    case = cases.int_case(**cases.INT_CASES[cid])
    q, r = ref.flat(ref.chain(case, True)), ref.flat(ref.chain(case, False))
    cases.check_exact(case, q)
    assert sorted(q) == sorted(r)
    for name in q:
        assert np.array_equal(q[name], r[name]), name
    assert any(np.abs(v).max() > 0 for n, v in q.items() if n.startswith('dw1'))       # the chain reaches the first conv


@pytest.mark.parametrize('S', [1.0, 1024.0])
def test_q16_against_r64(S):
    """What fp16 gradient storage costs: per tensor the max-abs distance of Q16 to R64, relative to the tensor's largest magnitude."""
    case = cases.real_case(11, 1, 6, 7, S)
    q, r = ref.flat(ref.chain(case, True)), ref.flat(ref.chain(case, False), S)
    for name in sorted(r):
        top = float(np.abs(r[name]).max())
        rel = float(np.abs(q[name] - r[name]).max()) / top if top > 0 else 0.0
        print('S=%g %s: max|R64| %.3e  |Q16 - R64| / max %.3e' % (S, name, top, rel))
        assert rel <= 2.0 ** -8, name          # fp16 keeps 11 bits; a sum of rounded terms stays well inside 8


def test_parameter_chain_rule_against_unfolded_autograd():
    rng = np.random.Generator(np.random.PCG64(5))
    co, ci, B, H, W, eps = 8, 6, 2, 5, 7, plan_mod.BN_EPS
    x, w, b = rng.standard_normal((B, ci, H, W)), rng.standard_normal((co, ci, 3, 3)), rng.standard_normal(co)
    gamma, beta, mean, var = rng.standard_normal(co), rng.standard_normal(co), rng.standard_normal(co), rng.random(co) + 0.5
    dy = rng.standard_normal((B, co, H, W))
    for dil in (1, 6):
        dw_u, db_u = ref.unfolded_param_grads(x, w, b, gamma, beta, mean, var, eps, dy, dil)
        import torch
        s = gamma / np.sqrt(var + eps)
        _, dwf, dbf = ref._layer_grads(torch.as_tensor(x), torch.as_tensor(w * s[:, None, None, None]), torch.as_tensor(dy), dil, need_dx=False)
        S = 64.0                                 # the rule: dw = s (1/S) sum (S dy) x
        assert np.allclose((dwf * S / S).numpy() * s[:, None, None, None], dw_u.numpy(), rtol=1e-12, atol=1e-12)
        assert np.allclose(dbf.numpy() * s, db_u.numpy(), rtol=1e-12, atol=1e-12)


def test_perm_tables_equal_the_host_packers_as_bytes():
    from rtm3d_amd import head_train as ht
    rng = np.random.Generator(np.random.PCG64(9))
    # the MFMA packing of a 256 -> G*256 conv (conv_d6) and of one 256 -> 256 group (conv_d1), both bn tiles
    for cout, bn in ((512, 128), (256, 128), (256, 64)):
        w = rng.standard_normal((9, cout, 256)).astype(np.float32)
        src = 1000 + np.arange(w.size, dtype=np.int64).reshape(w.shape)
        flat = np.concatenate([np.zeros(1000, np.float32), w.reshape(-1)])
        pack = lambda a: plan_mod.pack_mfma_weights(a, bn)[0]
        perm = ht.perm_through(pack, src)
        gathered = np.where(perm >= 0, flat[np.maximum(perm, 0)], 0).astype(np.float16)
        assert gathered.tobytes() == pack(w).tobytes()
    # the final convs (pack_headout_weights): ragged K, padding rows
    ws = [rng.standard_normal((k, 256, 3, 3)).astype(np.float32) for k in (3, 16, 2, 2)]
    offs = np.cumsum([0] + [w.size for w in ws])
    flat = np.concatenate([w.reshape(-1) for w in ws])
    pack = lambda p: plan_mod.pack_headout_weights(p, [np.zeros(len(x), np.float32) for x in p])[0]
    perm = ht.perm_through(pack, [offs[i] + np.arange(w.size, dtype=np.int64).reshape(w.shape) for i, w in enumerate(ws)])
    gathered = np.where(perm >= 0, flat[np.maximum(perm, 0)], 0).astype(np.float16)
    assert gathered.tobytes() == pack(ws).tobytes()


def _slices(npix, want):
    n, t = ctypes.c_int(), ctypes.c_int()
    rc = _lib.load().rtm3d_head_backward_slices(npix, want, ctypes.byref(n), ctypes.byref(t))
    return rc, n.value, t.value


def test_slice_table():
    assert _slices(35, 8) == (0, 2, 1)                  # fewer pixel tiles (2) than slices asked for
    assert _slices(780, 7) == (0, 7, 4)                 # 25 tiles: six slices of 4 and a remainder slice of 1
    assert _slices(1, 8) == (0, 1, 1)                   # one pixel
    assert _slices(33, 1) == (0, 1, 2)                  # B H W no multiple of the tile
    for npix in (1, 31, 32, 33, 1000, 983040):
        for want in (1, 3, 8, 64, 256):
            rc, n, t = _slices(npix, want)
            tiles = -(-npix // 32)
            assert rc == 0 and 1 <= n <= want and (n - 1) * t < tiles <= n * t


def _refused(rc, text):
    assert rc != 0
    msg = _lib.load().rtm3d_last_error().decode()
    assert text in msg, msg
    return rc


def test_refusals_of_the_host_functions():
    lib = _lib.load()
    K = (ctypes.c_int * 4)(3, 16, 2, 2)
    chk = lambda B=2, H=8, W=8, G=4, K=K, n=2, S=1.0: lib.rtm3d_head_backward_check(B, H, W, G, K, n, S)
    assert chk() == 0
    assert _refused(chk(K=None), 'null pointer') == 1
    assert _refused(chk(B=0), 'B, H, W = 0, 8, 8') == 2
    assert _refused(chk(H=20000), 'each must be 1 .. 16384') == 2
    assert _refused(chk(G=3), '3 head branches') == 3
    assert _refused(chk(K=(ctypes.c_int * 4)(3, 17, 2, 2)), 'head 1 has 17 output channels') == 4
    assert _refused(chk(K=(ctypes.c_int * 4)(0, 16, 2, 2)), 'head 0 has 0 output channels') == 4
    assert _refused(chk(n=0), 'HEADER_NUM_CONV = 0') == 5
    for S in (3.0, 0.0, -2.0, float('inf'), float('nan')):
        assert _refused(chk(S=S), 'is no power of two') == 6
    assert chk(S=2.0 ** -3) == 0 and chk(S=2.0 ** 15) == 0
    assert _refused(_slices(0, 1)[0], '0 pixels') == 2
    assert _refused(_slices(100, 0)[0], '0 slices asked for') == 7
    assert _refused(_slices(100, 257)[0], '257 slices asked for') == 7
    assert lib.rtm3d_head_backward_workspace_bytes(3, 1) == 0 and lib.rtm3d_head_backward_workspace_bytes(4, 0) == 0
    assert lib.rtm3d_head_backward_workspace_bytes(2, 3) == (3 * 2 * 9 * 256 * 256 + 1024 * 2 * 256) * 4
    # the launch entry points refuse before they launch: no device is touched on these paths
    buf = (ctypes.c_char * 64)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    m = lambda C=64, P=1, coff=0, gs=16, d=addr: _lib.HbMapC(d, C, P, coff, gs)
    dl = (ctypes.c_void_p * 4)(addr, addr, addr, addr)
    go = lambda mp, K=K, S=1.0: lib.rtm3d_head_go(None, 2, 8, 8, 4, K, dl, S, ctypes.byref(mp))
    assert _refused(go(m(d=None)), 'go is a NULL pointer') == 1
    assert _refused(go(m(d=addr + 2)), 'the address of go is no multiple of 16') == 9
    assert _refused(go(m(C=48)), 'do not fit 48 channels') == 4
    assert _refused(go(m(coff=4)), 'in steps of 8') == 4
    assert _refused(go(m(), S=5.0), 'is no power of two') == 6
    nul = (ctypes.c_void_p * 4)()
    one = (ctypes.c_void_p * 4)(addr, None, None, None)
    valid = (ctypes.c_int * 4)(256, 256, 256, 256)
    wg = lambda dy, x, G=4, dil=1, cout=256, valid=valid, want=4, ws=addr, nbytes=1 << 40, dw=one: lib.rtm3d_head_wgrad(
        None, 2, 8, 8, G, dil, cout, valid, ctypes.byref(dy), ctypes.byref(x), 1.0, nul, dw, nul, want, ws, nbytes, addr)
    big = lambda P=1: m(C=1024, P=P, gs=256)
    assert _refused(wg(big(), big(), cout=64), '64 gradient channels per branch') == 4
    assert _refused(wg(big(), big(P=0)), 'X has a border of 0 pixels, its reader\'s taps need 1') == 8
    assert _refused(wg(big(), m(C=256, P=1, gs=0), dil=6), 'its reader\'s taps need 6') == 8
    assert _refused(wg(m(C=2048, gs=512), big()), 'must be adjacent') == 4
    assert _refused(wg(big(), big(), valid=(ctypes.c_int * 4)(256, 300, 256, 256)), 'branch 1 has 300 of 256') == 4
    assert _refused(wg(big(), big(), want=0), '0 slices asked for') == 7
    assert _refused(wg(big(), big(), nbytes=1024), 'the workspace has 1024 bytes') == 10
    assert _refused(wg(big(), big(), ws=None), 'null pointer') == 1
    dg = lambda dy, out, n_out=4, n_sum=1, dil=1, kc=256, wr=addr: lib.rtm3d_head_dgrad(None, 2, 8, 8, n_out, n_sum, dil, kc, ctypes.byref(dy),
                                                                                        wr, None, ctypes.byref(out))
    assert _refused(dg(big(), big(), n_out=4, n_sum=4), '4 outputs each summing 4 branches') == 3
    assert _refused(dg(big(), big(), dil=6), 'dY has a border of 1 pixels, its reader\'s taps need 6') == 8
    assert _refused(dg(big(), big(), kc=32), '32 gradient channels per branch') == 4
    assert _refused(dg(big(), big(), wr=None), 'null pointer') == 1
    assert _refused(dg(big(), big(), wr=addr + 8), 'the address of the weights') == 9
    job = lambda dst=addr, perm=addr, n=4, kind=0: (_lib.HbRefreshJobC * 1)(_lib.HbRefreshJobC(dst, perm, n, kind, 0))
    assert lib.rtm3d_head_refresh_check(1, job()) == 0
    assert _refused(lib.rtm3d_head_refresh_check(0, job()), '0 jobs') == 7
    assert _refused(lib.rtm3d_head_refresh_check(1, job(dst=None)), 'job 0: NULL pointer') == 1
    assert _refused(lib.rtm3d_head_refresh_check(1, job(kind=2)), 'kind 2 is neither') == 4
    assert _refused(lib.rtm3d_head_refresh_check(1, job(n=0)), '0 elements') == 2
    assert _refused(lib.rtm3d_head_refresh_check(1, job(perm=addr + 2)), 'misaligned pointer') == 9


def test_python_refusals():
    from rtm3d_amd import head_train as ht
    with pytest.raises(ValueError, match='no power of two'):
        ht.HeadBackward(1, 4, 4, (3,), 2, 'cpu', grad_scale=3.0)
    with pytest.raises(RuntimeError, match='3 head branches'):
        ht.check(1, 4, 4, (3, 2, 2), 2, 1.0)
