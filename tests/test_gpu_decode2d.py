"""GPU (-m gpu): the 2D decode (rtm3d_amd/csrc/decode2d.hip: stand-alone sigmoid, NMS + append, select-and-gather, the
peaks-only finish and the SMOKE decode) through the C ABI, over every regime its launch code can take.  The cases and the
regimes they name are tests/decode2d_cases.py; tests/test_decode2d_cpu.py proves on the CPU that each case is in the regime it
names.

Every run: all six output arrays are filled with a sentinel and sit between guard words, the workspace is exactly
rtm3d_decode2d_workspace_bytes long with guard words after it.  Afterwards the guards are intact, rows at or above n[b] are
still the sentinel, rows below are fully written.  Each case runs twice on the same buffers and must give identical bits (atomics
decide the order of the candidate list; it must not show).

References: oracle.rtm3d_ref.inference on the CPU, bit for bit (non-finite values in the same places, `bbox` included); for the
cases whose scores tie, the NumPy restatement of the documented contract (tests/decode2d_ref.py: score descending, ties by
ascending class-major flat index), which test_decode2d_cpu.py pins to the oracle on every case without ties.  In the one regime
in which torch.sigmoid is itself not defined bit for bit (an image of >= 32768 elements that is no multiple of 32: its scalar
tails move with torch's thread count) class, cell and count equal the oracle's and every score is one of the two torch forms of
its logit.  The SMOKE decode is compared with oracle/smoke_ref.decode's formulas at rtol 1e-9 / atol 1e-9, the bar of
test_smoke_head_variant_self_consistency.  Nothing else has a tolerance.

Reference quirk, not asserted and not copied by the kernel: in the reference a NaN heat cell occupies a top-k slot before the
threshold removes it (topk = 1 with one NaN cell returns nothing), so the non-finite cases keep n + NaN cells below topk."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rtm3d_amd import _lib                                  # noqa: E402
from tests import decode2d_cases as dc                      # noqa: E402
from tests import decode2d_ref as R                         # noqa: E402

GUARD = 256                     # bytes of guard on both sides of every output array and after the workspace
GUARD_BYTE = 0xC3
SENT = {'n': np.int32(-77), 'cls': np.int64(-77), 'score': np.float32(-1234.5), 'mproj': np.float32(-1234.5),
        'verts': np.float32(-1234.5), 'bbox': np.float32(-1234.5)}
WIDTH = {'cls': 1, 'score': 1, 'mproj': 2, 'verts': 16, 'bbox': 4}
FIELDS = ('cls', 'score', 'mproj', 'verts', 'bbox')


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """A device array of `shape` filled with `sentinel`, GUARD bytes of GUARD_BYTE on both sides."""

    def __init__(self, shape, sentinel):
        self.shape, self.sentinel = tuple(shape), sentinel
        self.nbytes = int(np.prod(self.shape)) * sentinel.dtype.itemsize
        self.buf = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device='cuda')
        assert self.buf.data_ptr() % 8 == 0
        self.poison()

    def poison(self):
        host = np.full(2 * GUARD + self.nbytes, GUARD_BYTE, np.uint8)
        host[GUARD:GUARD + self.nbytes] = np.full(self.shape, self.sentinel).view(np.uint8).ravel()
        self.buf.copy_(torch.from_numpy(host))

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def read(self):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == GUARD_BYTE).all() and (host[GUARD + self.nbytes:] == GUARD_BYTE).all(), 'guard words overwritten'
        return host[GUARD:GUARD + self.nbytes].copy().view(self.sentinel.dtype).reshape(self.shape)


class Slots:
    def __init__(self, B, topk):
        self.B, self.topk = B, topk
        self.a = {'n': Guarded((B,), SENT['n'])}
        for k in FIELDS:
            self.a[k] = Guarded((B, topk, WIDTH[k]) if WIDTH[k] > 1 else (B, topk), SENT[k])

    def poison(self):
        for g in self.a.values():
            g.poison()

    def ptrs(self):
        return [self.a[k].ptr for k in ('n',) + FIELDS]

    def read(self):
        torch.cuda.synchronize()
        return {k: g.read() for k, g in self.a.items()}


class Workspace:
    """Exactly rtm3d_decode2d_workspace_bytes bytes, GUARD bytes of guard after them."""

    def __init__(self, lib, shape):
        self.nbytes = int(lib.rtm3d_decode2d_workspace_bytes(*shape))
        self.buf = torch.full((self.nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device='cuda')
        assert self.buf.data_ptr() % 8 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def check(self):
        torch.cuda.synchronize()
        assert (self.buf[self.nbytes:].cpu().numpy() == GUARD_BYTE).all(), 'the kernels wrote past the workspace'


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def is_sentinel(a, k):
    u = 'u%d' % a.dtype.itemsize
    return np.ascontiguousarray(a).view(u) == np.array([SENT[k]]).view(u)[0]


def run(lib, inp, ws=None, slots=None, peaks_only=False):
    """One rtm3d_decode2d call on poisoned slots; -> (outputs, slots, workspace) after the guard / sentinel checks."""
    heat = inp['heat']
    B, C, H, W = heat.shape
    ws = ws or Workspace(lib, (B, C, H, W))
    slots = slots or Slots(B, inp['topk'])
    slots.poison()
    d = [dev(inp[k]) for k in ('heat', 'offs', 'moff')]
    po, pm = (None, None) if peaks_only else (d[1].data_ptr(), d[2].data_ptr())
    rc = lib.rtm3d_decode2d(stream(), d[0].data_ptr(), po, pm, B, C, H, W, inp['thresh'], inp['topk'], inp['down'], ws.ptr, *slots.ptrs())
    assert rc == 0, lib.rtm3d_last_error()
    out = slots.read()
    ws.check()
    check_rows(out, written=('cls', 'score', 'mproj') if peaks_only else FIELDS)
    return out, slots, ws


def check_rows(out, written=FIELDS):
    """Rows at or above n[b] (and every array the call does not write) are the sentinel; rows below n[b] hold none."""
    topk = out['cls'].shape[1]
    assert ((out['n'] >= 0) & (out['n'] <= topk)).all(), out['n']
    for b, n in enumerate(out['n']):
        for k in FIELDS:
            a = out[k][b].reshape(topk, -1)
            if k in written:
                assert is_sentinel(a[n:], k).all(), '%s: rows at or above n[%d] = %d were written' % (k, b, n)
                if k != 'cls':                                    # (a class id is never the sentinel -77: checked against the reference)
                    assert not is_sentinel(a[:n], k).any(), '%s: a row below n[%d] = %d is not fully written' % (k, b, n)
                else:
                    assert (a[:n] >= 0).all()
            else:
                assert is_sentinel(a, k).all(), '%s was written' % k


def assert_slots_equal(got, ref, fields=FIELDS):
    """n equal; below n[b] non-finite exactly where the reference is (NaN where it is NaN) and bit-equal elsewhere."""
    np.testing.assert_array_equal(got['n'], ref['n'])
    for b, n in enumerate(ref['n']):
        for k in fields:
            g, r = got[k][b, :n], ref[k][b, :n]
            if g.dtype == np.float32:
                np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg='%s image %d: NaN pattern' % (k, b))
                np.testing.assert_array_equal(np.isfinite(g), np.isfinite(r), err_msg='%s image %d: non-finite pattern' % (k, b))
                m = ~np.isnan(r)
                np.testing.assert_array_equal(R.bits(g[m]), R.bits(r[m]), err_msg='%s image %d' % (k, b))
            else:
                np.testing.assert_array_equal(g, r, err_msg='%s image %d' % (k, b))


def assert_same_bits(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg='%s differs between two runs' % k)


_refs = {}


def reference(name):
    """The oracle, or the contract for a case whose scores tie (computed once, shared, never modified)."""
    if name not in _refs:
        inp = dc.build(name)
        _refs[name] = R.contract(inp) if dc.CASES[name]['ties'] else R.oracle(inp)
    return _refs[name]


DEFINED = [n for n in dc.CASES if n != 'heat_undefined_3x100x110']


# ------------------------------------------------------------------------------------------------------------ dense decode
@pytest.mark.parametrize('name', DEFINED)
def test_decode2d_case(lib, name):
    """One dense rtm3d_decode2d call per case, bit for bit against the oracle (the contract where scores tie), twice on the same
    buffers.  The non-finite cases (nf_*): outputs are non-finite exactly where the oracle's are and bit-equal elsewhere, bbox
    included; a NaN heat cell next to a maximum removes that peak.  Reference quirk (not asserted, not copied by the kernel): a
    NaN heat cell also occupies one of the reference's top-k slots before the threshold removes it - topk = 1 with one NaN cell
    returns nothing - so these cases keep n + (NaN heat cells) below topk."""
    inp = dc.build(name)
    out, slots, ws = run(lib, inp)
    ref = reference(name)
    print(name, 'n', out['n'].tolist(), 'reference', ref['n'].tolist())
    assert tuple(ref['n']) == dc.CASES[name]['expect']['n']
    assert_slots_equal(out, ref)
    again, _, _ = run(lib, inp, ws, slots)                     # the same buffers: the candidate order must not show
    assert_same_bits(out, again)


def test_undefined_sigmoid_regime(lib):
    """An image of 33000 elements: torch.sigmoid takes scalar tails whose position moves with its thread count, the kernel
    calls every element "vector".  Asserted: count, class and cell equal the oracle's (the scores are at least 16 ulp apart, so
    neither form can flip the order), every score is one of the two torch forms of its logit, and the key-point fields, which
    do not depend on the heat map's sigmoid, are bit-equal."""
    name = 'heat_undefined_3x100x110'
    inp = dc.build(name)
    out, slots, ws = run(lib, inp)
    ref = R.oracle(inp)
    assert_slots_equal(out, ref, fields=('cls', 'mproj', 'verts', 'bbox'))
    n = int(out['n'][0])
    x, y = (out['mproj'][0, :n, 0] // 4).astype(int), (out['mproj'][0, :n, 1] // 4).astype(int)
    lg = inp['heat'][0][out['cls'][0, :n], y, x]
    v, s, g = R.bits(R.sig_vector(lg)), R.bits(R.sig_scalar(lg)), R.bits(out['score'][0, :n])
    print('score forms: vector', (g == v).sum(), 'scalar', (g == s).sum(), 'of', n, '; forms differ at', (v != s).sum())
    assert ((g == v) | (g == s)).all(), (g, v, s)
    again, _, _ = run(lib, inp, ws, slots)
    assert_same_bits(out, again)


def test_nothing_written_for_an_empty_batch(lib):
    out, _, _ = run(lib, dc.build('select_n0'))
    assert (out['n'] == 0).all()                                # (check_rows: every other word is still the sentinel)


def test_refusals_write_nothing(lib):
    inp = dc.build('select_n1')
    B, C, H, W = inp['heat'].shape
    ws, slots = Workspace(lib, (B, C, H, W)), Slots(B, 256)
    d = [dev(inp[k]) for k in ('heat', 'offs', 'moff')]
    h, o, m = (t.data_ptr() for t in d)

    def call(heat=h, offs=o, moff=m, topk=100, wsp=ws.ptr):
        return lib.rtm3d_decode2d(stream(), heat, offs, moff, B, C, H, W, 0.4, topk, 4.0, wsp, *slots.ptrs())
    assert call(topk=0) != 0 and call(topk=257) != 0 and call(topk=-1) != 0
    assert call(heat=None) != 0 and call(wsp=None) != 0
    assert call(offs=None) != 0 and call(moff=None) != 0       # one regression map alone is neither mode
    fin = [slots.a[k].ptr for k in ('n', 'mproj', 'verts', 'bbox')]
    assert lib.rtm3d_decode2d_finish(stream(), B, 256, None, o, m, 4.0, *fin[1:]) != 0
    assert lib.rtm3d_decode2d_finish(stream(), B, 256, fin[0], None, m, 4.0, *fin[1:]) != 0
    assert lib.rtm3d_decode2d_finish(stream(), B, 0, fin[0], o, m, 4.0, *fin[1:]) != 0
    out = slots.read()
    ws.check()
    assert is_sentinel(out['n'], 'n').all()
    for k in FIELDS:
        assert is_sentinel(out[k], k).all(), k


def test_workspace_reuse_by_a_sparser_image(lib):
    dense, sparse = dc.build('select_3000_topk256'), dc.build('reuse_sparse')
    assert dense['heat'].shape == sparse['heat'].shape and dense['topk'] == sparse['topk']
    _, slots, ws = run(lib, dense)
    reused, _, _ = run(lib, sparse, ws, slots)
    fresh, _, _ = run(lib, sparse)
    assert_same_bits(reused, fresh)
    assert_slots_equal(reused, reference('reuse_sparse'))


# ---------------------------------------------------------------------------------------------------- peaks only + finish
@pytest.mark.parametrize('name', dc.FINISH_CASES)
def test_peaks_only_then_finish(lib, name):
    inp = dc.build(name)
    (B, _, H, W), topk = inp['heat'].shape, inp['topk']
    dense, _, _ = run(lib, inp)
    peaks, slots, _ = run(lib, inp, peaks_only=True)
    ref = reference(name)
    np.testing.assert_array_equal(peaks['n'], ref['n'])
    for b, n in enumerate(ref['n']):
        np.testing.assert_array_equal(peaks['cls'][b, :n], ref['cls'][b, :n])
        np.testing.assert_array_equal(R.bits(peaks['score'][b, :n]), R.bits(ref['score'][b, :n]))
        flat = R.candidates(inp['heat'][b], inp['thresh'])[1][:n]                    # contract order: the reference's, ties or not
        np.testing.assert_array_equal(flat // (H * W), ref['cls'][b, :n])
        np.testing.assert_array_equal(peaks['mproj'][b, :n], np.stack([flat % W, flat % (H * W) // W], -1))       # the integer peak
    ro, rm = R.gather_at_peaks(inp, peaks)
    dro, drm = dev(ro), dev(rm)
    rc = lib.rtm3d_decode2d_finish(stream(), B, topk, slots.a['n'].ptr, dro.data_ptr(), drm.data_ptr(), inp['down'],
                                   slots.a['mproj'].ptr, slots.a['verts'].ptr, slots.a['bbox'].ptr)
    assert rc == 0, lib.rtm3d_last_error()
    out = slots.read()
    check_rows(out)                                             # rows at or above n are untouched by both calls
    assert_same_bits(out, dense)
    assert_slots_equal(out, ref)


# ------------------------------------------------------------------------------------------------------------------- SMOKE
def test_decode_smoke_alone(lib):
    """rtm3d_decode_smoke on its own against oracle/smoke_ref.decode's formulas (tests/decode2d_ref.smoke, pinned to it in
    test_decode2d_cpu.py): a class id below 0 and one above the table (clamped), cos of each sign, ry beyond +pi and beyond -pi
    (wrapped), a peak in the last row and column, an empty image (status -1; x, fun and nit stay the sentinel)."""
    B, topk, H, W, ncls, down = 2, 8, 6, 16, 3, 4.0
    rng = np.random.Generator(np.random.PCG64(17))
    reg = (rng.standard_normal((B, 8, H, W)) * 0.3).astype(np.float32)
    n = np.array([5, 0], np.int32)
    cls = np.zeros((B, topk), np.int64)
    cls[0, :5] = [-3, 0, 1, 2, 7]
    peak = np.zeros((B, topk, 2), np.float32)
    peak[0, :5] = [(3, 2), (15, 5), (0, 1), (7, 3), (12, 4)]              # (x, y); row 1 is the last row and column
    reg[0, 6:8, 5, 15] = (-1.0, -0.01)                                     # cos < 0, alpha just below +pi, X > 0: ry beyond +pi
    reg[0, 6:8, 1, 0] = (-1.0, 0.01)                                       # cos > 0, alpha just above -pi, X < 0: ry beyond -pi
    reg[0, 6:8, 2, 3] = (0.5, 0.8)
    reg[0, 6:8, 3, 7] = (0.5, -0.8)
    K = np.tile(np.array([100.0, 0, 10.0, 0, 110.0, 8.0, 0, 0, 1]), (B, 1))
    dim_ref = np.array([[1.5, 1.6, 3.9], [1.7, 0.6, 0.8], [1.7, 0.6, 1.8]])
    want, raw, cosv = R.smoke(cls[0, :5], peak[0, :5, 0].astype(int), peak[0, :5, 1].astype(int), reg[0], K[0], dim_ref, down)
    assert raw[1] > np.pi and raw[2] < -np.pi and (np.abs(raw[[0, 3, 4]]) < np.pi).all(), raw
    assert (cosv > 0).any() and (cosv < 0).any()
    xs, fs = np.float64(-1234.5), np.float64(-1234.5)
    gx, gf = Guarded((B, topk, 8), xs), Guarded((B, topk), fs)
    gn, gs = Guarded((B, topk), np.int32(-77)), Guarded((B, topk), np.int32(-77))
    d = [dev(a) for a in (n, cls, peak, reg, K, dim_ref)]
    rc = lib.rtm3d_decode_smoke(stream(), B, topk, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), H, W, down,
                                d[4].data_ptr(), d[5].data_ptr(), ncls, gx.ptr, gf.ptr, gn.ptr, gs.ptr)
    assert rc == 0, lib.rtm3d_last_error()
    torch.cuda.synchronize()
    x, f, nit, st = gx.read(), gf.read(), gn.read(), gs.read()
    print('smoke decode: max |x - ref|', np.abs(x[0, :5] - want).max())
    np.testing.assert_allclose(x[0, :5], want, rtol=1e-9, atol=1e-9)
    assert (f[0, :5] == 0).all() and (nit[0, :5] == 0).all() and (st[0, :5] == 0).all()
    assert (st[0, 5:] == -1).all() and (st[1] == -1).all()
    for a, s in ((x[0, 5:], xs), (x[1], xs), (f[0, 5:], fs), (f[1], fs)):
        assert (a == s).all()
    assert (nit[0, 5:] == -77).all() and (nit[1] == -77).all()
    assert lib.rtm3d_decode_smoke(stream(), B, topk, None, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), H, W, down,
                                  d[4].data_ptr(), d[5].data_ptr(), ncls, gx.ptr, gf.ptr, gn.ptr, gs.ptr) != 0
