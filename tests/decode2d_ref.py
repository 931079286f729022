"""References of the 2D decode suites (tests/test_decode2d_cpu.py, tests/test_gpu_decode2d.py).  None of this is the code
under test.

- oracle(inp): oracle.rtm3d_ref.inference on the CPU, laid out like the device slots ([B] counts, [B, topk, ...] rows).  It is
  the reference of every bit-exact assertion.
- contract(inp): a NumPy restatement of the documented contract, for the cases whose scores tie: sigmoid, 3x3 equality NMS
  with a -inf border and a NaN-propagating maximum, s > thresh, order by score descending and ascending class-major flat index
  inside a tie (torch.topk's order inside a tie is arbitrary), the first topk, then the fp32 key-point arithmetic in the
  reference's operation order with NaN-propagating min / max.  It does not copy the reference's quirk that a NaN heat cell
  occupies a top-k slot before the threshold removes it.
- sig_vector / sig_scalar: the two forms torch.sigmoid takes on an fp32 CPU tensor.  Vector form: the value inside a
  zero-padded tensor shorter than 32768 elements whose length is a multiple of 32.  Scalar form: tensors shorter than 32
  elements.  sig_positional composes them by the rule of tensors below 32768 elements (the last total % 32 elements are
  scalar); sig_scalar_rounded is the scalar form with a correctly rounded expf, which torch's libm expf is not always;
  tests/test_decode2d_cpu.py asserts that it reproduces torch.sigmoid of every case tensor below that size.
- smoke(...): oracle/smoke_ref.decode's closed-form box for given peaks (fp64)."""
import numpy as np
import torch

from oracle import rtm3d_ref, smoke_ref

GRAIN, VSTEP = 32768, 32
_VCHUNK = GRAIN - VSTEP          # longest zero-padded tensor of the vector form
_SCHUNK = VSTEP - 1              # longest tensor of the scalar form


def sig_vector(x):
    x = np.ascontiguousarray(x, np.float32)
    flat, out = x.ravel(), np.empty(x.size, np.float32)
    for s in range(0, flat.size, _VCHUNK):
        c = flat[s:s + _VCHUNK]
        t = torch.zeros((len(c) + VSTEP - 1) // VSTEP * VSTEP, dtype=torch.float32)
        t[:len(c)] = torch.from_numpy(c.copy())
        out[s:s + len(c)] = torch.sigmoid(t).numpy()[:len(c)]
    return out.reshape(x.shape)


def sig_scalar(x):
    x = np.ascontiguousarray(x, np.float32)
    flat, out = x.ravel(), np.empty(x.size, np.float32)
    for s in range(0, flat.size, _SCHUNK):
        c = flat[s:s + _SCHUNK]
        out[s:s + len(c)] = torch.sigmoid(torch.from_numpy(c.copy())).numpy()
    return out.reshape(x.shape)


def sig_scalar_rounded(x):
    """The scalar form with a CORRECTLY ROUNDED expf in place of libm's: what torch does not compute.  libm's expf (error bound
    0.502 ulp) differs from it near rounding midpoints, for about one argument in 15000."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over='ignore'):
        e = np.exp(-x.astype(np.float64)).astype(np.float32)
        return (np.float32(1) / (np.float32(1) + e)).astype(np.float32)


def libm_midpoints(seed, count, lo, hi):
    """`count` seeded fp32 values in [lo, hi) whose torch scalar form is NOT the one a correctly rounded expf gives."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros(0, np.float32)
    while len(out) < count:
        c = rng.uniform(lo, hi, 1 << 18).astype(np.float32)
        out = np.unique(np.concatenate([out, c[bits(sig_scalar(c)) != bits(sig_scalar_rounded(c))]]))
    return np.random.Generator(np.random.PCG64(seed + 1)).permutation(out)[:count]


def vec_end(total):
    """First element of a `total`-element tensor below the grain that takes the scalar form."""
    assert total < GRAIN
    return total // VSTEP * VSTEP


def sig_positional(x):
    x = np.ascontiguousarray(x, np.float32)
    flat = x.ravel()
    v = vec_end(flat.size)
    return np.concatenate([sig_vector(flat[:v]), sig_scalar(flat[v:])]).reshape(x.shape)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def distinguishing(seed, count, lo, hi):
    """`count` seeded fp32 values in [lo, hi) whose two sigmoid forms differ in bits, distinct, in drawing order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    seen = set()
    while len(out) < count:
        c = rng.uniform(lo, hi, 16384).astype(np.float32)
        d = c[bits(sig_vector(c)) != bits(sig_scalar(c))]
        for v in d:
            if float(v) not in seen:
                seen.add(float(v))
                out.append(v)
    return np.array(out[:count], np.float32)


# --------------------------------------------------------------------------------------------------------------- slot layout
def empty_slots(B, topk):
    return dict(n=np.zeros(B, np.int32), cls=np.zeros((B, topk), np.int64), score=np.zeros((B, topk), np.float32),
                mproj=np.zeros((B, topk, 2), np.float32), verts=np.zeros((B, topk, 16), np.float32),
                bbox=np.zeros((B, topk, 4), np.float32))


def oracle(inp):
    """rtm3d_ref.inference in the slot layout (rows at or above n[b] are zero and mean nothing)."""
    heat, offs, moff = (torch.from_numpy(np.array(inp[k], np.float32)) for k in ('heat', 'offs', 'moff'))
    B, topk = heat.shape[0], inp['topk']
    d = rtm3d_ref.inference([heat, offs, moff, None], inp['thresh'], topk, inp['down'])
    out = empty_slots(B, topk)
    for b in range(B):
        if d[0][b] is None:
            continue
        n = len(d[0][b])
        out['n'][b] = n
        out['cls'][b, :n] = d[0][b].numpy()
        out['score'][b, :n] = d[1][b].numpy()
        out['mproj'][b, :n] = d[2][b].numpy()
        out['verts'][b, :n] = d[3][b].numpy().reshape(n, 16)
        out['bbox'][b, :n] = d[4][b].numpy()
    return out


def nms_scores(heat_b):
    """(sigmoid, survivor mask) of one image's [C, H, W] logits by the contract: torch.sigmoid of the whole tensor, s equal to
    the NaN-propagating 3x3 maximum with a -inf border.  A NaN cell is no survivor and neither is any of its neighbours."""
    s = torch.sigmoid(torch.from_numpy(np.array(heat_b, np.float32))).numpy()
    C, H, W = s.shape
    p = np.full((C, H + 2, W + 2), -np.inf, np.float32)
    p[:, 1:-1, 1:-1] = s
    mx = s.copy()
    for dy in range(3):
        for dx in range(3):
            mx = np.maximum(mx, p[:, dy:dy + H, dx:dx + W])            # np.maximum propagates NaN
    return s, mx == s


def candidates(heat_b, thresh):
    """(scores, class-major flat indices) of the survivors above the threshold, in contract order."""
    s, m = nms_scores(heat_b)
    with np.errstate(invalid='ignore'):
        m &= s > np.float32(thresh)
    flat = np.flatnonzero(m.ravel())
    sc = s.ravel()[flat]
    order = np.lexsort((flat, -sc.astype(np.float64)))
    return sc[order], flat[order]


def keypoint_rows(x, y, reg_offs, reg_moff, down):
    """The fp32 key-point arithmetic of models/model.py:48-72 for the n peaks (x, y) of one image; reg_offs [n, 16] and
    reg_moff [n, 2] are the regression logits at the peaks.  -> mproj [n, 2], verts [n, 16], bbox [n, 4]."""
    n = len(x)
    sub = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(reg_moff.T, np.float32))).numpy()       # contiguous (2, n)
    mp = np.stack([x.astype(np.float32) + sub[0], y.astype(np.float32) + sub[1]], -1)
    d = np.float32(down)
    with np.errstate(invalid='ignore'):
        vr = d * (reg_offs.reshape(n, 8, 2).astype(np.float32) + mp[:, None, :])
        bbox = np.concatenate([vr.min(1), vr.max(1)], -1)                                                # NaN-propagating
    return d * mp, vr.reshape(n, 16), bbox


def contract(inp):
    heat, offs, moff, topk = inp['heat'], inp['offs'], inp['moff'], inp['topk']
    B, C, H, W = heat.shape
    out = empty_slots(B, topk)
    for b in range(B):
        sc, flat = candidates(heat[b], inp['thresh'])
        sc, flat = sc[:topk], flat[:topk]
        n = len(sc)
        if n == 0:
            continue
        c, r = flat // (H * W), flat % (H * W)
        y, x = r // W, r % W
        mp, vr, bb = keypoint_rows(x, y, offs[b][:, y, x].T, moff[b][:, y, x].T, inp['down'])
        out['n'][b] = n
        out['cls'][b, :n], out['score'][b, :n], out['mproj'][b, :n], out['verts'][b, :n], out['bbox'][b, :n] = c, sc, mp, vr, bb
    return out


def gather_at_peaks(inp, peaks):
    """The [B, topk, 16] and [B, topk, 2] regression logits at the integer peaks a peaks-only decode returned (rows at or above
    n[b] stay zero): what the peaks-only regression heads hand to the finish kernel."""
    B, topk = inp['heat'].shape[0], inp['topk']
    ro, rm = np.zeros((B, topk, 16), np.float32), np.zeros((B, topk, 2), np.float32)
    for b in range(B):
        n = int(peaks['n'][b])
        x, y = peaks['mproj'][b, :n, 0].astype(int), peaks['mproj'][b, :n, 1].astype(int)
        ro[b, :n] = inp['offs'][b][:, y, x].T
        rm[b, :n] = inp['moff'][b][:, y, x].T
    return ro, rm


# ------------------------------------------------------------------------------------------------------------------- SMOKE
def smoke(cls, xs, ys, reg_b, K, dim_ref, down):
    """oracle/smoke_ref.decode's formulas (lines 44-55) for given peaks of one image, the class id clamped into the table as the
    kernel documents.  reg_b [8, H, W] fp32; -> ([n, 8] fp64 = [sin ry, cos ry, l, h, w, X, Y, Z], ry before
    the wrap, the cos channel)."""
    dim_ref = np.asarray(dim_ref, np.float64)
    r = reg_b[:, ys, xs].astype(np.float64)
    Kb = np.asarray(K, np.float64).reshape(9)
    z = smoke_ref.DEPTH_REF[0] + smoke_ref.DEPTH_REF[1] * r[0]
    u = down * (xs.astype(np.float64) + r[1]); v = down * (ys.astype(np.float64) + r[2])
    X = (u - Kb[2]) * z / Kb[0]; Y = (v - Kb[5]) * z / Kb[4]
    dr = dim_ref[np.clip(cls, 0, len(dim_ref) - 1)]
    h, w, l = dr[:, 0] * np.exp(r[3]), dr[:, 1] * np.exp(r[4]), dr[:, 2] * np.exp(r[5])
    alpha = np.arctan(r[6] / (r[7] + 1e-7)) + np.where(r[7] >= 0, -0.5 * np.pi, 0.5 * np.pi)
    raw = alpha + np.arctan2(X, z)
    ry = np.where(raw > np.pi, raw - 2 * np.pi, raw); ry = np.where(ry < -np.pi, ry + 2 * np.pi, ry)
    return np.stack([np.sin(ry), np.cos(ry), l, h, w, X, Y, z], 1), raw, r[7]
