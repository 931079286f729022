"""Plain numpy restatement of the optimiser-step rule (include/rtm3d_hip.h, "optimiser step"): one numpy call per operation of
the rule, in its order, so that every operation is rounded to fp32 on its own.  ``dt=np.float64`` runs the same statements in
double with the scalars left in fp64: the distance between the two runs is the rule's own precision on a case.  Written from
the rule, not from the kernel."""
import math

import numpy as np

F32 = np.float32


def scalars(lr, wd, betas, eps, t, dt=F32):
    """The per-step scalars of one hyper class, formed in Python fp64 and rounded once: {nclr, wd, w, beta2, eps}."""
    b1, b2 = betas
    return {'nclr': dt(-(lr / (1 - b1 ** t))), 'wd': dt(wd), 'w': dt(1 - b1), 'beta2': dt(b2), 'eps': dt(eps)}


def ema_scalars(decay, n, dt=F32):
    """(d, omd) of the EMA line at update count n."""
    d = decay * (1 - math.exp(-n / 2000))
    return dt(d), dt(1.0 - d)


def update(p, g, m, u, k):
    """-> (p1, m1, u1); p, g, m, u arrays of one dtype, k = scalars(...) of the same dtype."""
    dt = p.dtype.type
    with np.errstate(all='ignore'):
        g1 = g + k['wd'] * p if k['wd'] != 0 else g
        diff = g1 - m
        if k['w'] < 0.5:
            m1 = m + k['w'] * diff
        else:
            m1 = g1 - diff * (dt(1) - k['w'])
        a = u * k['beta2']
        b = np.abs(g1) + k['eps']
        u1 = np.where((a > b) | np.isnan(a), a, b)
        p1 = p + k['nclr'] * (m1 / u1)
    for v in (p1, m1, u1):
        assert v.dtype == p.dtype
    return p1, m1, u1


def ema(e, p, d, omd):
    """-> e1 = e * d + omd * p."""
    with np.errstate(all='ignore'):
        return e * d + omd * p


def same_bits(a, b):
    """Equal bytes, except that any NaN equals any NaN (which NaN a result is, is not part of the rule)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    ia, ib = a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64)
    return bool(np.array_equal(ia[~na], ib[~na]))


def first_difference(a, b):
    """Where two arrays stop having the same bits (for a failure message)."""
    a, b = np.ravel(a), np.ravel(b)
    if a.shape != b.shape:
        return 'shapes %s / %s' % (a.shape, b.shape)
    bad = ~((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b)))
    idx = np.flatnonzero(bad)
    return 'none' if idx.size == 0 else '%d elements, first at %d: %r / %r' % (idx.size, idx[0], a[idx[0]], b[idx[0]])
