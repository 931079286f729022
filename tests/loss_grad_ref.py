"""Plain numpy restatement of the loss-gradient rule (include/rtm3d_hip.h, "loss gradient"): the gradient of the total loss with
respect to the four logit maps, fp32 operation by operation in the order the header fixes.  ``f64=True`` runs the same code in
double (the targets stay the fp32 values the rule names): the distance between the two runs is the precision of the rule
itself on a case.  Written from the rule, not from the kernels: one object and one vertex at a time where the order matters."""
import numpy as np

from tests import loss_ref as ref

F32 = np.float32


def _pow(v, e, sq, four=False):
    if sq:                                                   # alpha = 2 and beta = 4: products
        s = v * v
        return s * s if four else s
    with np.errstate(all='ignore'):
        return np.power(v, v.dtype.type(e))


def _pow1(v, e, sq):
    if sq:
        return v
    with np.errstate(all='ignore'):
        return np.power(v, v.dtype.type(F32(e) - F32(1)))


def _sigmoid(x):
    one = x.dtype.type(1)
    with np.errstate(all='ignore'):
        return one / (one + np.exp(-x))


def _sigmoid_cr(x, dt):
    """The sigmoid of the regression logits: through fp64, rounded to the working type once."""
    with np.errstate(all='ignore'):
        return dt(1.0 / (1.0 + np.exp(-np.float64(x))))


def _sign(d):
    """1, -1, +0; a NaN stays a NaN."""
    dt = type(d)
    return dt(1) if d > 0 else (dt(-1) if d < 0 else (dt(0) if d == d else d))


def heat_grad(hm_logits, m_hm, num_pos, alpha, beta, w_mkf, u, dt):
    sq = float(alpha) == 2.0 and float(beta) == 4.0
    x, t = np.asarray(hm_logits, F32).astype(dt), np.asarray(m_hm, F32).astype(dt)
    a = dt(F32(alpha))
    with np.errstate(all='ignore'):
        s = _sigmoid(x)
        lo, hi = dt(F32(1e-4)) if dt is F32 else dt(1e-4), dt(F32(0.9999)) if dt is F32 else dt(0.9999)
        p = np.where(s < lo, lo, np.where(s > hi, hi, s)).astype(dt)          # a NaN stays
        inside = (s >= lo) & (s <= hi)
        q = dt(1) - p
        dp_pos = _pow(q, alpha, sq) / p - (a * _pow1(q, alpha, sq)) * np.log(p)
        dp_neg = (-_pow(p, alpha, sq) / q + (a * _pow1(p, alpha, sq)) * np.log(q)) * _pow(dt(1) - t, beta, sq, True)
        dp = np.where(t == dt(1), dp_pos, dp_neg).astype(dt)
        k = -((dt(u) * dt(F32(w_mkf))) / dt(max(int(num_pos), 1)))
        g = (k * np.where(inside, dp, dt(0))) * (s * (dt(1) - s))
    return g.astype(dt)


def grad(tab, img_start, B, C, H, W, logits, counts, alpha=2.0, beta=4.0, weights=(1.0, 1.0, 0.5, 0.5), upstream=None, f64=False,
         contributions=None, m_hm=None):
    """-> the four gradient maps of rtm3d_loss_grad (fp32, or double with f64).  counts: the forward's (loss_ref.loss).
    contributions: an optional dict that receives, per map name and element index, the number of contributions added.  m_hm: the
    target map where the caller has it already (loss_ref.heatmap)."""
    dt = np.float64 if f64 else F32
    hm_l, vc_l, mo_l, vo_l = [np.asarray(a, F32) for a in logits]
    u = dt(F32(1.0 if upstream is None else upstream))
    w = [dt(F32(x)) for x in weights]
    g_hm = heat_grad(hm_l, ref.heatmap(tab, img_start, B, C, H, W) if m_hm is None else m_hm, counts[0], alpha, beta, weights[0], u, dt)
    g_vc, g_mo, g_vo = np.zeros((B, 16, H, W), dt), np.zeros((B, 2, H, W), dt), np.zeros((B, 2, H, W), dt)
    with np.errstate(all='ignore'):
        k_vc = (u * w[1]) / (dt(2) * dt(int(counts[1])))
        k_vo = (u * w[3]) / (dt(2) * dt(int(counts[2])))
        k_mo = (u * w[2]) / (dt(2) * dt(int(counts[3])))

        def add(name, g, idx, c):
            g[idx] = dt(g[idx] + c)
            if contributions is not None:
                contributions.setdefault(name, {})
                contributions[name][idx] = contributions[name].get(idx, 0) + 1

        for t in tab:                                        # rising object order
            if t[2] == 0 or t[3] != 0:
                continue
            mx, my, b = t[8], t[9], int(t[0])
            if not (0 <= mx < W and 0 <= my < H):
                continue                                     # n_outside
            mx, my = int(mx), int(my)
            for e in range(2):
                s = _sigmoid_cr(mo_l[b, e, my, mx], dt)
                add('m_off', g_mo, (b, e, my, mx), (_sign(dt(s - dt(F32(t[10 + e])))) * (s * (dt(1) - s))) * k_mo)
            if t[4] == 0:
                continue
            for v in range(8):                               # rising vertex order
                if t[80 + v] == 0:
                    continue
                vx, vy = int(t[32 + 2 * v]), int(t[33 + 2 * v])
                for e in range(2):
                    x = dt(vc_l[b, 2 * v + e, my, mx])
                    add('ver_coor', g_vc, (b, 2 * v + e, my, mx), _sign(dt(x - dt(F32(t[64 + 2 * v + e])))) * k_vc)
                    s = _sigmoid_cr(vo_l[b, e, vy, vx], dt)
                    add('v_off', g_vo, (b, e, vy, vx), (_sign(dt(s - dt(F32(t[48 + 2 * v + e])))) * (s * (dt(1) - s))) * k_vo)
    return [g_hm, g_vc, g_mo, g_vo]


def main_item(hm_logits, m_hm, alpha=2.0, beta=4.0, w_mkf=1.0):
    """The forward's main item (W_MKF * main) of heat-map logits against the target m_hm, for the descent check."""
    pos, neg, npos = ref.focal(hm_logits, m_hm, alpha, beta)
    return float(F32(-neg if npos == 0 else -(pos + neg) / npos) * F32(w_mkf))
