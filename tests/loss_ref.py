"""Plain numpy restatement of the validation-loss rule (include/rtm3d_hip.h, "validation loss"): the per-object table in fp64
operation by operation (what csrc/loss.hip computes without contraction, so the two agree bit for bit), the heat-map target,
and the loss with fp32 element terms and fp64 sums.  Written from the rule, not from the kernels: one object and one cell at a
time where the order matters."""
import numpy as np

ROW, TABLE = 18, 88
F32 = np.float32


def _corner(xs, k, sn, cs, c):
    """csrc/box_project.h box_project_corner, operation by operation."""
    dx, dy, dz = xs[2] / 2, xs[3] / 2, xs[4] / 2
    sx = -1.0 if c & 4 else 1.0
    sy = -1.0 if c & 2 else 1.0
    sz = -1.0 if c & 1 else 1.0
    X = (cs * dx) * sx + (sn * dz) * sz + xs[5]
    Y = dy * sy + xs[6]
    Z = (-sn * dx) * sx + (cs * dz) * sz + xs[7]
    pu = k[0] * X + k[1] * Y + k[2] * Z
    pv = k[3] * X + k[4] * Y + k[5] * Z
    pw = k[6] * X + k[7] * Y + k[8] * Z
    with np.errstate(all='ignore'):
        return pu / (pw + 1e-6), pv / (pw + 1e-6), Z


def radius(x1, y1, x2, y2):
    """_compute_gaussian_radius / dynamic_radius on one box (already divided by DOWN_SAMPLE): r, sigma, R, inv."""
    mo = 0.7
    hh, ww = np.ceil(y2 - y1), np.ceil(x2 - x1)
    b1 = hh + ww
    c1 = ww * hh * (1 - mo) / (1 + mo)
    r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (hh + ww)
    c2 = (1 - mo) * ww * hh
    r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * mo
    b3 = -2 * mo * (hh + ww)
    c3 = (mo - 1) * ww * hh
    r3 = (b3 + np.sqrt(b3 * b3 - (4 * a3) * c3)) / 2
    r = min(r1, r2, r3)
    sigma = (2 * r + 1) / 6
    return r, sigma, np.ceil(r), 1.0 / (2 * (sigma * sigma))


def object_table(rows, K, B, H, W, ds=4.0):
    """rows (N, 18), K (B, 9) -> the table (N, 88) of rtm3d_loss_objects."""
    rows = np.asarray(rows, np.float64)
    N = len(rows)
    tab = np.zeros((N, TABLE))
    for i in range(N):
        o = [np.float64(v) for v in rows[i]]
        t = tab[i]
        img, cls = int(o[0]), int(o[1])
        x1, y1, x2, y2 = o[3] / ds, o[4] / ds, o[5] / ds, o[6] / ds
        cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
        mx, my = np.trunc(cx), np.trunc(cy)
        t[0], t[1], t[2], t[3] = img, cls, float(cls >= 0), float(o[2] != 0)
        t[5] = float(0 <= mx < W and 0 <= my < H)
        t[6], t[7], t[8], t[9], t[10], t[11] = cx, cy, mx, my, cx - mx, cy - my
        t[12], t[13], t[14], t[15] = radius(x1, y1, x2, y2)
        k = [np.float64(K[img][e]) / ds if e < 6 else np.float64(K[img][e]) for e in range(9)]
        sn, cs = o[14], o[15]
        sn = np.float64(0.0) if abs(sn) < 1e-3 else sn
        cs = np.float64(0.0) if abs(cs) < 1e-3 else cs
        xs = [sn, cs, o[9], o[7], o[8], o[10], o[11] - o[7] / 2, o[12]]
        front = True
        for c in range(8):
            u, v, Z = _corner(xs, k, sn, cs, c)
            front = front and bool(Z > 0)
            pu, pv = np.trunc(u), np.trunc(v)
            t[16 + 2 * c], t[17 + 2 * c] = u, v
            t[32 + 2 * c], t[33 + 2 * c] = pu, pv
            t[48 + 2 * c], t[49 + 2 * c] = u - pu, v - pv
            t[64 + 2 * c], t[65 + 2 * c] = u - cx, v - cy
            t[80 + c] = float(0 <= pu < W and 0 <= pv < H)
        t[4] = float(front) if o[16] < 0 else float(o[16] != 0)
    return tab


def heatmap64(tab, img_start, B, C, H, W):
    """m_hm before its one rounding to fp32: (B, C, H, W) float64."""
    hm = np.zeros((B, C, H, W))
    ys, xs = np.mgrid[0:H, 0:W]
    for b in range(B):
        for i in range(int(img_start[b]), int(img_start[b + 1])):
            t = tab[i]
            if t[2] == 0:
                continue
            mx, my, R, inv, c = int(t[8]), int(t[9]), int(t[14]), t[15], int(t[1])
            dx, dy = (xs - mx).astype(np.float64), (ys - my).astype(np.float64)
            g = np.exp(-(dx * dx + dy * dy) * inv)
            if t[3] != 0:
                g[(dx == 0) & (dy == 0)] = 0.9999
            cover = (np.abs(dx) <= R) & (np.abs(dy) <= R)
            hm[b, c] = np.where(cover, np.maximum(hm[b, c], g), hm[b, c])
    return hm


def heatmap(tab, img_start, B, C, H, W):
    return heatmap64(tab, img_start, B, C, H, W).astype(F32)


def sigmoid32(x):
    x = np.asarray(x, F32)
    with np.errstate(all='ignore'):
        return (F32(1) / (F32(1) + np.exp(-x))).astype(F32)


def _pow32(v, e, four):
    if four is not None:                                    # alpha = 2 and beta = 4: squares
        s = v * v
        return s * s if four else s
    with np.errstate(all='ignore'):
        return np.power(v, F32(e)).astype(F32)


def focal(hm_logits, m_hm, alpha=2.0, beta=4.0):
    """-> (pos, neg, num_pos): fp32 element terms, fp64 sums."""
    sq = float(alpha) == 2.0 and float(beta) == 4.0
    x, t = np.asarray(hm_logits, F32), np.asarray(m_hm, F32)
    p = sigmoid32(x)
    p = np.where(p < F32(1e-4), F32(1e-4), np.where(p > F32(0.9999), F32(0.9999), p)).astype(F32)      # a NaN stays
    with np.errstate(all='ignore'):
        pos_t = (np.log(p) * _pow32(F32(1) - p, alpha, False if sq else None)).astype(F32)
        neg_t = ((np.log(F32(1) - p) * _pow32(p, alpha, False if sq else None)) * _pow32(F32(1) - t, beta, True if sq else None)).astype(F32)
    is_pos = t == F32(1)
    return float(pos_t[is_pos].astype(np.float64).sum()), float(neg_t[~is_pos].astype(np.float64).sum()), int(is_pos.sum())


def loss(tab, img_start, B, C, H, W, logits, alpha=2.0, beta=4.0, weights=(1.0, 1.0, 0.5, 0.5)):
    """-> (items (5,) fp32, counts (5,) int32) of rtm3d_loss_eval."""
    hm_l, vc_l, mo_l, vo_l = [np.asarray(a, F32) for a in logits]
    pos, neg, npos = focal(hm_l, heatmap(tab, img_start, B, C, H, W), alpha, beta)
    with np.errstate(all='ignore'):
        main = -neg if npos == 0 else -(pos + neg) / npos
        s_vc = s_vo = s_mo = 0.0
        n_v = n_m = n_out = 0
        for t in tab:
            if t[2] == 0 or t[3] != 0:
                continue
            mx, my, b = t[8], t[9], int(t[0])
            if not (0 <= mx < W and 0 <= my < H):
                n_out += 1
                continue
            mx, my = int(mx), int(my)
            for j in range(2):
                s_mo += float(np.abs(sigmoid32(mo_l[b, j, my, mx]) - F32(t[10 + j])))
            n_m += 1
            if t[4] == 0:
                continue
            for v in range(8):
                if t[80 + v] == 0:
                    continue
                vx, vy = int(t[32 + 2 * v]), int(t[33 + 2 * v])
                for j in range(2):
                    s_vc += float(np.abs(F32(vc_l[b, 2 * v + j, my, mx] - F32(t[64 + 2 * v + j]))))
                    s_vo += float(np.abs(sigmoid32(vo_l[b, j, vy, vx]) - F32(t[48 + 2 * v + j])))
                n_v += 1
        div = lambda s, n: np.float64(s) / np.float64(2 * n)
        w = [F32(x) for x in weights]
        items = [F32(main) * w[0], F32(div(s_vc, n_v)) * w[1], F32(div(s_mo, n_m)) * w[2], F32(div(s_vo, n_v)) * w[3]]
        total = F32(F32(F32(items[0] + items[1]) + items[2]) + items[3])
    return np.array(items + [total], F32), np.array([npos, n_v, n_v, n_m, n_out], np.int32)
