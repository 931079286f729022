"""The yardstick of the tracking evaluation, written from include/rtm3d_hip.h ("tracking evaluation") alone: plain loops over
numpy arrays and scipy.optimize.linear_sum_assignment for ASSIGN.  It takes the arrays the device takes - sim (F, cap_g, cap_t),
ng, nt (F,), gid (F, cap_g), tid (F, cap_t) dense per sequence, seq_start (S + 1,) - and returns the arrays the device returns,
plus the MARGIN of the inputs: how far they are from a decision two correct implementations could take differently.
  * per ASSIGN: for every matched pair, forbid it, solve again, take the smallest drop of the optimum (0 when a second matching
    attains it);
  * the smallest distance of any valid sim from any alpha_a, from the CLEAR threshold and from 0.5.
Generated cases assert margin >= 1e-6 on these numbers before anything is compared."""
import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = 2.220446049250313e-16
N_ALPHA = 19
ALPHAS = [0.05 + a * 0.05 for a in range(N_ALPHA)]
DISTRACTOR = {'car': 'van', 'pedestrian': 'person_sitting'}


# ---------------------------------------------------------------------------------------------------------------- ASSIGN
def _solve(w):
    """w (n, m) >= 0, candidates w > 0 -> (col (n,), total): real columns cost -w (inf where no candidate), then one private
    zero-cost column per row."""
    n, m = w.shape
    C = np.full((n, m + n), np.inf)
    C[:, :m] = np.where(w > 0, -w, np.inf)
    C[np.arange(n), m + np.arange(n)] = 0.0
    r, c = linear_sum_assignment(C)
    col = np.full(n, -1, np.int64)
    col[r] = np.where(c < m, c, -1)
    return col, float(sum(w[i, col[i]] for i in range(n) if col[i] >= 0))


def assign(w, with_margin=True):
    """ASSIGN of one frame: (match (n,) tracker slot or -1, total, uniqueness margin)."""
    w = np.asarray(w, np.float64)
    n, m = w.shape
    if n == 0 or m == 0:
        return np.full(n, -1, np.int64), 0.0, np.inf
    col, total = _solve(w)
    margin = np.inf
    if with_margin:
        for i in np.flatnonzero(col >= 0):
            w2 = w.copy()
            w2[i, col[i]] = 0.0
            margin = min(margin, total - _solve(w2)[1])
    return col, total, margin


def sim_margin(sim, ng, nt, values):
    """The smallest distance of any valid entry of sim from any of ``values``."""
    out = np.inf
    for f in range(len(ng)):
        s = sim[f, :ng[f], :nt[f]]
        if s.size:
            out = min(out, min(float(np.abs(s - v).min()) for v in values))
    return out


# ------------------------------------------------------------------------------------------------------------------ HOTA
def hota(sim, ng, nt, gid, tid, seq_start, with_margin=True):
    sim = np.asarray(sim, np.float64)
    F, cap_g, cap_t = sim.shape
    S = len(seq_start) - 1
    n_gid = max(max([int(gid[f, :ng[f]].max(initial=-1)) for f in range(F)], default=-1) + 1, 1)
    n_tid = max(max([int(tid[f, :nt[f]].max(initial=-1)) for f in range(F)], default=-1) + 1, 1)
    potential = np.zeros((S, n_gid, n_tid))
    gcount, tcount = np.zeros((S, n_gid), np.int32), np.zeros((S, n_tid), np.int32)
    match = np.full((F, cap_g), -1, np.int32)
    tp, fn, fp = (np.zeros((S, N_ALPHA), np.int32) for _ in range(3))
    loc = np.zeros((S, N_ALPHA))
    mc = np.zeros((S, N_ALPHA, n_gid, n_tid), np.int32)
    margin = np.inf
    for s in range(S):
        frames = range(int(seq_start[s]), int(seq_start[s + 1]))
        for f in frames:                                                   # 1 alignment
            n, m = int(ng[f]), int(nt[f])
            rowsum, colsum = [0.0] * n, [0.0] * m
            for g in range(n):
                for t in range(m):
                    rowsum[g] = rowsum[g] + sim[f, g, t]
            for t in range(m):
                for g in range(n):
                    colsum[t] = colsum[t] + sim[f, g, t]
            for g in range(n):
                gcount[s, gid[f, g]] += 1
                for t in range(m):
                    den = (rowsum[g] + colsum[t]) - sim[f, g, t]
                    potential[s, gid[f, g], tid[f, t]] += sim[f, g, t] / den if den > 0 else 0.0
            for t in range(m):
                tcount[s, tid[f, t]] += 1
        den = (gcount[s][:, None] + tcount[s][None, :]).astype(np.float64) - potential[s]     # 2
        A = np.where(den > 0, potential[s] / np.where(den > 0, den, 1.0), 0.0)
        for f in frames:                                                   # 3 - 5
            n, m = int(ng[f]), int(nt[f])
            w = A[gid[f, :n]][:, tid[f, :m]] * sim[f, :n, :m]
            col, _, mg = assign(w, with_margin)
            margin = min(margin, mg)
            match[f, :n] = col
            for a in range(N_ALPHA):
                counted = 0
                for g in range(n):
                    if col[g] >= 0 and sim[f, g, col[g]] >= ALPHAS[a] - EPS:
                        counted += 1
                        loc[s, a] = loc[s, a] + sim[f, g, col[g]]
                        mc[s, a, gid[f, g], tid[f, col[g]]] += 1
                tp[s, a] += counted
                fn[s, a] += n - counted
                fp[s, a] += m - counted
    margin = min(margin, sim_margin(sim, ng, nt, ALPHAS))
    return dict(potential=potential, gcount=gcount, tcount=tcount, match=match, tp=tp, fn=fn, fp=fp, loc=loc, mc=mc, margin=margin)


def hota_metrics(o):
    """Closing formulas per alpha over all sequences -> {name: (19,)}."""
    S = o['tp'].shape[0]
    out = {k: np.zeros(N_ALPHA) for k in ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')}
    for a in range(N_ALPHA):
        TP, FN, FP = (float(sum(int(o[k][s, a]) for s in range(S))) for k in ('tp', 'fn', 'fp'))
        assa = assre = asspr = 0.0
        for s in range(S):
            m = o['mc'][s, a].astype(np.float64)
            g, t = o['gcount'][s].astype(np.float64)[:, None], o['tcount'][s].astype(np.float64)[None, :]
            assa += float((m * (m / np.maximum(1.0, (g + t) - m))).sum())
            assre += float((m * (m / np.maximum(1.0, g))).sum())
            asspr += float((m * (m / np.maximum(1.0, t))).sum())
        out['DetA'][a] = TP / max(1.0, TP + FN + FP)
        out['DetRe'][a] = TP / max(1.0, TP + FN)
        out['DetPr'][a] = TP / max(1.0, TP + FP)
        out['AssA'][a], out['AssRe'][a], out['AssPr'][a] = assa / max(1.0, TP), assre / max(1.0, TP), asspr / max(1.0, TP)
        out['LocA'][a] = float(o['loc'][:, a].sum()) / max(1.0, TP) if TP > 0 else 1.0
        out['HOTA'][a] = np.sqrt(out['DetA'][a] * out['AssA'][a])
    return out


# ----------------------------------------------------------------------------------------------------------------- CLEAR
def clear(sim, ng, nt, gid, tid, seq_start, thr=0.5, with_margin=True):
    sim = np.asarray(sim, np.float64)
    F, cap_g, cap_t = sim.shape
    S = len(seq_start) - 1
    n_gid = max(max([int(gid[f, :ng[f]].max(initial=-1)) for f in range(F)], default=-1) + 1, 1)
    match = np.full((F, cap_g), -1, np.int32)
    counts = np.zeros((S, 4), np.int32)
    simsum = np.zeros(S)
    idcount, matched, frag = (np.zeros((S, n_gid), np.int32) for _ in range(3))
    margin = np.inf
    for s in range(S):
        last, prev = {}, {}
        for f in range(int(seq_start[s]), int(seq_start[s + 1])):
            n, m = int(ng[f]), int(nt[f])
            if n == 0:
                counts[s, 2] += m
                continue
            if m == 0:
                counts[s, 1] += n
                for g in range(n):
                    idcount[s, gid[f, g]] += 1
                continue
            w = np.zeros((n, m))
            for g in range(n):
                for t in range(m):
                    if not sim[f, g, t] < thr - EPS:
                        w[g, t] = (1000.0 if prev.get(int(gid[f, g])) == int(tid[f, t]) else 0.0) + sim[f, g, t]
            col, _, mg = assign(w, with_margin)
            margin = min(margin, mg)
            match[f, :n] = col
            new_prev = {}
            for g in range(n):
                i = int(gid[f, g])
                idcount[s, i] += 1
                if col[g] < 0:
                    continue
                t = int(tid[f, col[g]])
                matched[s, i] += 1
                if i in last and last[i] != t:
                    counts[s, 3] += 1
                if i not in prev:
                    frag[s, i] += 1
                last[i] = t
                new_prev[i] = t
                simsum[s] = simsum[s] + sim[f, g, col[g]]
            k = int((col >= 0).sum())
            counts[s, 0] += k
            counts[s, 1] += n - k
            counts[s, 2] += m - k
            prev = new_prev
    margin = min(margin, sim_margin(sim, ng, nt, [thr]))
    return dict(clear_match=match, counts=counts, simsum=simsum, idcount=idcount, matched=matched, frag=frag, margin=margin)


def clear_metrics(o):
    TP, FN, FP, IDSW = (int(o['counts'][:, k].sum()) for k in range(4))
    MT = PT = ML = Frag = 0
    for s in range(o['idcount'].shape[0]):
        for i in range(o['idcount'].shape[1]):
            if o['idcount'][s, i] > 0:
                ratio = o['matched'][s, i] / o['idcount'][s, i]
                if ratio > 0.8:
                    MT += 1
                elif ratio >= 0.2:
                    PT += 1
                else:
                    ML += 1
            if o['frag'][s, i] > 0:
                Frag += int(o['frag'][s, i]) - 1
    return {'MOTA': (TP - FP - IDSW) / max(1, TP + FN), 'MOTP': float(o['simsum'].sum()) / max(1, TP), 'Recall': TP / max(1, TP + FN),
            'Precision': TP / max(1, TP + FP), 'MT': MT, 'PT': PT, 'ML': ML, 'Frag': Frag, 'IDSW': IDSW, 'TP': TP, 'FN': FN, 'FP': FP}


# ---------------------------------------------------------------------------------------------------- KITTI preprocessing
def rect_share(a, b):
    """intersection / area of a, of two rectangles x1 y1 x2 y2 (rtm3d_rect_overlaps, criterion 1)."""
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    sa = (a[2] - a[0]) * (a[3] - a[1])
    return 0.0 if w <= 0 or h <= 0 or sa == 0 else (w * h) / sa


def preprocess_frame(cls, gt, trk, sim):
    """One frame.  gt: [(type, truncation, occlusion, rect)] in file order, DontCare rows included; trk: [(type, rect)]; sim[i][j]:
    the similarity of the i-th ground truth that is NOT DontCare and the j-th tracker box of type cls (both in file order).
    Returns (kept ground truths, kept tracker boxes) as indices into gt / trk, and the margin of the decision."""
    name = cls.lower()
    rows = [i for i, g in enumerate(gt) if g[0].lower() != 'dontcare']
    cols = [j for j, t in enumerate(trk) if t[0].lower() == name]
    dontcare = [g[3] for g in gt if g[0].lower() == 'dontcare']
    sim = np.asarray(sim, np.float64).reshape(len(rows), len(cols))
    col, _, margin = assign(np.where(sim >= 0.5 - EPS, sim, 0.0))
    if sim.size:
        margin = min(margin, float(np.abs(sim - 0.5).min()))
    hard = [gt[i][2] > 2 or gt[i][1] > 0 for i in rows]
    removed, is_matched = set(), set()
    for r, i in enumerate(rows):
        if col[r] < 0:
            continue
        is_matched.add(int(col[r]))
        t = gt[i][0].lower()
        if t == DISTRACTOR.get(name) or (t == name and hard[r]):
            removed.add(int(col[r]))
    for c, j in enumerate(cols):
        if c not in is_matched:
            share = [rect_share(trk[j][1], d) for d in dontcare]
            if share:
                margin = min(margin, min(abs(v - 0.5) for v in share))
            if any(v > 0.5 for v in share):
                removed.add(c)
    keep_g = [i for r, i in enumerate(rows) if gt[i][0].lower() == name and not hard[r]]
    keep_t = [j for c, j in enumerate(cols) if c not in removed]
    return keep_g, keep_t, margin
