"""Case table and regime mirror of the 2D decode (rtm3d_amd/csrc/decode2d.hip): every case names the regime of the launch code
it is there for (`expect`), and regime() derives the same quantities from the inputs and the reference alone.  Importable
without a GPU: tests/test_decode2d_cpu.py checks the table, tests/test_gpu_decode2d.py runs it.

The launch code, as mirrored here
- sigmoid: element i of an image's C*H*W logits takes ATen's vector form below vec_end = total // 32 * 32 and the scalar form
  from there on, for total < 32768; at or above 32768 the kernel calls every element "vector".  With total % 32 != 0 there
  torch.sigmoid itself takes scalar tails whose position depends on its thread count: the reference is not defined bit for
  bit ('defined' below is False) and the scores are only required to be one of the two forms.
- sub-pixel sigmoid: the same rule over the contiguous (2, n) gather: x of rank r is element r, y of rank r is element n + r.
- NMS + append: one lane per element, waves of 64 consecutive elements of the B*total range (blocks of 256); a wave that
  holds elements of two images takes the per-lane fallback, which matters when it has survivors on both sides.
- select: radix select over the bytes of the 64-bit key (score bits << 32 | ~flat index), most significant first, when an
  image has more candidates than topk; 1024 threads stride over the candidate list.
"""
import numpy as np
import torch

from oracle import rtm3d_ref
from tests import decode2d_ref as R

DOWN = 4.0
F32 = np.float32


# --------------------------------------------------------------------------------------------------------------- builders
def _base(B, C, H, W, seed, bg=-6.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    heat = np.full((B, C, H, W), bg, F32)
    offs = (rng.standard_normal((B, 16, H, W)) * 3).astype(F32)
    moff = (rng.standard_normal((B, 2, H, W)) * 2).astype(F32)
    return heat, offs, moff


def _inp(heat, offs, moff, thresh=0.4, topk=100):
    return dict(heat=heat, offs=offs, moff=moff, thresh=float(thresh), topk=int(topk), down=DOWN)


def _grid_cells(C, H, W, n):
    """n cells (c, y, x) on the stride-2 grid (no two adjacent), class-major."""
    cells = [(c, y, x) for c in range(C) for y in range(0, H, 2) for x in range(0, W, 2)]
    assert n <= len(cells)
    return cells[:n]


def _descending(n, hi=3.0, lo=0.0):
    return np.linspace(hi, lo, n).astype(F32) if n > 1 else np.array([hi], F32)


def _unflat(flat, H, W):
    c, r = divmod(int(flat), H * W)
    return c, r // W, r % W


def _next_score_logit(a, ulps=1):
    """The smallest fp32 logit above `a` whose vector-form sigmoid is `ulps` ulp above that of `a`."""
    c = np.full(4096, a, F32)
    for i in range(1, len(c)):
        c[i] = np.nextafter(c[i - 1], F32(np.inf))
    s = R.bits(R.sig_vector(c)).astype(np.int64)
    hit = np.flatnonzero(s == s[0] + ulps)
    assert len(hit), 'no logit found %d ulp above' % ulps
    return c[hit[0]]


def heat_tail(B, C, H, W, tail_cells, other_cells, seed, topk=100):
    """Peaks with distinguishing logits (the two sigmoid forms differ) at tail_cells / other_cells [(b, c, y, x)]."""
    def build():
        heat, offs, moff = _base(B, C, H, W, seed)
        cells = list(tail_cells) + list(other_cells)
        lg = np.sort(R.distinguishing(seed + 1000, len(cells), 0.2, 3.0))[::-1]
        order = np.random.Generator(np.random.PCG64(seed + 1)).permutation(len(cells))
        for (b, c, y, x), v in zip([cells[i] for i in order], lg):
            heat[b, c, y, x] = v
        return _inp(heat, offs, moff, topk=topk)
    return build


def sub_pixel(n):
    """n peaks of strictly descending score on a 3 x 24 x 40 map (no heat tail); every main_offset value at a peak is a
    distinguishing value, so every rank on both sides of vend tells the two forms apart, for x and for y."""
    def build():
        heat, offs, moff = _base(1, 3, 24, 40, 40 + n)
        pool = R.distinguishing(7000 + n, 2 * n, -3.0, 3.0)
        for r, ((c, y, x), v) in enumerate(zip(_grid_cells(3, 24, 40, n), _descending(n))):
            heat[0, c, y, x] = v
            moff[0, 0, y, x], moff[0, 1, y, x] = pool[2 * r], pool[2 * r + 1]
        return _inp(heat, offs, moff, topk=256 if n > 100 else 100)
    return build


def sub_values(values):
    """len(values) / 2 < 16 peaks (every sub-pixel value in a scalar position) whose main_offset x, y are `values`."""
    def build():
        n = len(values) // 2
        heat, offs, moff = _base(1, 3, 24, 40, 70 + n)
        v = values() if callable(values) else np.asarray(values, F32)
        for r, ((c, y, x), lg) in enumerate(zip(_grid_cells(3, 24, 40, n), _descending(n))):
            heat[0, c, y, x] = lg
            moff[0, 0, y, x], moff[0, 1, y, x] = v[2 * r], v[2 * r + 1]
        return _inp(heat, offs, moff)
    return build


class _Lazy:
    """A list of values computed at build time."""
    def __init__(self, n, f):
        self.n, self.f = n, f

    def __len__(self):
        return self.n

    def __call__(self):
        return self.f()


EXTREME = [88.5, -88.5, 95.0, -95.0, 103.9, -103.9, 104.5, -104.5, 87.9, -87.9, 110.0, -110.0, 89.0, -89.0, 20.0, -20.0, 17.0, -17.0]


def planted(B, C, H, W, peaks, seed=5, topk=100, thresh=0.4, bg=-6.0, edit=None):
    """peaks: [(b, c, y, x, logit)]; edit(heat, offs, moff) may poison the maps afterwards."""
    def build():
        heat, offs, moff = _base(B, C, H, W, seed, bg)
        for b, c, y, x, v in peaks:
            heat[b, c, y, x] = v
        if edit:
            edit(heat, offs, moff)
        return _inp(heat, offs, moff, thresh=thresh, topk=topk)
    return build


def n_peaks(n, topk, C=3, H=24, W=40, seed=11):
    def build():
        heat, offs, moff = _base(1, C, H, W, seed)
        for (c, y, x), v in zip(_grid_cells(C, H, W, n), _descending(n)):
            heat[0, c, y, x] = v
        return _inp(heat, offs, moff, topk=topk)
    return build


def all_equal(B, C, H, W, topk=100, value=2.0):
    def build():
        heat, offs, moff = _base(B, C, H, W, 3, bg=value)
        return _inp(heat, offs, moff, topk=topk)
    return build


def dense_random(B, C, H, W, seed, thresh, topk):
    def build():
        heat, offs, moff = _base(B, C, H, W, seed)
        rng = np.random.Generator(np.random.PCG64(seed + 7))
        heat[:] = (rng.standard_normal(heat.shape) * 1.5).astype(F32)
        return _inp(heat, offs, moff, thresh=thresh, topk=topk)
    return build


def ulp_neighbour():
    """(2, 4) at logit a; its right neighbour one fp32 ulp higher in SCORE: the neighbour suppresses it."""
    def build():
        heat, offs, moff = _base(1, 3, 8, 16, 21)
        a = F32(1.25)
        heat[0, 1, 2, 4], heat[0, 1, 2, 5] = a, _next_score_logit(a)
        heat[0, 0, 5, 9] = 0.5
        return _inp(heat, offs, moff)
    return build


def threshold_equal():
    """thresh is the float value of torch.sigmoid at logit 0.75; a peak at exactly that score, one at the next float up."""
    def build():
        heat, offs, moff = _base(1, 3, 8, 16, 22)
        t0 = F32(0.75)
        heat[0, 0, 2, 2], heat[0, 2, 5, 11] = t0, _next_score_logit(t0)
        return _inp(heat, offs, moff, thresh=float(R.sig_vector(np.array([t0]))[0]))
    return build


def score_cut(byte):
    """topk = 4 of 8 peaks on a map without a tail; the 4th and the 5th score differ first in score byte `byte`."""
    ab = {0: (0.2, -0.2), 1: (1.2, 0.5), 2: (1.0, 0.999)}

    def build():
        heat, offs, moff = _base(1, 3, 8, 16, 30 + byte)
        a, b = (F32(1.0), None) if byte == 3 else (F32(v) for v in ab[byte])
        if byte == 3:
            b, a = a, _next_score_logit(a)
        lg = [3.0, 2.5, 2.0, a, b, F32(b) - F32(0.05), F32(b) - F32(0.1), F32(b) - F32(0.15)]
        cells = _grid_cells(3, 8, 16, 8)
        for i, j in enumerate(np.random.Generator(np.random.PCG64(byte)).permutation(8)):
            c, y, x = cells[j]
            heat[0, c, y, x] = lg[i]
        return _inp(heat, offs, moff, topk=4)
    return build


def tie_cut(flats):
    """topk = 4: three higher peaks, then equal peaks at the flat indices `flats` of a 3 x 8 x 16 map: the cut falls inside the
    tie and the lower flat index wins."""
    def build():
        heat, offs, moff = _base(1, 3, 8, 16, 35)
        for (c, y, x), v in zip([(0, 0, 0), (0, 0, 4), (0, 0, 8)], (3.0, 2.5, 2.0)):
            heat[0, c, y, x] = v
        for f in flats:
            c, y, x = _unflat(f, 8, 16)
            heat[0, c, y, x] = 1.0
        return _inp(heat, offs, moff, topk=4)
    return build


def _poison_regression(heat, offs, moff):
    # peaks at (0, c, y, x) below, in score order
    offs[0, 3, 2, 2] = np.nan            # rank 0: NaN vertex offset (y of vertex 1)
    moff[0, 1, 2, 6] = np.nan            # rank 1: NaN sub-pixel y
    moff[0, 0, 2, 10] = np.nan           # rank 2: NaN sub-pixel x
    offs[0, 0, 4, 2] = np.inf            # rank 3: +Inf vertex offset
    offs[0, 5, 4, 6] = -np.inf           # rank 4: -Inf vertex offset
    moff[0, 0, 4, 10] = np.inf           # rank 5: sub-pixel sigmoid 1
    moff[0, 1, 6, 2] = -np.inf           # rank 6: sub-pixel sigmoid 0
    offs[0, 2, 6, 6], offs[0, 8, 6, 6] = np.nan, np.inf      # rank 7: NaN in x and +Inf in x of another vertex


REG_PEAKS = [(0, 1, y, x, v) for (y, x), v in zip([(2, 2), (2, 6), (2, 10), (4, 2), (4, 6), (4, 10), (6, 2), (6, 6), (6, 10)],
                                                    _descending(9, 3.0, 1.0))]


def _nan_heat(cells):
    def edit(heat, offs, moff):
        for b, c, y, x in cells:
            heat[b, c, y, x] = np.nan
    return edit


def _inf_heat(heat, offs, moff):
    heat[0, 2, 1, 1] = np.inf


def case(build, ties=False, **expect):
    return dict(build=build, ties=ties, expect=expect)


T3 = 3 * 13 * 37                                   # 1443 elements per image: 1443 % 64 == 35, tail 1440..1442
SUB_N = (1, 15, 16, 17, 31, 32, 33, 100, 256)
SUB_SCALAR = {1: (1, 1), 15: (15, 15), 16: (0, 0), 17: (0, 2), 31: (0, 30), 32: (0, 0), 33: (0, 2), 100: (0, 8), 256: (0, 0)}

CASES = {
    # ---- sigmoid position rule, heat map: kept peaks in the scalar tail whose two forms differ
    'heat_tail_3x7x9': case(heat_tail(1, 3, 7, 9, [(0, 2, y, x) for y in (4, 6) for x in (0, 2, 4, 6, 8)],
                                      [(0, 0, 1, 1), (0, 0, 3, 5), (0, 1, 2, 2), (0, 2, 1, 7)], 50),
                            total=189, vec_end=160, defined=True, n=(14,), heat_scalar_kept=10, heat_scalar_distinct=10, heat_vector_distinct=4),
    'heat_tail_2x3x13x37': case(heat_tail(2, 3, 13, 37, [(0, 2, 12, 36), (1, 2, 12, 35)],
                                          [(0, 0, 0, 0), (0, 2, 12, 33), (1, 1, 6, 20), (1, 2, 12, 32), (1, 2, 10, 35)], 51),
                                total=T3, vec_end=1440, defined=True, n=(3, 4), heat_scalar_kept=2, heat_scalar_distinct=2, heat_vector_distinct=5,
                                grid_tail=True),
    'heat_notail_3x8x16': case(heat_tail(1, 3, 8, 16, [], [(0, 2, 7, 15), (0, 2, 7, 13), (0, 2, 5, 15), (0, 0, 0, 0), (0, 1, 3, 3)], 52),
                               total=384, vec_end=384, defined=True, n=(5,), heat_scalar_kept=0, heat_vector_distinct=5, grid_tail=True),
    'heat_grain_1x128x256': case(heat_tail(1, 1, 128, 256, [], [(0, 0, 127, 255), (0, 0, 127, 253), (0, 0, 125, 255), (0, 0, 127, 230),
                                                                (0, 0, 0, 0), (0, 0, 64, 100)], 53),
                                 total=32768, vec_end=32768, defined=True, n=(6,), heat_scalar_kept=0, heat_vector_distinct=6, grid_tail=False),
    'heat_below_grain_3x104x105': case(heat_tail(1, 3, 104, 105, [(0, 2, 103, x) for x in range(82, 105, 2)],
                                                 [(0, 2, 103, 78), (0, 0, 0, 0), (0, 1, 50, 50)], 54),
                                       total=32760, vec_end=32736, defined=True, n=(15,), heat_scalar_kept=12, heat_scalar_distinct=12,
                                       heat_vector_distinct=3, scalar_not_rounded=1),
    # ---- the regime in which torch.sigmoid itself is not defined bit for bit (total >= 32768, total % 32 != 0)
    'heat_undefined_3x100x110': case(heat_tail(1, 3, 100, 110, [], [(0, 2, 99, x) for x in (102, 104, 106, 108)] +
                                               [(0, 2, 97, 109), (0, 0, 0, 0), (0, 1, 50, 55), (0, 1, 99, 109)], 55),
                                     total=33000, defined=False, n=(8,), last8_distinct=4),
    # ---- NMS geometry
    'nms_borders': case(planted(1, 2, 7, 9, [(0, 0, 0, 0, 3.0), (0, 0, 0, 8, 2.9), (0, 0, 6, 0, 2.8), (0, 0, 6, 8, 2.7),       # corners
                                             (0, 0, 0, 4, 2.6), (0, 0, 6, 4, 2.5), (0, 0, 3, 0, 2.4), (0, 0, 3, 8, 2.3),       # edges
                                             (0, 1, 3, 8, 2.2),                                   # the same cell high in two classes
                                             (0, 1, 1, 8, 2.1), (0, 1, 2, 0, 2.0),                # end of row 1, start of row 2
                                             (0, 0, 2, 4, 1.0), (0, 0, 3, 4, 1.5), (0, 0, 4, 5, 0.9)],       # suppressed by (3, 4)
                                    topk=100),
                        n=(12,), cells=[(0, 0, 0, 0), (0, 0, 0, 8), (0, 0, 6, 0), (0, 0, 6, 8), (0, 0, 0, 4), (0, 0, 6, 4), (0, 0, 3, 0),
                                        (0, 0, 3, 8), (0, 1, 3, 8), (0, 1, 1, 8), (0, 1, 2, 0), (0, 0, 3, 4)]),
    'nms_image_wrap': case(planted(2, 2, 5, 6, [(0, 1, 4, 5, 2.0), (1, 0, 0, 0, 1.5), (0, 0, 0, 0, 1.0), (1, 1, 4, 5, 0.8)], topk=60),
                           n=(2, 2), cells=[(0, 1, 4, 5), (0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 4, 5)], straddle_waves=1),
    'nms_h1': case(planted(1, 3, 1, 40, [(0, 0, 0, 0, 2.0), (0, 0, 0, 1, 1.0), (0, 1, 0, 20, 1.5), (0, 1, 0, 21, 1.4), (0, 2, 0, 39, 1.2),
                                         (0, 2, 0, 37, 0.7)], topk=100),
                   n=(4,), cells=[(0, 0, 0, 0), (0, 1, 0, 20), (0, 2, 0, 39), (0, 2, 0, 37)]),
    'nms_w1': case(planted(1, 3, 40, 1, [(0, 0, 0, 0, 2.0), (0, 0, 1, 0, 1.0), (0, 1, 20, 0, 1.5), (0, 1, 21, 0, 1.4), (0, 2, 39, 0, 1.2),
                                         (0, 2, 37, 0, 0.7)], topk=100),
                   n=(4,), cells=[(0, 0, 0, 0), (0, 1, 20, 0), (0, 2, 39, 0), (0, 2, 37, 0)]),
    'nms_1x1': case(planted(1, 3, 1, 1, [(0, 0, 0, 0, 1.0), (0, 2, 0, 0, 2.0)], topk=3), n=(2,), cells=[(0, 0, 0, 0), (0, 2, 0, 0)]),
    'nms_equal_neighbours': case(planted(1, 2, 8, 16, [(0, 0, 2, 3, 1.5), (0, 0, 2, 4, 1.5),         # horizontal plateau: both kept
                                                       (0, 1, 4, 8, 1.0), (0, 1, 5, 9, 1.0),         # diagonal plateau: both kept
                                                       (0, 1, 1, 1, 2.0)]), ties=True,
                                 n=(5,), cells=[(0, 0, 2, 3), (0, 0, 2, 4), (0, 1, 4, 8), (0, 1, 5, 9), (0, 1, 1, 1)]),
    'nms_ulp_neighbour': case(ulp_neighbour(), n=(2,), cells=[(0, 1, 2, 5), (0, 0, 5, 9)], ulp_pairs=1),
    # ---- the strict s > thresh
    'thresh_equal': case(threshold_equal(), n=(1,), cells=[(0, 2, 5, 11)], at_thresh=1, ulp_above_thresh=1),
    # ---- candidate append
    'append_straddle_b3': case(planted(3, 3, 13, 37, [(b, 2, 12, x, 2.0 + 0.1 * b + 0.01 * x) for b in range(3) for x in (36, 34, 32)] +
                                       [(b, 0, 0, x, 1.0 + 0.1 * b + 0.01 * x) for b in range(3) for x in (0, 2, 4)] +
                                       [(1, 1, 6, 6, 0.3)], topk=100),
                               total=T3, n=(6, 7, 6), straddle_waves=2, grid_tail=True),
    'append_full_wave': case(all_equal(1, 3, 8, 16), ties=True, cand=(384,), n=(100,), full_waves=6, cut_byte=(7,)),
    # ---- select: n against topk, the strided loops, topk 1 / 30 / 100 / 256
    'select_n0': case(planted(2, 3, 8, 16, [(0, 0, 3, 3, -1.0), (1, 2, 5, 5, -0.5)]), cand=(0, 0), n=(0, 0)),
    'select_n1': case(n_peaks(1, 100), cand=(1,), n=(1,)),
    'select_topk_minus1': case(n_peaks(29, 30), cand=(29,), n=(29,)),
    'select_topk': case(n_peaks(30, 30), cand=(30,), n=(30,)),
    'select_topk_plus1': case(n_peaks(31, 30), cand=(31,), n=(30,)),
    'select_topk1': case(n_peaks(5, 1), cand=(5,), n=(1,)),
    'select_3000_topk256': case(dense_random(1, 3, 96, 100, 61, 0.05, 256), n=(256,), strided=True, many=True),
    'select_3000_topk100': case(dense_random(2, 3, 96, 100, 62, 0.05, 100), n=(100, 100), strided=True, many=True),
    'reuse_sparse': case(planted(1, 3, 96, 100, [(0, 0, 10, 10, 2.0), (0, 1, 50, 50, 1.5), (0, 2, 95, 99, 1.0)], topk=256), cand=(3,), n=(3,)),
    # ---- select: the byte of the 64-bit key in which the cut between the topk-th and the next candidate falls
    'cut_score_byte0': case(score_cut(0), cand=(8,), n=(4,), cut_byte=(0,)),
    'cut_score_byte1': case(score_cut(1), cand=(8,), n=(4,), cut_byte=(1,)),
    'cut_score_byte2': case(score_cut(2), cand=(8,), n=(4,), cut_byte=(2,)),
    'cut_score_byte3': case(score_cut(3), cand=(8,), n=(4,), cut_byte=(3,)),
    'cut_tie_index_low': case(tie_cut((40, 44, 100, 200, 300)), ties=True, cand=(8,), n=(4,), cut_byte=(7,)),
    'cut_tie_index_second': case(tie_cut((250, 260, 300)), ties=True, cand=(6,), n=(4,), cut_byte=(6,)),
    'cut_tie_index_third': case(all_equal(1, 3, 96, 320), ties=True, cand=(92160,), n=(100,), active_byte5=True, strided=True),
    # ---- peaks-only + finish on a batch with an empty image
    'finish_b3_one_empty': case(planted(3, 3, 8, 16, [(0, 0, 1, 1, 2.0), (0, 1, 5, 9, 1.0), (2, 2, 7, 15, 1.5), (2, 0, 0, 0, 0.5), (2, 1, 3, 3, 2.5)]),
                                n=(2, 0, 3)),
    # ---- non-finite values
    'nf_regression': case(planted(1, 3, 8, 16, REG_PEAKS, edit=_poison_regression), n=(9,), nonfinite_rows=dict(mproj=2, verts=6, bbox=6),
                          nan_bbox_entries=8),
    'nf_nan_heat_horizontal': case(planted(1, 3, 8, 16, [(0, 1, 3, 5, 2.0), (0, 0, 6, 12, 1.0)], edit=_nan_heat([(0, 1, 3, 6)])),
                                   n=(1,), cells=[(0, 0, 6, 12)], nan_heat=1),
    'nf_nan_heat_diagonal': case(planted(1, 3, 8, 16, [(0, 1, 3, 5, 2.0), (0, 0, 6, 12, 1.0), (0, 2, 0, 0, 1.5)],
                                         edit=_nan_heat([(0, 1, 4, 6), (0, 2, 1, 1)])),
                                 n=(1,), cells=[(0, 0, 6, 12)], nan_heat=2),
    'nf_inf_heat': case(planted(1, 3, 8, 16, [(0, 1, 3, 5, 2.0), (0, 0, 6, 12, 1.0)], bg=-np.inf, edit=_inf_heat),
                        n=(3,), cells=[(0, 2, 1, 1), (0, 1, 3, 5), (0, 0, 6, 12)], score_one=1),
}
for _n in SUB_N:
    CASES['sub_n%d' % _n] = case(sub_pixel(_n), cand=(_n,), n=(_n,), sub_scalar=SUB_SCALAR[_n], sub_all_distinct=True)

# the scalar form is libm's expf, which is not always the correctly rounded one; arguments at which expf over- or underflows
CASES['sub_libm_expf'] = case(sub_values(_Lazy(18, lambda: R.libm_midpoints(90, 18, -4.0, 4.0))), cand=(9,), n=(9,), sub_scalar=(9, 9),
                              scalar_not_rounded=18)
CASES['sub_extreme'] = case(sub_values(EXTREME), cand=(9,), n=(9,), sub_scalar=(9, 9))

SUB_CASES = ['sub_n%d' % n for n in SUB_N]
FINISH_CASES = SUB_CASES + ['sub_libm_expf', 'sub_extreme', 'finish_b3_one_empty']

_built = {}


def build(name):
    """The inputs of a case (built once, never modified)."""
    if name not in _built:
        inp = CASES[name]['build']()
        for k in ('heat', 'offs', 'moff'):
            inp[k].setflags(write=False)
        _built[name] = inp
    return _built[name]


# ---------------------------------------------------------------------------------------------------------------- mirror
def _keys(sc, flat):
    return (R.bits(sc).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - flat.astype(np.uint64))


def _byte(k, i):
    return (k >> np.uint64(56 - 8 * i)) & np.uint64(255)


def reference_candidates(heat_b, thresh):
    """(scores, flat indices) of the reference's survivors above the threshold (oracle nms_hm on torch.sigmoid of the whole
    tensor), ordered by the contract."""
    hm = rtm3d_ref.nms_hm(torch.sigmoid(torch.from_numpy(np.array(heat_b, F32))).unsqueeze(0), 3).squeeze(0).numpy().ravel()
    with np.errstate(invalid='ignore'):
        flat = np.flatnonzero(hm > F32(thresh))
    sc = hm[flat]
    order = np.lexsort((flat, -sc.astype(np.float64)))
    return sc[order], flat[order]


def regime(inp):
    """The regime of a case from its inputs and the reference alone."""
    heat, topk = inp['heat'], inp['topk']
    B, C, H, W = heat.shape
    total = C * H * W
    defined = total < R.GRAIN or total % R.VSTEP == 0
    vend = R.vec_end(total) if total < R.GRAIN else total
    r = dict(total=total, vec_end=vend if defined else None, defined=defined, grid_tail=(B * total) % 256 != 0)
    cand, n, cut, ties, cells, act5 = [], [], [], False, [], False
    hs_kept = hs_dist = hv_dist = 0
    not_rounded = 0
    sub_scalar, sub_dist_ok, at_thresh, ulp_above, ulp_pairs, score_one, last8 = [0, 0], True, 0, 0, 0, 0, 0
    keep_gi = []
    min_gap = None
    for b in range(B):
        sc, flat = reference_candidates(heat[b], inp['thresh'])
        cand.append(len(sc))
        keep_gi.append(b * total + flat)
        k = min(len(sc), topk)
        n.append(k)
        top = sc[:min(len(sc), topk + 1)]
        ties = ties or len(np.unique(top)) != len(top)
        if len(sc) > 1:
            gap = np.diff(R.bits(sc[:k + 1]).astype(np.int64)).__abs__().min()
            min_gap = gap if min_gap is None else min(min_gap, gap)
        if len(sc) > topk:
            keys = _keys(sc, flat)
            d = [i for i in range(8) if _byte(keys[topk - 1], i) != _byte(keys[topk], i)]
            cut.append(d[0])
            m = np.ones(len(keys), bool)
            for i in range(8):
                if i == 5 and len(np.unique(_byte(keys[m], i))) > 1:
                    act5 = True
                m &= _byte(keys, i) == _byte(keys[topk - 1], i)
        else:
            cut.append(None)
        kf = flat[:k]
        cells += [(b,) + _unflat(f, H, W) for f in kf]
        lg = heat[b].ravel()[kf]
        differ = R.bits(R.sig_vector(lg)) != R.bits(R.sig_scalar(lg)) if k else np.zeros(0, bool)
        if defined:
            hs_kept += int((kf >= vend).sum())
            hs_dist += int((differ & (kf >= vend)).sum())
            hv_dist += int((differ & (kf < vend)).sum())
            not_rounded += int((R.bits(R.sig_scalar(lg)) != R.bits(R.sig_scalar_rounded(lg)))[kf >= vend].sum())
        last8 += int((differ & (kf >= total - 8)).sum())
        score_one += int((sc[:k] == 1.0).sum())
        # the sub-pixel sigmoid over the contiguous (2, k) gather
        ve = 2 * k // R.VSTEP * R.VSTEP
        xs, ys = np.arange(k) >= ve, k + np.arange(k) >= ve
        sub_scalar[0] += int(xs.sum()); sub_scalar[1] += int(ys.sum())
        y_, x_ = (kf % (H * W)) // W, kf % W
        mo = inp['moff'][b][:, y_, x_]
        with np.errstate(invalid='ignore'):
            sub_dist_ok = sub_dist_ok and k > 0 and bool((R.bits(R.sig_vector(mo)) != R.bits(R.sig_scalar(mo))).all())
        if k and np.isfinite(mo).all():
            not_rounded += int((R.bits(R.sig_scalar(mo)) != R.bits(R.sig_scalar_rounded(mo)))[np.stack([xs, ys])].sum())
        # the strict threshold and one-ulp neighbours, from the reference's sigmoid of the whole map
        s_all = torch.sigmoid(torch.from_numpy(np.array(heat[b], F32))).numpy()
        t = F32(inp['thresh'])
        at_thresh += int((s_all == t).sum())
        ulp_above += int((s_all == np.nextafter(t, F32(np.inf))).sum())
        sb = R.bits(s_all).astype(np.int64)
        fin = np.isfinite(s_all)
        ulp_pairs += int(((sb[:, :, 1:] - sb[:, :, :-1] == 1) & fin[:, :, 1:] & fin[:, :, :-1]).sum())
    gi = np.concatenate(keep_gi) if keep_gi else np.zeros(0, np.int64)
    straddle = full = 0
    for w in np.unique(gi // 64):
        lanes = gi[gi // 64 == w]
        imgs = np.unique(lanes // total)
        if (w * 64) // total != min(w * 64 + 63, B * total - 1) // total:
            straddle += int(len(imgs) > 1)
        elif len(lanes) == 64:
            full += 1
    o = R.oracle(inp) if defined else None
    r.update(cand=tuple(cand), n=tuple(n), cut_byte=tuple(cut), ties=bool(ties), cells=sorted(cells), active_byte5=act5,
             heat_scalar_kept=hs_kept, heat_scalar_distinct=hs_dist, heat_vector_distinct=hv_dist, last8_distinct=last8,
             sub_scalar=tuple(sub_scalar), sub_all_distinct=sub_dist_ok, at_thresh=at_thresh, ulp_above_thresh=ulp_above,
             ulp_pairs=ulp_pairs, score_one=score_one, straddle_waves=straddle, full_waves=full,
             strided=max(cand) > 1024, many=all(2500 <= c <= 3500 for c in cand), min_gap_ulps=min_gap,
             nan_heat=int(np.isnan(heat).sum()), scalar_not_rounded=not_rounded)
    if o is not None:
        rows = {k: sum(int((~np.isfinite(o[k][b, :o['n'][b]])).reshape(int(o['n'][b]), o[k].shape[-1]).any(1).sum()) for b in range(B))
                for k in ('mproj', 'verts', 'bbox')}
        r.update(nonfinite_rows=rows, nan_bbox_entries=sum(int(np.isnan(o['bbox'][b, :o['n'][b]]).sum()) for b in range(B)))
    return r


# every regime the suite promises, and the predicate a case's regime must satisfy to count for it
COVERAGE = {
    'heat: kept peak in the scalar tail, forms differ': lambda r: r['defined'] and r['heat_scalar_distinct'] > 0,
    'heat: two images with a tail each': lambda r: r['defined'] and r['heat_scalar_distinct'] > 1 and len(r['n']) > 1,
    'heat: no tail, forms differ': lambda r: r['defined'] and r['total'] < R.GRAIN and r['vec_end'] == r['total'] and r['heat_vector_distinct'] > 0,
    'heat: exactly the grain': lambda r: r['total'] == R.GRAIN and r['heat_vector_distinct'] > 0,
    'heat: tail just below the grain': lambda r: R.GRAIN - 32 < r['total'] < R.GRAIN and r['heat_scalar_distinct'] > 0,
    'heat: undefined regime': lambda r: not r['defined'] and r['last8_distinct'] > 0,
    'straddling wave with survivors on both sides': lambda r: r['straddle_waves'] > 0,
    'wave with 64 survivors': lambda r: r['full_waves'] > 0,
    'grid tail (B * total % 256 != 0)': lambda r: r['grid_tail'],
    'strided candidate loops (> 1024 candidates)': lambda r: r['strided'],
    'about 3000 candidates': lambda r: r['many'],
    'n == 0': lambda r: r['cand'] == (0,) * len(r['cand']),
    'n == 1': lambda r: r['cand'] == (1,),
    'cut inside a tie': lambda r: r['ties'] and r['cut_byte'][0] is not None and r['cut_byte'][0] >= 4,
    'third index byte decides': lambda r: r['active_byte5'],
    'score equal to the threshold': lambda r: r['at_thresh'] > 0 and r['ulp_above_thresh'] > 0,
    'neighbour one ulp higher': lambda r: r['ulp_pairs'] > 0,
    'NaN heat cell': lambda r: r['nan_heat'] > 0,
    '+Inf heat cell': lambda r: r['score_one'] > 0,
    "scalar position, libm's expf is not the correctly rounded one": lambda r: r['scalar_not_rounded'] > 0,
    'NaN in bbox': lambda r: r.get('nan_bbox_entries', 0) > 0,
}
for _b in range(8):
    COVERAGE['cut in key byte %d' % _b] = (lambda r, _b=_b: _b in r['cut_byte']) if _b not in (4, 5) else None
COVERAGE = {k: v for k, v in COVERAGE.items() if v is not None}       # (index bytes 4 and 5 cannot hold a cut: topk <= 256)
