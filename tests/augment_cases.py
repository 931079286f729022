"""The case tables of the training-augmentation tests (tests/test_augment_cpu.py, tests/test_gpu_augment.py): parameter sets that
reach every branch of the pixel rule, the shapes they run over, and the regime table of rtm3d_frames_augment_plan with the
schedule each regime must get - computed here by enumeration from the header's text, not by the library's formulas."""
import numpy as np

from tests import augment_ref as ref

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SRC_SIZES = [(1, 1), (2, 2), (5, 4), (37, 53)]                # (h, w)
CANVASES = [(32, 32), (33, 65), (48, 64)]                     # (H, W)
RECT_WIDTHS = [1, 3, 4, 5, 7, 8, 9, 64]                       # whole runs of 4 and every partial run
THREADS, PX, CHUNK, BORDER_GRID = 256, 4, 32, 512

# name -> dict(alpha, beta, sigma_q, scale, off ('ref': RandomAffine's own offset, or (fx, fy) as fractions of the rectangle), flip, fill)
PARAMS = {
    'identity': dict(),
    'brightness_contrast': dict(alpha=1.15, beta=-0.1),
    'noise': dict(sigma_q=202),
    'affine': dict(scale=1.2, off='ref'),
    'mirror': dict(flip=1),
    'all_on': dict(alpha=0.85, beta=0.12, sigma_q=453, scale=1.13, off='ref', flip=1),
    'zoom_out_fill': dict(scale=0.5, off=(0.31, 0.17), fill=(7, 200, 255)),           # OUT pixels on every side of the half-size frame
    'zoom_out_mirror': dict(scale=0.5, off=(0.1, 0.4), flip=1, fill=(1, 2, 3), sigma_q=202),
    'zoom_1_2': dict(scale=1.2, off=(-0.1, -0.1)),
    'clip_both_ends': dict(alpha=3.0, beta=-0.9),                                    # v < 77 -> 0, v > 161 -> 255
    'clip_negative_gain': dict(alpha=-1.0, beta=1.0),                                # the negative: 255 - v
    'sigma_453': dict(sigma_q=453),
    'sigma_max': dict(sigma_q=65535),                                                # +-3756 grey levels: every byte clips or stays
}
PARAM_NAMES = list(PARAMS)


def descriptor(h, w, x0, y0, rw, rh, name, seed):
    """One frame's descriptor fields as a dict (the rectangle is the test's own: any place, any size)."""
    p = PARAMS[name]
    scale = float(p.get('scale', 1.0))
    off = p.get('off', (0.0, 0.0))
    if isinstance(off, str):
        wh = np.array([rw, rh], np.float32)
        off = ((wh - wh * np.float32(scale)) / np.float32(2.0)).astype(np.float64)
    else:
        off = (off[0] * rw, off[1] * rh)
    ax, bx, ay, by = ref.geometry(h, w, rh, rw, scale, off[0], off[1], p.get('flip', 0))
    aq, bq, _ = ref.quantise(p.get('alpha', 1.0), p.get('beta', 0.0))
    return dict(h=h, w=w, x0=x0, y0=y0, rw=rw, rh=rh, alpha_q=aq, beta_q=bq, sigma_q=p.get('sigma_q', 0), seed=seed,
                fill=tuple(p.get('fill', (0, 0, 0))), ax=ax, bx=bx, ay=ay, by=by, scale=scale, off=(float(off[0]), float(off[1])),
                flip=int(p.get('flip', 0)))


def frame_bytes(h, w, rng, kind='random'):
    if kind == 'random':
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return np.full((h, w, 3), {'zeros': 0, 'ones': 255}[kind], np.uint8)


def reference_canvas(src, d, H, W, table=None):
    return ref.canvas(src, H, W, d['x0'], d['y0'], d['rw'], d['rh'], (d['ax'], d['bx'], d['ay'], d['by']), alpha_q=d['alpha_q'],
                      beta_q=d['beta_q'], sigma_q=d['sigma_q'], seed=d['seed'], fill=d['fill'], table=table)


def shape_jobs(H, W, seed):
    """[(src, descriptor)] of one canvas size: every source size x every rectangle width that fits x every parameter set, the
    rectangle's height and place drawn (so runs begin at every phase of 4 and touch every canvas edge)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    jobs = []
    for h, w in SRC_SIZES:
        src = frame_bytes(h, w, rng)
        for rw in RECT_WIDTHS:
            if rw > W:
                continue
            for k, name in enumerate(PARAM_NAMES):
                rh = int(rng.integers(1, H + 1)) if k % 3 else [1, H, 5][(k // 3) % 3]
                x0 = int(rng.integers(0, W - rw + 1)) if k % 4 else [0, W - rw][(k // 4) % 2]
                y0 = int(rng.integers(0, H - rh + 1))
                jobs.append((src, descriptor(h, w, x0, y0, rw, rh, name, seed=int(rng.integers(0, 2 ** 63)))))
    return jobs


# ---------------------------------------------------------------------------------------------------- the plan's regimes
def runs_meeting(lo, hi, shift, limit=20000):
    """The runs [4k - shift, 4k - shift + 3] that meet the columns lo .. hi - 1, by enumeration."""
    return sum(1 for k in range(limit) if 4 * k - shift + 3 >= lo and 4 * k - shift < hi)


# name -> (mode, H, W, border, [(x0, y0, rw, rh)] per frame)
REGIMES = {
    'one_full_canvas': (0, 32, 32, 0, [(0, 0, 32, 32)]),                              # no border launch
    'one_centred': (0, 48, 64, 0, [(3, 2, 57, 44)]),
    'packed_odd_width': (2, 33, 65, 0, [(1, 0, 64, 33), (0, 0, 65, 33)]),
    'nhwc4_border_0': (1, 48, 64, 0, [(5, 1, 9, 7)]),
    'nhwc4_border_1': (1, 48, 64, 1, [(5, 1, 9, 7)]),                                 # shift 1
    'nhwc4_border_3': (1, 48, 64, 3, [(0, 0, 64, 48), (1, 1, 3, 3)]),                 # shift 3; the first frame alone would need no border
    'nhwc4_border_6': (1, 48, 64, 6, [(61, 40, 3, 8)]),                               # shift 2
    'single_pixel': (2, 32, 32, 0, [(31, 31, 1, 1)]),
    'chunk_31': (0, 32, 32, 0, [(i % 5, i % 3, 8 + i % 7, 9 + i % 11) for i in range(31)]),
    'chunk_32': (0, 32, 32, 0, [(i % 5, i % 3, 8 + i % 7, 9 + i % 11) for i in range(32)]),
    'chunk_33': (0, 32, 32, 0, [(i % 5, i % 3, 8 + i % 7, 9 + i % 11) for i in range(33)]),
    'chunk_65_last_full': (1, 32, 64, 2, [(i % 5, i % 3, 8 + i % 7, 9 + i % 11) for i in range(64)] + [(0, 0, 64, 32)]),
    'kitti': (1, 384, 1280, 4, [(19, 4, 1242, 375)] * 32),
    'many_border_blocks': (0, 1024, 1280, 0, [(0, 0, 1279, 1024)]),                   # more canvas runs than the border grid takes at once
}


def expected_plan(name):
    """[dict] per chunk of 32 frames."""
    mode, H, W, border, rects = REGIMES[name]
    shift = (border & 3) if mode == 1 else 0
    out = []
    for b0 in range(0, len(rects), CHUNK):
        chunk = rects[b0:b0 + CHUNK]
        runs = max(runs_meeting(x0, x0 + rw, shift) * rh for x0, y0, rw, rh in chunk)
        per_row = runs_meeting(0, W, shift)
        any_border = any((rw, rh) != (W, H) for _, _, rw, rh in chunk)
        out.append(dict(first=b0, count=len(chunk), px_per_thread=PX, threads=THREADS, shift=shift, runs=runs, grid_x=-(-runs // THREADS),
                        grid_y=len(chunk), border_runs_per_row=per_row,
                        border_grid_x=min(-(-per_row * H // THREADS), BORDER_GRID) if any_border else 0))
    return out
