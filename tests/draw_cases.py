"""Case tables of the drawing tests (tests/test_draw_cpu.py checks their conditions on the CPU, tests/test_gpu_draw.py runs
them on the device against tests/draw_ref.py).  A case = dict(name, hw = [(h, w)] per frame, rec (B, topk, 32) fp32, K (B, 9)
fp64 or None, params = keywords of draw_ref.draw / DrawParams, seed of the background).  Shapes are the smallest at which
the kernel (64 x 16 tiles, four pixels per thread, lists of 256 primitives) can go wrong."""
import os

import numpy as np

from tests import draw_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
COLORS = [(255, 64, 64), (64, 224, 64), (64, 128, 255)]
ALL_FRAME = ref.FACE | ref.BOX2D | ref.WIREFRAME | ref.KEYPOINT
MARGIN = 1e-6           # distance of every fp64 coordinate from an integer (and of every depth from 0.1): device sin / cos
#                         differ from numpy's by an ulp or so, 1e-12 in a pixel coordinate; they cannot move a pixel


def backgrounds(case):
    rng = np.random.Generator(np.random.PCG64(case['seed']))
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in case['hw']]
    bev = None
    if case['params'].get('layers', ALL_FRAME) & ref.BEV:
        bh, bw = case['params']['bev_hw']
        bev = rng.integers(0, 64, (len(imgs), bh, bw, 3), dtype=np.uint8)
    return imgs, bev


def record(cls, kp, verts, box, flag, box3d=None, score=0.9):
    r = np.zeros(32, np.float32)
    r[0], r[1], r[2:4], r[20:24], r[31] = cls, score, kp, box, flag
    r[4:20] = np.asarray(verts, np.float32).reshape(16)
    if box3d is not None:
        r[24:31] = box3d
    return r


def cuboid(x, y, sx, sy, ox, oy):
    """Eight vertices of a drawn cuboid in the record's vertex order (c = 4 i + 2 j + k, signs + before -): front face at
    (x, y) of half size (sx, sy), back face shifted by (ox, oy)."""
    v = []
    for i in (1, -1):
        for j in (1, -1):
            for k in (1, -1):
                v.append((x + i * sx + (ox if k < 0 else 0), y + j * sy + (oy if k < 0 else 0)))
    return v


def margins_ok(r, K, bev_hw, m):
    """The input conditions of the source 1 / bird's-eye cases for one flag-2 record."""
    pts = [ref.bev_points(r, bev_hw, m)]
    uv, depth = ref.project_corners(r, K)
    if np.any(np.abs(depth - 0.1) < MARGIN):
        return False
    if np.all(depth >= 0.1):
        pts.append(uv)
    pts = np.concatenate(pts).ravel()
    pts = pts[np.isfinite(pts) & (np.abs(pts) < 1e6)]
    return bool(np.all(np.abs(pts - np.round(pts)) >= MARGIN))


def _box3d(rng, K, bev_hw, m, near=False):
    """A random car-sized box that meets the margin conditions (redrawn until it does: met by construction)."""
    while True:
        b = np.array([rng.uniform(1.3, 1.9), rng.uniform(1.5, 1.9), rng.uniform(3.2, 4.6), rng.uniform(-12, 12), rng.uniform(0.8, 1.6),
                      rng.uniform(0.5, 1.5) if near else rng.uniform(6, 45), rng.uniform(-3.1, 3.1)], np.float32)
        r = np.zeros(32, np.float32)
        r[24:31] = b
        if margins_ok(r, K, bev_hw, m):
            return b


SMALL_K = np.array([60.0, 0, 26.0, 0, 60.0, 18.0, 0, 0, 1.0])


def _tiny():
    """37 x 53: smaller than one tile.  Slot 0: a cuboid partly off the frame with a vertex on the last row and column; slot 1:
    one NaN vertex (three edges and the face go, nine edges stay), a box wholly off the frame; slot 2: one coordinate of 9000."""
    v0 = cuboid(30, 20, 12, 9, 10, 7)
    v0[0] = (52, 36)
    v1 = cuboid(12, 14, 8, 8, -6, 5)
    v1[5] = (np.nan, 11.0)
    v2 = cuboid(25, 8, 10, 5, 4, -9)
    v2[6] = (9000.0, 4.0)
    rec = np.stack([record(0, (30.7, 20.2), v0, (-5.5, 3.2, 30.7, 50.9), 2), record(1, (12.9, 14.1), v1, (100, 100, 120, 130), 1),
                    record(2, (-3.0, 36.9), v2, (2.2, 1.1, 9000.0, 30.0), 1)])[None]
    return dict(name='tiny', hw=[(37, 53)], rec=rec, K=None, seed=1, params=dict(thickness=2, colors=COLORS))


def _ragged(name='ragged', **params):
    """64 x 200 (tile-exact rows) and 70 x 203 (inexact, odd row stride 609) in one call: primitives across the tile corners
    (64, 16), (128, 32), (192, 48), flags 1 and 2 mixed, one empty slot, solved boxes for the panel."""
    rng = np.random.Generator(np.random.PCG64(7))
    K = np.tile(np.array([150.0, 0, 100.0, 0, 150.0, 30.0, 0, 0, 1.0]), (2, 1))
    bev_hw, m = (70, 90), 0.5
    rec = np.zeros((2, 5, 32), np.float32)
    for b in range(2):
        for s, (x, y) in enumerate(((64, 16), (128, 32), (192, 48), (100, 60))):
            flag = 2 if (s + b) % 2 == 0 else 1
            rec[b, s] = record(s % 3, (x + 0.5, y - 0.5), cuboid(x, y, 14 + 3 * s, 9 + s, 11, -6), (x - 30.5, y - 14.5, x + 25.5, y + 12.5), flag,
                               _box3d(rng, K[b], bev_hw, m) if flag == 2 else None)
    p = dict(thickness=3, colors=COLORS, bev_hw=bev_hw, bev_m_per_px=m)
    p.update(params)
    return dict(name=name, hw=[(64, 200), (70, 203)], rec=rec, K=K, seed=2, params=p)


def _stack():
    """48 x 96, topk = 100: every slot's disc, box, wireframe and face over the same 20 x 20 pixels - 1800 primitives on one
    tile (eight list chunks), painter's order under compounding shade."""
    rng = np.random.Generator(np.random.PCG64(11))
    rec = np.zeros((1, 100, 32), np.float32)
    for s in range(100):
        verts = np.stack([rng.uniform(58, 78, 8), rng.uniform(12, 32, 8)], 1)
        x1, y1 = rng.uniform(58, 66), rng.uniform(12, 20)
        rec[0, s] = record(s % 3, (rng.uniform(60, 76), rng.uniform(14, 30)), verts, (x1, y1, x1 + rng.uniform(3, 12), y1 + rng.uniform(3, 12)), 1 + s % 2)
    return dict(name='stack', hw=[(48, 96)], rec=rec, K=None, seed=3, params=dict(thickness=1, radius=3, colors=COLORS))


def _kitti(source):
    """375 x 1242: twelve planted cuboids of tests/golden/planted_full.npz (the first twelve kept detections that meet the margin
    conditions), two 2D-only detections, one box nearer than the image plane allows and an empty slot; 400 x 400 panel."""
    g = np.load(os.path.join(GOLDEN, 'planted_full.npz'), allow_pickle=False)
    K = np.array(g['K'], np.float64)
    bev_hw, m = (400, 400), 0.2
    x, fun = g['d3_raw_x_0'], g['d3_raw_fun_0']
    rec, extra = [], []
    for i in range(len(fun)):
        r = record(int(g['det_cls_0'][i]), g['det_mproj_0'][i], g['det_verts_0'][i], g['det_bbox_0'][i], 2, score=float(g['det_score_0'][i]))
        r[24:31] = (x[i, 3], x[i, 4], x[i, 2], x[i, 5], x[i, 6], x[i, 7], np.arctan2(x[i, 0], x[i, 1]))
        if fun[i] < 0.1 and len(rec) < 12 and margins_ok(r, K, bev_hw, m):
            rec.append(r)
        elif not fun[i] < 0.1 and len(extra) < 2:
            r[31] = 1
            extra.append(r)
    assert len(rec) == 12 and len(extra) == 2
    rng = np.random.Generator(np.random.PCG64(13))
    near = record(1, (600.5, 180.5), cuboid(600, 180, 40, 30, 20, -10), (560.5, 150.5, 640.5, 210.5), 2, _box3d(rng, K, bev_hw, m, near=True))
    rec = np.stack(rec + extra + [near, np.zeros(32, np.float32)])[None]
    return dict(name='kitti_source%d' % source, hw=[(375, 1242)], rec=rec, K=K[None], seed=4,
                params=dict(layers=ALL_FRAME | ref.BEV, source=source, thickness=2, colors=COLORS, bev_hw=bev_hw, bev_m_per_px=m))


def _empty():
    return dict(name='empty', hw=[(37, 53), (70, 203)], rec=np.zeros((2, 6, 32), np.float32), K=np.tile(SMALL_K, (2, 1)), seed=5,
                params=dict(layers=ALL_FRAME | ref.BEV, source=1, colors=COLORS, bev_hw=(40, 70), bev_m_per_px=0.5))


def cases():
    out = [_tiny(), _ragged(layers=ALL_FRAME | ref.BEV), _stack(), _kitti(0), _kitti(1), _empty(),
           _ragged('min_flag2', layers=ALL_FRAME | ref.BEV, min_flag=2),
           _ragged('source1', layers=ALL_FRAME, source=1, thickness=1)]
    out += [_ragged('layer%d' % bit, layers=bit) for bit in (ref.FACE, ref.BOX2D, ref.WIREFRAME, ref.KEYPOINT, ref.BEV)]
    out += [_ragged('thickness%d' % t, thickness=t) for t in (1, 2, 15)]
    return out


# every case but 'empty' must paint something in every layer it enables
def layers_of(case):
    return [bit for bit in (ref.FACE, ref.BOX2D, ref.WIREFRAME, ref.KEYPOINT, ref.BEV) if case['params'].get('layers', ALL_FRAME) & bit]
