"""CPU: the numpy yardstick of the drawing rule (tests/draw_ref.py) against closed forms, and the conditions of the case
tables (tests/draw_cases.py) that make the device comparison of tests/test_gpu_draw.py a comparison of bytes."""
import numpy as np
import pytest

from tests import draw_ref as ref
from tests import draw_cases as dc


def blank(h, w):
    return np.zeros((h, w, 3), np.uint8)


def cover(img):
    return img.any(2)


def test_horizontal_segment_covers_exactly_its_row():
    img = blank(9, 20)
    n = ref.paint_segment(img, (3, 4), (15, 4), 1, (255, 255, 255))
    want = np.zeros((9, 20), bool)
    want[4, 3:16] = True
    assert n == 13 and np.array_equal(cover(img), want)


def test_disc_of_radius_5_covers_81_pixels():
    img = blank(21, 21)
    n = ref.paint_segment(img, (10, 10), (10, 10), 10, (1, 2, 3))
    ys, xs = np.mgrid[0:21, 0:21]
    assert n == 81 and np.array_equal(cover(img), (xs - 10) ** 2 + (ys - 10) ** 2 <= 25)


def test_thin_segments_of_every_slope_are_8_connected_without_a_gap():
    for qx in range(17):
        for qy in range(17):
            img = blank(17, 17)
            ref.paint_segment(img, (8, 8), (qx, qy), 1, (9, 9, 9))
            m = cover(img)
            assert m[8, 8] and m[qy, qx]
            dx, dy = qx - 8, qy - 8
            if abs(dx) >= abs(dy):                         # some pixel in every column (row) of the major direction
                assert m[:, min(8, qx):max(8, qx) + 1].any(0).all(), (qx, qy)
            else:
                assert m[min(8, qy):max(8, qy) + 1].any(1).all(), (qx, qy)
            # 8-connected: a flood fill from P over the covered pixels reaches every covered pixel
            seen, todo = {(8, 8)}, [(8, 8)]
            while todo:
                y, x = todo.pop()
                for ny in range(max(y - 1, 0), min(y + 2, 17)):
                    for nx in range(max(x - 1, 0), min(x + 2, 17)):
                        if m[ny, nx] and (ny, nx) not in seen:
                            seen.add((ny, nx))
                            todo.append((ny, nx))
            assert len(seen) == int(m.sum()), (qx, qy)


@pytest.mark.parametrize('alpha', [0, 77, 256])
def test_shade_formula(alpha):
    for px in (0, 255):
        for colour in (0, 200, 255):
            img = np.full((6, 6, 3), px, np.uint8)
            n = ref.paint_face(img, [(1, 1), (4, 1), (4, 4), (1, 4)], (colour,) * 3, alpha)
            assert n == 16
            want = (px * (256 - alpha) + colour * alpha + 128) >> 8
            assert (img[1:5, 1:5] == want).all() and (img[0] == px).all() and (img[:, 5] == px).all()
    # alpha 0 keeps the pixel, alpha 256 gives the colour, exactly
    assert (0 * 256 + 200 * 0 + 128) >> 8 == 0 and (255 * 256 + 128) >> 8 == 255 and (0 * 0 + 200 * 256 + 128) >> 8 == 200


def test_zero_area_face_covers_nothing():
    img = blank(8, 8)
    assert ref.paint_face(img, [(1, 1), (3, 3), (5, 5), (6, 6)], (255, 0, 0), 128) == 0
    assert ref.paint_face(img, [(2, 2), (2, 2), (2, 2), (2, 2)], (255, 0, 0), 128) == 0
    assert not img.any()
    # one degenerate triangle of the two: only the other covers
    assert ref.paint_face(img, [(1, 1), (5, 1), (5, 5), (3, 3)], (255, 0, 0), 256) == 15


def test_slot_0_lies_on_top_of_slot_1():
    rec = np.zeros((1, 2, 32), np.float32)
    rec[0, 0] = dc.record(0, (5, 5), np.zeros((8, 2)), (2, 10, 18, 10), 1)       # a horizontal box side through (10, 10)
    rec[0, 1] = dc.record(1, (5, 5), np.zeros((8, 2)), (10, 2, 10, 18), 1)       # a vertical one
    img = blank(20, 20)
    ref.draw([img], rec, layers=ref.BOX2D, colors=[(255, 0, 0), (0, 255, 0)])
    assert tuple(img[10, 10]) == (255, 0, 0) and tuple(img[5, 10]) == (0, 255, 0) and tuple(img[10, 5]) == (255, 0, 0)


def test_bad_coordinates_remove_one_primitive_only():
    assert ref.coord(8192.9) == 8192 and ref.coord(-8192.9) == -8192 and ref.coord(8193.0) is None and ref.coord(np.nan) is None
    assert ref.coord(-0.9) == 0 and ref.coord(np.inf) is None
    case = [c for c in dc.cases() if c['name'] == 'tiny'][0]
    imgs, _ = dc.backgrounds(case)
    before = [i.copy() for i in imgs]
    ref.draw(imgs, case['rec'][:, 1:2], layers=ref.WIREFRAME, colors=dc.COLORS)   # slot 1: vertex 5 is NaN
    assert (imgs[0] != before[0]).any()


CASES = dc.cases()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_case_conditions(case):
    p = case['params']
    layers = p.get('layers', dc.ALL_FRAME)
    rec, K = case['rec'], case['K']
    # every fp64 coordinate of the source 1 / bird's-eye cases lies at least MARGIN from an integer, no depth within MARGIN of 0.1
    if p.get('source', 0) == 1 or layers & ref.BEV:
        n = 0
        for b in range(rec.shape[0]):
            for r in rec[b]:
                if r[31] == 2:
                    assert dc.margins_ok(r, K[b], p['bev_hw'], p['bev_m_per_px']), case['name']
                    n += 1
        assert n > 0 or case['name'] == 'empty'
    imgs, bev = dc.backgrounds(case)
    before = [i.copy() for i in imgs]
    bev0 = None if bev is None else bev.copy()
    stats = ref.draw(imgs, rec, K, bev, **p)
    if case['name'] == 'empty':
        assert all(np.array_equal(a, b) for a, b in zip(imgs, before)) and np.array_equal(bev, bev0) and not any(stats.values())
        return
    for bit in dc.layers_of(case):                 # no case passes because everything was skipped
        assert stats[bit] > 0, (case['name'], bit, stats)
    for bit in set(stats) - set(dc.layers_of(case)):
        assert stats[bit] == 0


def test_case_specials():
    by = {c['name']: c for c in CASES}
    # min_flag = 2 paints less than min_flag = 1 on the same records; source 1 differs from source 0
    a, _ = dc.backgrounds(by['ragged'])
    b, _ = dc.backgrounds(by['min_flag2'])
    ref.draw(a, by['ragged']['rec'], by['ragged']['K'], dc.backgrounds(by['ragged'])[1], **by['ragged']['params'])
    ref.draw(b, by['min_flag2']['rec'], by['min_flag2']['K'], dc.backgrounds(by['min_flag2'])[1], **by['min_flag2']['params'])
    assert any((x != y).any() for x, y in zip(a, b))
    # the kitti case holds a box nearer than depth 0.1 that source 1 must skip
    k = by['kitti_source1']
    near = k['rec'][0, 14]
    assert near[31] == 2 and (ref.project_corners(near, k['K'][0])[1] < 0.1).any()
    assert k['hw'] == [(375, 1242)] and int((k['rec'][0, :, 31] == 2).sum()) == 13
    assert by['stack']['rec'].shape[1] == 100
