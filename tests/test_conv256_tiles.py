"""The host mirror of the conv256 tile lists (tests/conv256_tiles.py), which the GPU cases of tests/test_gpu_conv256.py use to
assert their regime, checked by hand-worked launches."""
import pytest

from tests import conv256_tiles as tl


# (B, H, W, cin, cout) of the dilation-6 lattice cases of test_gpu_kernels.py: tiles, per-XCD list, guaranteed run, ring bases
@pytest.mark.parametrize('shape,want', [
    ((1, 48, 32, 64, 256), (6, 1, 1, [0])),
    ((2, 48, 64, 256, 512), (48, 6, 1, [0])),
    ((40, 48, 32, 128, 256), (240, 30, 1, [0])),
    ((1, 96, 320, 256, 1024), (480, 60, 2, [0, 8])),
    ((3, 96, 64, 192, 256), (72, 9, 1, [0])),
    ((4, 96, 320, 64, 1024), (1920, 240, 8, [0, 2, 4, 6, 8, 10, 12, 14])),
    ((6, 96, 320, 192, 768), (2160, 270, 9, [0, 2, 4, 6, 8, 10, 12, 14])),
])
def test_lattice_lists(shape, want):
    B, H, W, cin, cout = shape
    r = tl.tiles('lattice', B * H * W, cout, 1, cin)
    assert (r['total'], max(r['lists']), r['run'], r['bases']) == want
    assert r['one_list'] is False


def test_one_list_boundary_and_empty_lists():
    assert tl.tiles('halo', 8 * 64 * 128, 256)['one_list'] is True                    # 256 tiles
    r = tl.tiles('halo', 257 * 8 * 32, 256)                                            # 257 tiles: chunk 33, the last list 26
    assert r['one_list'] is False and r['lists'] == [33] * 7 + [26] and r['run'] == 2
    r = tl.tiles('persistent', 256 * 256, 512, groups=2)                               # 1024 tiles, 128 per list
    assert r['lists'] == [128] * 8 and r['run'] == 4
    r = tl.tiles('lattice', 48 * 32, 256)                                              # MT = 6 < 8: two XCDs without a tile
    assert r['lists'] == [1] * 6 + [0, 0] and r['empty'] == 2
    assert tl.tiles('lattice', 48 * 32, 256, groups=4)['lists'] == [4] * 6 + [0, 0]
    assert tl.tiles('persistent', 48 * 32, 256)['lists'] == [6]                        # the same launch on the generic kernel: one list
    assert tl.tiles('1tile', 1000, 2304)['NT'] == 9


def test_ring_bases_reachable():
    assert [tl.reachable_bases(cpt) for cpt in (1, 2, 3, 4, 8)] == [list(range(0, 16, 2)), [0, 4, 8, 12], list(range(0, 16, 2)), [0, 8], [0]]


def test_route_of_names():
    assert tl.route_of('conv3x3_mfma256') == 'persistent' and tl.route_of('conv1x1_mfma256_1tile') == '1tile'
    assert tl.route_of('deconv4x4_phase_mfma256_halo') == 'halo' and tl.route_of('conv3x3_mfma256_lattice') == 'lattice'
    for bad in ('conv3x3_mfma', 'conv3x3_mfma256_deep', 'conv1x1_mfma_deep_splitk'):
        with pytest.raises(ValueError):
            tl.route_of(bad)
