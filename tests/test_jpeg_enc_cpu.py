"""Host side of the JPEG encoding (include/rtm3d_hip.h, "JPEG encoding"; no device): the numpy restatement
tests/jpeg_enc_ref.py against the streams libjpeg-turbo (through Pillow) wrote for every fixture picture - bytes and
coefficients -, the library's Huffman encoder against the same bytes, the round trip over the decoder's fixture, the quality
tables, the quantiser's division and the size bound in stand-alone programs, every refusal with its reason, the launch
schedule against the case table, and the header against the binding and the Makefile."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import jpeg_enc_cases as cases
from tests import jpeg_enc_ref as enc
from tests import jpeg_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


@pytest.fixture(scope='module')
def jpeg(lib):
    from rtm3d_amd import jpeg
    return jpeg


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_fixture_grid():
    """The file holds what the issue lists - nine sizes x four modes at quality 90, four more qualities at two sizes, three
    restart intervals at two sizes - and is no larger than the decoder's fixture."""
    names = cases.names()
    for h, w in cases.SMALL_SIZES:
        for mode in ('grey', '444', '422', '420'):
            assert '%dx%d_%s_q90' % (h, w, mode) in names
    for size in ('9x17', '37x53'):
        for mode in ('grey', '444', '422', '420'):
            for q in (1, 30, 75, 100):
                assert '%s_%s_q%d' % (size, mode, q) in names
    for size, w in (('37x53', 53), ('17x33', 33)):
        for mode, mcu_w in (('grey', 8), ('444', 8), ('422', 16), ('420', 16)):
            for ri in (1, 2, -(-w // mcu_w)):
                assert '%s_%s_q90_r%d' % (size, mode, ri) in names
    assert len(names) == 92
    assert os.path.getsize(cases.GOLDEN) <= os.path.getsize(cases.OLD_GOLDEN)
    # (20, 40) in 4:2:0 has padding blocks both right and below
    L = ref.layout(20, 40, ref.YUV420)
    assert L['bw'][0] > -(-L['cw'][0] // 8) and L['bh'][0] > -(-L['ch'][0] // 8)


@pytest.mark.parametrize('name', cases.names())
def test_reference_bytes_equal_libjpeg(name):
    """tests/jpeg_enc_ref.py encodes the picture to the very bytes libjpeg-turbo wrote."""
    img, h, w, mode, q, ri, stream = cases.case(name)
    assert enc.entropy_encode(cases.reference(name), h, w, mode, ri) == stream


@pytest.mark.parametrize('name', cases.names())
def test_reference_coefficients_equal_libjpeg(name):
    """... and its coefficients are those of Pillow's stream on the tables and on every real block; its padding blocks are zero,
    Pillow's hold the running predictor and no AC."""
    img, h, w, mode, q, ri, stream = cases.case(name)
    info, buf = ref.entropy_decode(stream)
    mine = cases.reference(name)
    L = ref.layout(h, w, mode)
    real = enc.real_block_mask(L)
    assert (info['h'], info['w'], info['mode'], info['restart']) == (h, w, mode, ri)
    assert np.array_equal(mine[real], buf[real])
    assert not mine[~real].any()
    pad = ~real
    pad[:192] = False
    ac = pad.copy()
    ac[192::64] = False
    assert not buf[ac].any()


def test_a_block_written_out_by_hand():
    """A flat block of samples 128 + 24: pass 1 gives (8 * 24) << 2 = 768 in column 0 of every row, pass 2 (8 * 768 + 2) >> 2 = 1536
    at DC and nothing else; with q = 16 the DC quantises to (1536 + 64) / 128 = 12.  Its code bits with the Annex K luma tables:
    DC category 4 is '101', the value 12 is '1100', EOB is '1010': 1011 1001 010 and five 1-bits of padding = B9 5F."""
    c = enc.fdct(np.full((1, 8, 8), 152))
    assert c[0, 0] == 1536 and not c[0, 1:].any()
    assert enc.quantise(c, np.full(64, 16))[0, 0] == 12
    assert enc.quantise(np.array([-1536, 63, 64, -63, -64]), 16).tolist() == [-12, 0, 1, 0, -1]
    buf = np.zeros(192 + 64, np.int16)
    buf[:64] = 16
    buf[192] = 12
    s = enc.entropy_encode(buf, 8, 8, ref.GREY)
    sos = s.index(b'\xff\xda')
    assert s[sos + 10:] == b'\xb9\x5f\xff\xd9'
    # a negative DC and one AC term: DC -3 (category 2 '011', bits '00'), coefficient 1 = +1 (run 0 size 1 '00', bit '1'), EOB '1010'
    buf[192], buf[193] = -3, 1
    s = enc.entropy_encode(buf, 8, 8, ref.GREY)
    assert s[sos + 10:] == bytes([0b01100001, 0b10101111]) + b'\xff\xd9'


def test_edges_follow_libjpegs_order():
    """The last chroma row of 4:2:0 below an even height is the downsampled row ch - 1 repeated, not a downsample of row h - 1."""
    img = np.zeros((10, 8, 3), np.uint8)
    img[8] = 200
    img[9] = 40
    L = ref.layout(10, 8, ref.YUV420)
    y = enc.colour(img)[0]
    p = enc.component_plane(y, 1, L)                                       # (Y through the chroma path: any plane will do)
    assert p.shape == (8, 8) and (p[4] == 120).all() and (p[5:] == 120).all()
    p = enc.component_plane(y, 0, L)
    assert p.shape == (16, 8) and (p[9:] == 40).all()


# ---------------------------------------------------------------------------------------------------- the library's host encoder
@pytest.mark.parametrize('name', cases.names())
def test_entropy_encode_equals_libjpeg(jpeg, name):
    """rtm3d_jpeg_entropy_encode, fed the reference's coefficient buffer, writes Pillow's stream byte for byte."""
    img, h, w, mode, q, ri, stream = cases.case(name)
    got = jpeg.entropy_encode(cases.reference(name), h, w, mode, ri)
    assert got == stream
    assert len(got) <= jpeg.encode_bound(h, w, mode, ri)


def test_round_trip_over_the_decoders_fixture(jpeg):
    """For every decodable stream of tests/golden/jpeg_cases.npz whose Huffman tables are not optimised,
    entropy_encode(entropy_decode(s)) is s up to and including EOI - headers included: no header byte differed (that file and
    the encoder's fixture were written by the same Pillow, 12.2.0)."""
    from tests import jpeg_cases as old
    n = 0
    for name in old.decodable():
        if '_opt' in name:
            continue
        s = old.fixtures()[name][0]
        I = jpeg.info(s)
        got = jpeg.entropy_encode(jpeg.entropy_decode(s), I['h'], I['w'], I['mode'], I['restart_interval'])
        assert got == s[:s.rindex(b'\xff\xd9') + 2], name
        n += 1
    assert n >= 50


def test_quality_tables(jpeg):
    """quality_tables equals the formula for quality 1..100, luma and chroma, and the DQT segments Pillow wrote."""
    for q in range(1, 101):
        luma, chroma = jpeg.quality_tables(q)
        scale = 5000 // q if q < 50 else 200 - 2 * q
        for got, base in ((luma, enc.BASE_LUMA), (chroma, enc.BASE_CHROMA)):
            assert got.dtype == np.uint16 and np.array_equal(got, np.clip((base * scale + 50) // 100, 1, 255))
        assert np.array_equal(luma, enc.quality_tables(q)[0]) and np.array_equal(chroma, enc.quality_tables(q)[1])
    seen = set()
    for name in cases.names():
        img, h, w, mode, q, ri, stream = cases.case(name)
        P = ref.parse(stream)
        luma, chroma = jpeg.quality_tables(q)
        assert np.array_equal(P['q'][0], luma)
        if mode != ref.GREY:
            assert np.array_equal(P['q'][1], chroma) and np.array_equal(P['q'][2], chroma)
            seen.add(q)
    assert seen == {1, 30, 75, 90, 100}
    with pytest.raises(RuntimeError, match='quality 0'):
        jpeg.quality_tables(0)
    with pytest.raises(RuntimeError, match='quality 101'):
        jpeg.quality_tables(101)


def test_layout_and_bound(jpeg):
    for h, w in cases.SMALL_SIZES + [(384, 1280), (16384, 16384)]:
        for mode in cases.MODES:
            L, I = ref.layout(h, w, mode), jpeg.frame_layout(h, w, mode)
            assert (I['mcus_x'], I['mcus_y'], I['bw'], I['bh'], I['plane_offset'], I['coef_count']) == (L['mcus_x'], L['mcus_y'], L['bw'], L['bh'], L['plane'], L['count'])
            blocks = (L['count'] - 192) // 64
            n, t = L['ncomp'], 1 if mode == ref.GREY else 2
            head = 2 + 18 + 69 * t + 10 + 3 * n + 216 * t + 8 + 2 * n
            assert jpeg.encode_bound(h, w, mode) == head + 416 * blocks + 2
            mcus = L['mcus_x'] * L['mcus_y']
            assert jpeg.encode_bound(h, w, mode, 3) == head + 6 + 416 * blocks + 2 * ((mcus - 1) // 3) + 2


def _compile(tmp_path, name, sources):
    exe = str(tmp_path / name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-Wall', '-Wextra', '-Werror', '-o', exe] + [os.path.join(REPO, s) for s in sources], check=True)
    return exe


def test_quantiser_division_is_exact(tmp_path):
    """tests/jpeg_quant_main.cpp compiles csrc/jpeg_quant.h - the function the device stage uses - and walks every q in 1..255 and
    every |c| <= 32767, both signs."""
    exe = _compile(tmp_path, 'jpeg_quant_main', ['tests/jpeg_quant_main.cpp'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip() == '%d cases, no mismatch' % (255 * 32768 * 2)
    assert '#include "jpeg_quant.h"' in open(os.path.join(REPO, 'rtm3d_amd', 'csrc', 'jpeg_enc.hip')).read()


def test_bound_holds_on_adversarial_buffers(tmp_path):
    """tests/jpeg_bound_main.cpp, compiled plainly with g++ against csrc/jpeg_host.cpp alone: adversarial coefficient buffers
    (every AC +-1023, DC differences of category 11, streams full of stuffed 0xFF) stay within the bound and between their
    canaries, a capacity of bound - 1 is refused and writes nothing."""
    exe = _compile(tmp_path, 'jpeg_bound_main', ['tests/jpeg_bound_main.cpp', 'rtm3d_amd/csrc/jpeg_host.cpp'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r'(\d+) cases, fullest stream (0\.\d+) of its bound, (\d+) stuffed bytes, no failure', r.stdout)
    assert m and int(m.group(1)) == 8 * 4 * 3 * 3 and float(m.group(2)) > 0.8 and int(m.group(3)) > 100000, r.stdout


# ---------------------------------------------------------------------------------------------------- refusals
_REFUSALS = cases.entropy_refusals()


@pytest.mark.parametrize('case', _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_entropy_encode_refusals(lib, jpeg, case):
    _, buf, h, w, mode, restart, cap, word = case
    buf = np.ascontiguousarray(buf)
    out = np.full(1 << 16, 0xA5, np.uint8)
    capacity = out.size if cap is None else jpeg.encode_bound(h, w, mode, restart) + cap
    n = ctypes.c_size_t()
    assert lib.rtm3d_jpeg_entropy_encode(buf.ctypes.data, h, w, mode, restart, out.ctypes.data, capacity, ctypes.byref(n)) == 1
    msg = lib.rtm3d_last_error().decode()
    assert msg.startswith('jpeg_entropy_encode: ') and word in msg, msg
    if 'category' not in word and 'AC coefficient' not in word:
        assert (out == 0xA5).all()                                          # refused before a byte was written


def test_null_pointers(lib):
    n = ctypes.c_size_t()
    buf = np.zeros(256, np.int16)
    out = np.zeros(4096, np.uint8)
    err = lambda: lib.rtm3d_last_error().decode()
    assert lib.rtm3d_jpeg_entropy_encode(None, 8, 8, 0, 0, out.ctypes.data, out.size, ctypes.byref(n)) == 1 and 'null' in err()
    assert lib.rtm3d_jpeg_entropy_encode(buf.ctypes.data, 8, 8, 0, 0, None, out.size, ctypes.byref(n)) == 1 and 'null' in err()
    assert lib.rtm3d_jpeg_entropy_encode(buf.ctypes.data, 8, 8, 0, 0, out.ctypes.data, out.size, None) == 1 and 'null' in err()
    assert lib.rtm3d_jpeg_quality_tables(50, None, None) == 1 and 'null' in err()
    assert lib.rtm3d_jpeg_frame_layout(8, 8, 0, None) == 1 and 'null' in err()
    assert lib.rtm3d_jpeg_encode_workspace_bytes(0, None, 0, ctypes.byref(n)) == 1 and 'B = 0' in err()


# ---------------------------------------------------------------------------------------------------- the device stage's host side
def test_plan_equals_the_regime_table(jpeg):
    assert jpeg.CHUNK == cases.CHUNK
    for sizes, want in cases.plan_regimes():
        for mode in cases.MODES:
            plans = jpeg.fdct_plan([(0, 0, h, w, mode) for h, w in sizes])
            assert [(p.first, p.count, p.tiles, p.grid_x, p.grid_y) for p in plans] == want, (sizes, mode)
            assert all((p.tile_w, p.tile_h, p.threads, p.lds_stride, p.lds_stride_sub) ==
                       (cases.TILE_W, cases.TILE_H, cases.THREADS, cases.LDS_STRIDE, cases.LDS_STRIDE_SUB) for p in plans)
    # the strides keep a half-wave's 8-byte block reads on distinct banks: 64 banks of 4 bytes, 32 lanes
    for stride, blocks_x in ((cases.LDS_STRIDE, 16), (cases.LDS_STRIDE_SUB, 8)):
        for row in range(8):
            banks = [(((t // blocks_x) * 8 + row) * stride + (t % blocks_x) * 8) // 4 % 64 for t in range(32)]
            assert len(set(banks)) == 32 and all((b + 1) % 64 not in banks for b in banks)


def test_device_stage_refusals(lib, jpeg):
    ok = (0x1000, 0x2000, 8, 8, 0)
    luma, chroma = jpeg.quality_tables(90)
    err = lambda: lib.rtm3d_last_error().decode()

    def check(frames, ql=luma, qc=chroma, order=0):
        return lib.rtm3d_frames_jpeg_fdct_check(len(frames), jpeg.c_enc_frames(frames), ql.ctypes.data if ql is not None else None,
                                                qc.ctypes.data if qc is not None else None, order)

    assert check([ok, ok]) == 0
    for bad, word in cases.fdct_refusals():
        assert check([ok, bad]) == 1 and word in err(), (bad, err())
    assert check([ok, ok], order=2) == 1 and 'src_order 2' in err()
    assert check([ok], ql=None) == 1 and 'null' in err()
    zero, big = luma.copy(), chroma.copy()
    zero[7], big[9] = 0, 256
    assert check([ok], ql=zero) == 1 and 'entry 7 of the luma table is 0' in err()
    assert check([ok], qc=big) == 1 and 'entry 9 of the chroma table is 256' in err()
    assert lib.rtm3d_frames_jpeg_fdct_check(0, jpeg.c_enc_frames([ok]), luma.ctypes.data, chroma.ctypes.data, 0) == 1 and 'B = 0' in err()
    arr = jpeg.c_enc_frames([ok])
    arr[0].reserved = 7
    assert lib.rtm3d_frames_jpeg_fdct_check(1, arr, luma.ctypes.data, chroma.ctypes.data, 0) == 1 and 'reserved = 7' in err()
    out = (_lib.JpegEncPlan * 1)()
    assert lib.rtm3d_frames_jpeg_fdct_plan(1, arr, out) == 1 and lib.rtm3d_frames_jpeg_fdct_plan(1, jpeg.c_enc_frames([ok]), None) == 1


def test_chain_refuses_before_it_touches_the_device(lib, jpeg):
    """Refusals of rtm3d_frames_jpeg_encode that come before the first launch need no device.  The device pointers are made up;
    nothing dereferences them."""
    luma, chroma = jpeg.quality_tables(90)
    err = lambda: lib.rtm3d_last_error().decode()
    stage = np.zeros(1 << 14, np.int16)
    need = 2 * 2 * ref.layout(9, 17, ref.YUV420)['count']
    bound = jpeg.encode_bound(9, 17, '420')
    outs = [np.full(bound, 0xA5, np.uint8) for _ in range(2)]

    def chain(hw=(9, 17, 9, 17), mode=3, cap=need, out_cap=bound, order=0, restart=0, threads=0, d_coef=0x10000, src1=0x200000, ql=luma):
        B = len(hw) // 2
        src = (ctypes.c_void_p * B)(*([0x100000, src1][:B]))
        ptrs = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs[:B]])
        caps = (ctypes.c_size_t * B)(*[out_cap] * B)
        lens = (ctypes.c_size_t * B)()
        return lib.rtm3d_frames_jpeg_encode(None, B, src, (ctypes.c_int * len(hw))(*hw), mode, ql.ctypes.data, chroma.ctypes.data, order, restart, d_coef,
                                            stage.ctypes.data, cap, ptrs, caps, lens, threads)

    assert chain(hw=(9, 17, 0, 17)) == 1 and 'frame 1: a frame of 0 x 17' in err()
    assert chain(mode=5) == 1 and 'unknown mode 5' in err()
    assert chain(cap=need - 2) == 1 and 'the batch needs %d' % need in err()
    assert chain(out_cap=bound - 1) == 1 and 'frame 0: the output holds %d bytes, a stream of this frame may need %d' % (bound - 1, bound) in err()
    assert chain(order=3) == 1 and 'src_order 3' in err()
    assert chain(restart=65536) == 1 and 'restart interval of 65536' in err()
    assert chain(threads=65) == 1 and 'n_threads = 65' in err()
    assert chain(d_coef=0x10040) == 1 and '128-byte aligned' in err()
    assert chain(src1=0) == 1 and 'frame 1: the source is a NULL' in err()
    bad = luma.copy()
    bad[0] = 300
    assert chain(ql=bad) == 1 and 'entry 0 of the luma table is 300' in err()
    assert chain(hw=()) == 1 and 'B = 0' in err()
    assert all((o == 0xA5).all() for o in outs)
    n = ctypes.c_size_t()
    assert lib.rtm3d_jpeg_encode_workspace_bytes(2, (ctypes.c_int * 4)(9, 17, 9, 17), 3, ctypes.byref(n)) == 0 and n.value == need


# ---------------------------------------------------------------------------------------------------- header, binding, Makefile
def test_header_binding_and_makefile(lib):
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert '#define RTM3D_ABI_VERSION 9' in hdr and lib.rtm3d_abi_version() == 9 and _lib.ABI_VERSION == 9
    for name in ('rtm3d_jpeg_quality_tables', 'rtm3d_jpeg_frame_layout', 'rtm3d_jpeg_encode_bound', 'rtm3d_jpeg_entropy_encode', 'rtm3d_frames_jpeg_fdct_plan',
                 'rtm3d_frames_jpeg_fdct_check', 'rtm3d_frames_jpeg_fdct', 'rtm3d_jpeg_encode_workspace_bytes', 'rtm3d_frames_jpeg_encode',
                 'rtm3d_frames_jpeg_encode_queue', 'rtm3d_frames_jpeg_encode_finish'):
        m = re.search(r'int %s\(([^;]*)\);' % name, hdr)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    src = ('#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\nint main(){printf("%%zu %%zu", sizeof(rtm3d_jpeg_enc_frame), '
           'sizeof(rtm3d_jpeg_enc_plan));return 0;}' % REPO)
    os.makedirs(os.path.join(REPO, 'tests', '_build'), exist_ok=True)
    exe = os.path.join(REPO, 'tests', '_build', 'sizeof_jpeg_enc')
    subprocess.run(['gcc', '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.JpegEncFrame), ctypes.sizeof(_lib.JpegEncPlan)] == [32, 40]
    assert 'JPEG encoding (csrc/jpeg_enc.hip, csrc/jpeg_host.cpp)' in hdr and 'OUT OF SCOPE: optimised Huffman tables' in hdr
    decoder_scope = hdr[hdr.index('OUT OF SCOPE: entropy decoding on the device'):hdr.index('#define RTM3D_JPEG_GREY')]
    assert 'JPEG encoding,' not in decoder_scope
    mk = open(os.path.join(REPO, 'rtm3d_amd', 'csrc', 'Makefile')).read()
    assert ' jpeg_enc.hip ' in mk and 'EXAMPLES += engine_draw_jpeg' in mk
    assert os.path.exists(os.path.join(REPO, 'examples', 'engine_draw_jpeg.c'))
    assert 'rtm3d_amd/_C/engine_draw_jpeg' in open(os.path.join(REPO, '.gitignore')).read().split()
