"""Host side of the JPEG frames (include/rtm3d_hip.h, "JPEG frames"; no device): the numpy restatement tests/jpeg_ref.py
against libjpeg-turbo's pixels of every fixture stream, the library's parser and Huffman decoder against the restatement,
what the header accepts made by byte surgery on the fixtures (no DHT, 16-bit DQT, fill bytes, bytes after EOI, no EOI), every
refusal with its reason, the launch schedule against the case table, the stand-alone robustness program, and the header
against the binding and the Makefile."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from rtm3d_amd import _lib
from tests import jpeg_cases as cases
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
    """The file holds what the tests below lean on: every size x every mode, three qualities, optimised tables, restart
    intervals 1, 2 and one MCU row - one of them past RST7 - and stays small."""
    names = cases.decodable()
    for size in ('1x1', '7x5', '8x8', '9x17', '16x16', '17x33', '37x53', '72x136'):
        for mode in ('grey', '444', '422', '420'):
            assert '%s_%s_q90' % (size, mode) in names
    for tag in ('q30', 'q100', 'q30_opt', 'q90_r1', 'q90_r2', 'q90_rrow'):
        for mode in ('grey', '444', '422', '420'):
            assert any(n.endswith('_%s_%s' % (mode, tag)) for n in names), (mode, tag)
    assert len(cases.restart_markers(cases.fixtures()['37x53_420_q90_r1'][0])) > 8
    assert os.path.getsize(cases.GOLDEN) < 200 * 1000


@pytest.mark.parametrize('name', cases.decodable())
def test_reference_equals_libjpeg(name):
    """tests/jpeg_ref.py decodes the stream to the very bytes libjpeg-turbo (through Pillow) decoded it to."""
    data, pixels = cases.fixtures()[name]
    info, buf = cases.reference(name)
    got = ref.decode_coef(buf, info['h'], info['w'], info['mode'])
    assert got.shape == pixels.shape and np.array_equal(got, pixels), name
    assert np.array_equal(ref.decode_coef(buf, info['h'], info['w'], info['mode'], 'bgr'), pixels[:, :, ::-1])


def test_fixtures_reach_both_clamps():
    """The pictures drive the inverse DCT past 0 and past 255 - in many planes, luma and chroma: the clamps of the rule are live."""
    low = high = 0
    for name in cases.decodable():
        info, buf = cases.reference(name)
        for c in range(info['ncomp']):
            n, at = info['bw'][c] * info['bh'][c], info['plane'][c]
            q = buf[64 * c:64 * c + 64].view(np.uint16).astype(np.int64)
            d = ref._w32(buf[at:at + 64 * n].astype(np.int64).reshape(n, 64) * q).reshape(n, 8, 8)
            col = np.stack(ref._pass([d[:, v, :] for v in range(8)], 11), axis=1)
            row = np.stack(ref._pass([col[:, :, u] for u in range(8)], 18), axis=2) + 128
            low += int(row.min() < 0)
            high += int(row.max() > 255)
    assert low >= 10 and high >= 10, (low, high)


def test_a_block_written_out_by_hand():
    """DC only: pass 1 gives (dc << 13 + 1024) >> 11 = 4 dc in row 0 of every column ... the sample is dc / 8 + 128 rounded."""
    for dc, q in ((8, 1), (-8, 1), (3, 5), (1000, 2), (-1000, 2)):
        c = np.zeros((1, 64), np.int16)
        c[0, 0] = dc
        want = min(max(((((dc * q) << 13) + 1024 >> 11 << 13) + (1 << 17) >> 18) + 128, 0), 255)
        assert (ref.idct(c, np.full(64, q)) == want).all(), (dc, q)


# ---------------------------------------------------------------------------------------------------- the library's host decoder
@pytest.mark.parametrize('name', cases.decodable())
def test_entropy_decode_equals_reference(jpeg, name):
    data = cases.fixtures()[name][0]
    info, buf = cases.reference(name)
    got = jpeg.entropy_decode(data)
    assert got.dtype == np.int16 and got.shape == buf.shape
    assert np.array_equal(got[:192], buf[:192]), 'tables'
    assert np.array_equal(got, buf)


@pytest.mark.parametrize('name', cases.decodable())
def test_info_fields(jpeg, name):
    data = cases.fixtures()[name][0]
    h, w = [int(v) for v in name.split('_')[0].split('x')]
    mode = name.split('_')[1]
    I = jpeg.info(data)
    L = ref.layout(h, w, jpeg.MODES[mode])
    assert (I['h'], I['w'], I['mode'], I['components']) == (h, w, mode, 1 if mode == 'grey' else 3)
    assert (I['mcus_x'], I['mcus_y'], I['bw'], I['bh']) == (L['mcus_x'], L['mcus_y'], L['bw'], L['bh'])
    assert I['table_offset'] == [0, 64, 128][:I['components']] and I['plane_offset'] == L['plane'] and I['coef_count'] == L['count']
    assert all(o % 64 == 0 for o in I['plane_offset']) and I['coef_count'] % 64 == 0
    mcu_w = {'grey': 8, '444': 8, '422': 16, '420': 16}[mode]
    want_ri = 0
    if name.endswith('_r1'):
        want_ri = 1
    elif name.endswith('_r2'):
        want_ri = 2
    elif name.endswith('_rrow'):
        want_ri = -(-w // mcu_w)
    assert I['restart_interval'] == want_ri
    assert jpeg.workspace_bytes([data, data]) == 4 * L['count']


def test_capacity_is_checked(lib, jpeg):
    data = cases.fixtures()['9x17_420_q90'][0]
    a = np.frombuffer(data, np.uint8)
    n = jpeg.info(data)['coef_count']
    buf = np.full(n, 0x5A5A, np.int16)
    assert lib.rtm3d_jpeg_entropy_decode(a.ctypes.data, a.size, buf.ctypes.data, n - 1) == 1
    assert 'holds %d int16, the frame needs %d' % (n - 1, n) in lib.rtm3d_last_error().decode() and (buf == 0x5A5A).all()
    assert lib.rtm3d_jpeg_entropy_decode(a.ctypes.data, a.size, buf.ctypes.data, n) == 0


@pytest.mark.parametrize('name', ['16x16_420_q90', '37x53_422_q90_r1', '9x17_grey_q100', '72x136_444_q90'])
def test_without_dht_the_annex_k_tables_apply(jpeg, name):
    """MJPEG style: a stream Pillow wrote with the standard tables decodes the same with its DHT segments cut out."""
    data = cases.fixtures()[name][0]
    cut = cases.cut_segments(data, 0xC4)
    assert len(cut) < len(data) - 200 and b'\xff\xc4' not in cut[:cases.scan_offset(cut)]
    assert np.array_equal(jpeg.entropy_decode(cut), cases.reference(name)[1])
    assert np.array_equal(ref.entropy_decode(cut)[1], cases.reference(name)[1])


@pytest.mark.parametrize('name', ['16x16_420_q90', '17x33_grey_q30_opt'])
def test_dqt_of_16_bit_entries(jpeg, name):
    data = cases.fixtures()[name][0]
    wide = cases.dqt_16bit(data)
    assert len(wide) > len(data) + 63
    assert np.array_equal(jpeg.entropy_decode(wide), cases.reference(name)[1])
    # and entries above 255 arrive whole
    at = cases.find_segment(wide, 0xDB)[0]
    big = cases.patch(wide, at + 5, [0xAB, 0xCD, 0x12, 0x34])
    got = jpeg.entropy_decode(big).view(np.uint16)
    assert got[0] == 0xABCD and got[1] == 0x1234 and np.array_equal(got[192:], cases.reference(name)[1].view(np.uint16)[192:])


def test_fill_bytes_after_eoi_and_missing_eoi(jpeg):
    name = '17x33_420_q90_r2'
    data, want = cases.fixtures()[name][0], cases.reference(name)[1]
    assert data[-2:] == b'\xff\xd9'
    # 0xFF fill bytes in front of every marker segment, of a restart marker and of EOI
    filled, last = b'', 0
    for m, at, n in ref.segments(data)[1:]:
        filled += data[last:at] + b'\xff\xff\xff'
        last = at
    filled += data[last:]
    r = cases.restart_markers(filled)[1]
    filled = filled[:r] + b'\xff\xff' + filled[r:-2] + b'\xff\xff\xff\xd9'
    assert len(filled) > len(data) + 20
    assert np.array_equal(jpeg.entropy_decode(filled), want)
    # bytes after EOI are ignored, even ones that look like a scan
    assert np.array_equal(jpeg.entropy_decode(data + b'\xff\xda\x00\x03garbage' * 3), want)
    # a missing EOI after a complete scan
    assert np.array_equal(jpeg.entropy_decode(data[:-2]), want)
    assert np.array_equal(jpeg.entropy_decode(data[:-1]), want)


def test_sof1_and_comments_are_accepted(jpeg):
    name = '9x17_422_q90'
    data, want = cases.fixtures()[name][0], cases.reference(name)[1]
    sof = cases.sof_offset(data)
    ext = cases.patch(data, sof + 1, [0xC1])
    ext = ext[:2] + b'\xff\xfe\x00\x07hello' + b'\xff\xe1\x00\x08Exif\x00\x00' + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01' + ext[2:]
    assert np.array_equal(jpeg.entropy_decode(ext), want)


def test_grey_sampling_factors_are_ignored(jpeg):
    name = '17x33_grey_q90'
    data, want = cases.fixtures()[name][0], cases.reference(name)[1]
    sof = cases.sof_offset(data)
    assert np.array_equal(jpeg.entropy_decode(cases.patch(data, sof + 11, [0x22])), want)


# ---------------------------------------------------------------------------------------------------- refusals
_REFUSALS = cases.refusals()


@pytest.mark.parametrize('case', _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_refusals(lib, case):
    """Each is refused with a message that names the reason; what the headers show is refused by rtm3d_jpeg_info already."""
    _, data, word = case
    a = np.frombuffer(data, np.uint8)
    info = _lib.JpegInfo()
    rc_info = lib.rtm3d_jpeg_info(a.ctypes.data, a.size, ctypes.byref(info))
    msg_info = lib.rtm3d_last_error().decode()
    buf = np.zeros(1 << 16, np.int16)
    assert lib.rtm3d_jpeg_entropy_decode(a.ctypes.data, a.size, buf.ctypes.data, buf.size) == 1
    msg = lib.rtm3d_last_error().decode()
    assert word in msg, msg
    if rc_info:
        assert word in msg_info and msg_info.startswith('jpeg_info: ')
    else:
        assert msg.startswith('jpeg_entropy_decode: ')


def test_null_and_empty(lib):
    info = _lib.JpegInfo()
    assert lib.rtm3d_jpeg_info(None, 0, ctypes.byref(info)) == 1 and 'null' in lib.rtm3d_last_error().decode()
    a = np.frombuffer(b'\xff\xd8', np.uint8)
    assert lib.rtm3d_jpeg_info(a.ctypes.data, 2, ctypes.byref(info)) == 1
    assert lib.rtm3d_jpeg_info(a.ctypes.data, 2, None) == 1
    n = ctypes.c_size_t()
    assert lib.rtm3d_jpeg_workspace_bytes(0, None, None, ctypes.byref(n)) == 1


# ---------------------------------------------------------------------------------------------------- the device stage's host side
def test_plan_equals_the_regime_table(jpeg):
    assert cases.tile() == (cases.TILE_W, cases.TILE_H, cases.HALO, cases.THREADS) and jpeg.CHUNK == cases.CHUNK
    for sizes, want in cases.plan_regimes():
        for mode in cases.MODES:
            plans = jpeg.plan([(0x1000, h, w, mode) for h, w in sizes])
            assert [(p.first, p.count, p.tiles, p.grid_x, p.grid_y) for p in plans] == want, (sizes, mode)
            assert all((p.tile_w, p.tile_h, p.halo, p.threads) == cases.tile() for p in plans)


def test_device_stage_refusals(lib, jpeg):
    ok = (0x1000, 8, 8, 0)
    dst = (ctypes.c_void_p * 2)(0x2000, 0x3000)
    err = lambda: lib.rtm3d_last_error().decode()
    check = lambda frames, d=dst, order=0: lib.rtm3d_frames_jpeg_check(len(frames), jpeg.c_frames(frames), d, order)
    assert check([ok, ok]) == 0
    for bad, word in (((0x1000, 0, 8, 0), 'frame 1 is 0 x 8'), ((0x1000, 8, 16385, 0), 'frame 1 is 8 x 16385'), ((0x1000, 8, 8, 4), 'frame 1 has the unknown mode 4'),
                      ((0x1000, 8, 8, -1), 'unknown mode'), ((0, 8, 8, 0), 'frame 1: the coefficient buffer is a NULL'),
                      ((0x1008, 8, 8, 0), 'frame 1: the coefficient buffer is not 16-byte aligned')):
        assert check([ok, bad]) == 1 and word in err(), (bad, err())
    assert check([ok, ok], order=2) == 1 and 'dst_order 2' in err()
    assert check([ok, ok], d=(ctypes.c_void_p * 2)(0x2000, 0)) == 1 and 'frame 1: the destination is a NULL' in err()
    assert lib.rtm3d_frames_jpeg_check(0, jpeg.c_frames([ok]), dst, 0) == 1 and 'B = 0' in err()
    arr = jpeg.c_frames([ok])
    arr[0].reserved = 7
    assert lib.rtm3d_frames_jpeg_check(1, arr, dst, 0) == 1 and 'reserved = 7' in err()
    out = (_lib.JpegPlan * 1)()
    assert lib.rtm3d_frames_jpeg_plan(1, arr, out) == 1 and lib.rtm3d_frames_jpeg_plan(1, jpeg.c_frames([ok]), None) == 1


def test_chain_refuses_before_it_touches_the_device(lib):
    """Refusals of rtm3d_frames_jpeg that come before the first copy need no device: a bad stream in the batch (named by its
    index), a short destination, a short workspace, bad arguments.  The pointers are made up; nothing dereferences them."""
    fx = cases.fixtures()
    good = np.frombuffer(fx['9x17_420_q90'][0], np.uint8)
    bad = np.frombuffer(fx[cases.PROGRESSIVE][0], np.uint8)
    cut = np.frombuffer(fx['9x17_420_q90'][0][:-40], np.uint8)
    n = 2 * ref.layout(9, 17, ref.YUV420)['count']
    stage = np.zeros(3 * n // 2, np.int16)
    err = lambda: lib.rtm3d_last_error().decode()

    def chain(streams, cap=3 * n, dst_bytes=9 * 17 * 3, order=0, threads=0, d_coef=0x10000):
        ptrs = (ctypes.c_void_p * len(streams))(*[s.ctypes.data for s in streams])
        sizes = (ctypes.c_size_t * len(streams))(*[s.size for s in streams])
        dst = (ctypes.c_void_p * len(streams))(*[0x100000 * (i + 1) for i in range(len(streams))])
        nb = (ctypes.c_size_t * len(streams))(*[dst_bytes] * len(streams))
        return lib.rtm3d_frames_jpeg(None, len(streams), ptrs, sizes, stage.ctypes.data, d_coef, cap, dst, nb, order, threads)

    assert chain([good, good, bad]) == 1 and err() == 'frames_jpeg: frame 2: progressive coding (SOF2)'
    assert chain([good, cut, good]) == 1 and err().startswith('frames_jpeg: frame 1: the entropy-coded data ends before the last MCU')
    assert chain([cut, cut, cut], threads=3) == 1 and err().startswith('frames_jpeg: frame 0: ')
    assert chain([good, good], dst_bytes=9 * 17 * 3 - 1) == 1 and 'frame 0: the destination holds 458 bytes, 9 x 17 x 3 = 459' in err()
    assert chain([good, good], cap=2 * n - 2) == 1 and 'the batch needs %d' % (2 * n) in err()
    assert chain([good], order=3) == 1 and 'dst_order 3' in err()
    assert chain([good], threads=65) == 1 and 'n_threads = 65' in err()
    assert chain([good], d_coef=0x10040) == 1 and '128-byte aligned' in err()
    assert chain([]) == 1 and 'B = 0' in err()


# ---------------------------------------------------------------------------------------------------- robustness, stand-alone
def test_parser_survives_truncations_and_mutations(tmp_path):
    """tests/jpeg_parse_main.cpp, compiled plainly with g++ against csrc/jpeg_host.cpp alone: every truncation and a fixed set of
    seeded mutations of every fixture stream, both buffers between canaries; it fails on a changed canary or on a return code
    that is neither success nor refusal."""
    fx = cases.fixtures()
    good = [fx[n][0] for n in cases.decodable()]
    streams = good + [b''] + [fx[cases.PROGRESSIVE][0]]
    path = tmp_path / 'streams.bin'
    path.write_bytes(struct.pack('<I', len(streams)) + b''.join(struct.pack('<I', len(s)) + s for s in streams))
    exe = str(tmp_path / 'jpeg_parse_main')
    subprocess.run(['g++', '-std=c++17', '-O2', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(REPO, 'tests', 'jpeg_parse_main.cpp'),
                    os.path.join(REPO, 'rtm3d_amd', 'csrc', 'jpeg_host.cpp')], check=True)
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r'(\d+) streams, (\d+) calls, (\d+) decoded, (\d+) refused, no failure', r.stdout)
    assert m and int(m.group(1)) == len(streams) and int(m.group(3)) >= len(good) and int(m.group(4)) > 10 * len(good), r.stdout


# ---------------------------------------------------------------------------------------------------- header, binding, Makefile
def test_header_binding_and_makefile(lib):
    hdr = open(os.path.join(REPO, 'include', 'rtm3d_hip.h')).read()
    assert '#define RTM3D_ABI_VERSION 9' in hdr and lib.rtm3d_abi_version() == 9 and _lib.ABI_VERSION == 9
    for name in ('rtm3d_jpeg_info', 'rtm3d_jpeg_entropy_decode', 'rtm3d_jpeg_workspace_bytes', 'rtm3d_frames_jpeg_plan', 'rtm3d_frames_jpeg_check',
                 'rtm3d_frames_jpeg_idct', 'rtm3d_frames_jpeg', 'rtm3d_engine_detect_frames_jpeg'):
        m = re.search(r'int %s\(([^;]*)\);' % name, hdr)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    for k, v in (('GREY', 0), ('444', 1), ('422', 2), ('420', 3)):
        assert '#define RTM3D_JPEG_%s %d' % (k, v) in hdr
    # the structs mirrored in Python have the C sizes
    src = ('#include "%s/include/rtm3d_hip.h"\n#include <stdio.h>\nint main(){printf("%%zu %%zu %%zu", sizeof(rtm3d_jpeg_stream_info), '
           'sizeof(rtm3d_jpeg_frame), sizeof(rtm3d_jpeg_plan));return 0;}' % REPO)
    os.makedirs(os.path.join(REPO, 'tests', '_build'), exist_ok=True)
    exe = os.path.join(REPO, 'tests', '_build', 'sizeof_jpeg')
    subprocess.run(['gcc', '-x', 'c', '-o', exe, '-'], input=src.encode(), check=True)
    sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(_lib.JpegInfo), ctypes.sizeof(_lib.JpegFrame), ctypes.sizeof(_lib.JpegPlan)]
    assert 'JPEG frames' in hdr and 'OUT OF SCOPE: entropy decoding on the device' in hdr
    mk = open(os.path.join(REPO, 'rtm3d_amd', 'csrc', 'Makefile')).read()
    assert ' jpeg.hip ' in mk and re.search(r'^HOST_SRCS := .*\bjpeg_host\.cpp\b', mk, re.M) and 'EXAMPLES += engine_detect_jpeg' in mk
    assert os.path.exists(os.path.join(REPO, 'examples', 'engine_detect_jpeg.c'))
    ignore = open(os.path.join(REPO, '.gitignore')).read().split()
    assert 'rtm3d_amd/_C/engine_detect_jpeg' in ignore
