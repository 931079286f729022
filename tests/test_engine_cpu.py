"""CPU: engine files (rtm3d_amd/engine.py, csrc/engine.cpp).  An exported engine holds exactly the C ABI call stream that
plan.PlanRecorder issues (same digest as tests/abi_recorder.py gives for the direct recording), export is deterministic,
the C loader's host-side checks refuse every kind of damaged file before any device work, struct rtm3d_engine_info has
the same layout in C and in ctypes, and the plain C example compiles and links against the header and the library."""
import ctypes
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import rtm3d_amd
from rtm3d_amd import _lib, engine, plan as plan_mod, weights
from tests.abi_recorder import AbiRecorder, record

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, 'tests', '_build')

DIM5 = [[1.52607842, 1.62858147, 3.88396124], [1.76067766, 0.6602296, 0.84220464], [1.73712792, 0.59677122, 1.76338868],
        [2.0, 1.9, 5.0], [3.2, 2.5, 9.0]]


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    return True


def make_model(bb, seed=3, nconv=2, classes=3, head_precision='fp16'):
    cfg = rtm3d_amd.kitti_config(bb)
    cfg.MODEL.HEADER_NUM_CONV = nconv
    if classes != 3:
        cfg.DATASET.OBJs = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck'][:classes]
    m = rtm3d_amd.create_model(cfg, head_precision=head_precision)
    m.load_state_dict(weights.synth_state_dict(bb, seed, 'trained', header_num_conv=nconv, num_classes=classes))
    return m


# case: (backbone, B, H, W, model options, save_engine options)
CASES = {
    'dla34_b1_64x128': ('DLA-34', 1, 64, 128, {}, {}),
    'dla34_b32_384x1280': ('DLA-34', 32, 384, 1280, {}, {}),
    'resnet18_b2_128x256': ('RESNET-18', 2, 128, 256, {}, {}),
    'resnet34_b2_128x256': ('RESNET-34', 2, 128, 256, {}, {}),
    'dla34_header_num_conv1': ('DLA-34', 2, 128, 256, {'nconv': 1}, {}),
    'dla34_header_num_conv3': ('DLA-34', 2, 128, 256, {'nconv': 3}, {}),
    'resnet18_five_classes': ('RESNET-18', 2, 64, 128, {'classes': 5}, {'dim_ref': DIM5}),
    'dla34_mxfp8': ('DLA-34', 2, 128, 256, {}, {'head_precision': 'mxfp8'}),
}


def _direct_recording(m, B, H, W, prec):
    rec = record(plan_mod.build_plan(m._sd, m._backbone_name, B, H, W, m._head_variant, num_classes=m._num_classes,
                                     header_num_conv=m._num_conv, head_precision=prec))
    return rec.digest(), len(rec.calls), len(rec.launches())


@pytest.mark.parametrize('case', sorted(CASES))
def test_engine_holds_the_realized_call_stream(case, tmp_path):
    bb, B, H, W, mk, sk = CASES[case]
    m = make_model(bb, **mk)
    path = str(tmp_path / 'e.rtm3d')
    meta = m.save_engine(path, B, H, W, **sk)
    prec = sk.get('head_precision', 'fp16')
    assert (meta['B'], meta['H'], meta['W'], meta['backbone'], meta['head_precision']) == (B, H, W, bb, prec)
    assert meta['header_num_conv'] == mk.get('nconv', 2) and meta['num_classes'] == mk.get('classes', 3)
    assert meta['head_channels'] == [mk.get('classes', 3), 16, 2, 2] and meta['topk'] == 100 and meta['fun_accept'] == 0.1
    assert meta['use_graph'] == (B <= 8) and meta['solver_form'] == 1 and meta['ref_loc'] == [0.0, -0.5, 20.0]
    parsed = engine.read_engine(path)
    rec = AbiRecorder()
    engine.replay(parsed, rec)
    want, n_calls, n_launches = _direct_recording(m, B, H, W, prec)
    assert len(rec.calls) == n_calls and len(rec.launches()) == n_launches
    assert rec.digest() == want
    # the body holds only allowlisted state-changing calls
    assert {name for name, _ in parsed['records']} <= set(engine.OPCODES)
    os.remove(path)


def test_export_is_deterministic_and_keyed_by_the_weights(tmp_path):
    from rtm3d_amd.weight_cache import state_dict_digest
    m = make_model('DLA-34')
    a, b, c = (str(tmp_path / n) for n in ('a', 'b', 'c'))
    m.save_engine(a, 1, 64, 128)
    make_model('DLA-34').save_engine(b, 1, 64, 128)          # a fresh model of the same weights (no shared weight cache)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    make_model('DLA-34', seed=4).save_engine(c, 1, 64, 128)
    pa, pc = engine.read_engine(a), engine.read_engine(c)
    assert pa['state_digest'] == state_dict_digest(m._sd) and pa['state_digest'] != pc['state_digest']
    assert pa['blobs'] != pc['blobs']


def test_export_does_not_need_the_loader(tmp_path, monkeypatch):
    """save_engine "needs neither a GPU nor the library": with a loader that refuses, export and record_plan still work."""
    def refuse():
        raise AssertionError('export loaded the library')
    monkeypatch.setattr('rtm3d_amd._lib.load', refuse)
    m = make_model('DLA-34')
    path = str(tmp_path / 'e.rtm3d')
    assert m.save_engine(path, 1, 64, 128)['B'] == 1 and engine.read_engine(path)['records']
    records, blobs = engine.record_plan(plan_mod.build_plan(m._sd, 'DLA-34', 2, 64, 128))
    assert len(blobs) == sum(1 for name, _ in records if name == 'rtm3d_blob_create') > 0


def test_export_never_replaces_the_loader(tmp_path, monkeypatch):
    """While an export records, rtm3d_amd._lib.load is the function it always was: a thread that decodes or builds a real
    plan beside it gets the library."""
    original, seen = _lib.load, []

    class Watching(engine._Recorder):
        def _record(self, name, args):
            seen.append(_lib.load is original)
            return super(Watching, self)._record(name, args)
    monkeypatch.setattr(engine, '_Recorder', Watching)
    make_model('DLA-34').save_engine(str(tmp_path / 'e.rtm3d'), 1, 64, 128)
    assert len(seen) > 100 and all(seen) and _lib.load is original


def test_sparse_heads_and_other_head_tables_are_not_exported(tmp_path):
    m = make_model('DLA-34')
    with pytest.raises(NotImplementedError, match='sparse_heads'):
        m.save_engine(str(tmp_path / 'p'), 1, 64, 128, sparse_heads=True)
    pir = plan_mod.build_peak_plan(m._sd, 100, (16, 32))
    with pytest.raises(NotImplementedError, match='sparse_heads'):
        engine.record_plan(pir)
    cfg = rtm3d_amd.kitti_config('DLA-34')
    cfg.MODEL.HEAD_VARIANT = 'smoke'
    with pytest.raises(NotImplementedError, match='smoke'):
        rtm3d_amd.create_model(cfg).save_engine(str(tmp_path / 's'), 1, 64, 128)
    with pytest.raises(IndexError, match='dim_ref'):
        make_model('RESNET-18', classes=5).save_engine(str(tmp_path / 'd'), 1, 64, 128)
    assert not os.listdir(str(tmp_path))


def test_engine_info_layout_matches_ctypes(built):
    fields = [f for f, _ in engine.EngineInfo._fields_]
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "%s/include/rtm3d_hip.h"' % REPO, 'int main(void) {',
           '  printf("%zu\\n", sizeof(rtm3d_engine_info));']
    src += ['  printf("%%zu\\n", offsetof(rtm3d_engine_info, %s));' % f for f in fields]
    src += ['  return 0;', '}']
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'engine_info_layout')
    subprocess.run(['gcc', '-x', 'c', '-o', exe, '-'], input='\n'.join(src).encode(), check=True)
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(engine.EngineInfo)
    assert got[1:] == [getattr(engine.EngineInfo, f).offset for f in fields]


# ---------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope='module')
def small_engine(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('eng') / 'small.rtm3d')
    make_model('DLA-34').save_engine(path, 1, 64, 128)
    return open(path, 'rb').read()


H0 = engine.HEADER_BYTES
META_END = H0 + engine._META.size


def _sections(data):
    """(records start, records end, blob area start) file offsets and [(opcode, payload offset, payload bytes)]."""
    nrec, _, rbytes = engine._COUNTS.unpack_from(data, META_END)
    pos = rbeg = META_END + engine._COUNTS.size
    recs = []
    for _ in range(nrec):
        op, n = engine._REC.unpack_from(data, pos)
        recs.append((op, pos + 8, n))
        pos += 8 + n
    boff, _ = engine._BLOBS.unpack_from(data, rbeg + rbytes)
    return rbeg, rbeg + rbytes, H0 + boff, recs


def _resign(data):
    """Header body length and sha256 made consistent with a (damaged) body, so that the inner checks are reached."""
    data = bytearray(data)
    body = bytes(data[H0:])
    struct.pack_into('<32sQ', data, 96, hashlib.sha256(body).digest(), len(body))
    return bytes(data)


def _first(recs, name):
    return next(r for r in recs if r[0] == engine.OPCODES[name][0])


def _patch(data, off, fmt, *vals):
    data = bytearray(data)
    struct.pack_into(fmt, data, off, *vals)
    return bytes(data)


def _damaged(data):
    rbeg, rend, bstart, recs = _sections(data)
    blob, conv, inp = _first(recs, 'rtm3d_blob_create'), _first(recs, 'rtm3d_op_conv'), _first(recs, 'rtm3d_op_input_nhwc4')
    flipped = bytearray(data)
    flipped[bstart + 1000] ^= 0x01
    out = {
        'bad_magic': (_patch(data, 0, '8s', b'RTM3DXXX'), 'bad magic'),
        'format_version': (_patch(data, 8, '<I', 2), 'format version 2'),
        'abi_version': (_patch(data, 12, '<I', 8), 'ABI 8'),
        'flipped_payload_byte': (bytes(flipped), 'sha256'),
        'truncated_header': (data[:100], 'truncated header'),
        'blob_past_eof': (_resign(_patch(data, blob[1], '<Q', len(data))), r'record \d+ \(blob_create\).*past the end of the file'),
        'unknown_opcode': (_resign(_patch(data, inp[1] - 8, '<I', 99)), r'record \d+: unknown opcode 99'),
        'wrong_desc_size': (_resign(_patch(data, conv[1], '<I', ctypes.sizeof(_lib.ConvDesc) - 4)), r'record \d+ \(op_conv\): descriptor'),
        'tensor_id_out_of_range': (_resign(_patch(data, inp[1], '<i', 9999)), r'record \d+ \(op_input_nhwc4\): tensor id 9999'),
    }
    # truncation at each section boundary: as cut (the header's body length no longer matches), and re-signed so that the
    # section lengths themselves are checked against the end of the file
    for name, at in (('header_end', H0), ('metadata_end', META_END), ('records_start', rbeg), ('records_end', rend),
                     ('blob_area_start', bstart), ('last_blob_byte', len(data) - 1)):
        out['cut_at_' + name] = (data[:at], 'truncated or padded')
        out['cut_at_%s_resigned' % name] = (_resign(data[:at]), 'truncated metadata|runs past the end|does not end at the end|past the end of the file')
    return out


DAMAGE = ['bad_magic', 'format_version', 'abi_version', 'flipped_payload_byte', 'truncated_header', 'blob_past_eof', 'unknown_opcode',
          'wrong_desc_size', 'tensor_id_out_of_range'] + \
    ['cut_at_%s%s' % (n, r) for n in ('header_end', 'metadata_end', 'records_start', 'records_end', 'blob_area_start', 'last_blob_byte')
     for r in ('', '_resigned')]


def test_the_small_engine_is_accepted(built, small_engine, tmp_path):
    path = str(tmp_path / 'ok.rtm3d')
    open(path, 'wb').write(small_engine)
    info = engine.inspect_engine(path)
    parsed = engine.read_engine(path)
    assert info['n_records'] == len(parsed['records']) and info['n_blobs'] == len(parsed['blobs'])
    assert info['blob_bytes'] == sum(len(b) for b in parsed['blobs']) and info['file_bytes'] == len(small_engine)
    assert info['state_digest'] == parsed['state_digest'] and info['arch'] == 'gfx950' and info['abi_version'] == _lib.ABI_VERSION
    assert (info['B'], info['H'], info['W'], info['backbone'], info['topk']) == (1, 64, 128, 'DLA-34', 100)
    assert info['dim_ref'] == parsed['meta']['dim_ref'] and info['score_thresh'] == np.float32(0.4)
    assert info['n_launches'] == sum(1 for n, _ in parsed['records'] if n.startswith('rtm3d_op_'))


@pytest.mark.parametrize('damage', DAMAGE)
def test_damaged_engines_are_refused_before_device_work(built, small_engine, tmp_path, damage):
    data, why = _damaged(small_engine)[damage]
    path = str(tmp_path / 'bad.rtm3d')
    open(path, 'wb').write(data)
    lib = _lib.load()
    info = engine.EngineInfo()
    assert lib.rtm3d_engine_inspect(path.encode(), ctypes.byref(info)) != 0
    msg = lib.rtm3d_last_error().decode()
    assert msg.startswith('engine_inspect: ')
    assert re.search(why, msg), msg
    # the loader runs the same checks first: it fails with the file's reason, not at a device (there is none here)
    ctx = ctypes.c_void_p(1)
    assert lib.rtm3d_engine_load(path.encode(), 0, ctypes.byref(ctx), None) != 0
    assert ctx.value is None
    assert lib.rtm3d_last_error().decode() == 'engine_load: ' + msg[len('engine_inspect: '):]


def test_c_example_compiles_and_links(built):
    """examples/engine_detect.c through the library build's own rule (rtm3d_amd/csrc/Makefile: example), warnings as errors,
    into a fresh file: it compiles as plain C against the header and links librtm3d_hip.so and the HIP runtime only."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'engine_detect')
    if os.path.exists(exe):
        os.remove(exe)
    subprocess.run(['make', '-C', os.path.join(REPO, 'rtm3d_amd', 'csrc'), 'example', 'EXAMPLE=' + exe, 'CC=gcc -Werror'], check=True)
    assert os.path.exists(exe)
    libs = subprocess.check_output(['ldd', exe]).decode()
    assert 'librtm3d_hip.so => ' + _lib.LIB_PATH in libs and 'libamdhip64' in libs and 'python' not in libs
    # the library build makes the same program next to the library
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), 'engine_detect'))
