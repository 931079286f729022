"""The two launch shapes of the JPEG device stage on 32 JPEG files (the figures of profiles/jpeg.txt): rtm3d_frames_jpeg_idct - one
launch, halo chroma blocks recomputed - against tools/microbench/jpeg_two_launch.hip - two launches, sample planes in a workspace.
Builds the microbenchmark's library if it is missing, checks that both write the same bytes, then times each call between two
events, enqueued behind a matrix product of about a millisecond so that it waits in the queue; 5 interleaved rounds.

    python tools/jpeg_two_launch.py FRAMES_DIR_OR_FILE OUT.txt
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtm3d_amd import _lib, jpeg
from tools.jpeg_cost import load, B

datas = load(sys.argv[1])
infos = [jpeg.info(d) for d in datas]
dev = torch.device('cuda', 0)
bufs = [jpeg.entropy_decode(d) for d in datas]
up = [(torch.from_numpy(b).to(dev), i['h'], i['w'], i['mode']) for b, i in zip(bufs, infos)]
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, 'microbench', 'jpeg_two_launch.out')
if not os.path.exists(SO):
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-o', SO,
                           os.path.join(HERE, 'microbench', 'jpeg_two_launch.hip')])
two = ctypes.CDLL(SO)
two.two_launch.restype = ctypes.c_int
two.two_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_lib.JpegFrame), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
ws = [torch.zeros(i['coef_count'] - 192, dtype=torch.uint8, device=dev) for i in infos]
frames = jpeg.c_frames(up)
out1 = jpeg.idct(up)
out2 = [torch.zeros_like(o) for o in out1]
stream = _lib.stream_ptr(dev)
run2 = lambda: two.two_launch(stream, B, frames, dst2, wsp, 0)
dst1 = _lib.ptr_array(out1)
lib = _lib.load()
run1 = lambda: lib.rtm3d_frames_jpeg_idct(stream, B, frames, dst1, 0)
busy = torch.randn(8192, 8192, device=dev, dtype=torch.float16)
dst2, wsp = _lib.ptr_array(out2), _lib.ptr_array(ws)
assert run2() == 0
torch.cuda.synchronize()
same = all(torch.equal(a, b) for a, b in zip(out1, out2))
lines = ['two-launch output equals the one-launch output on all %d frames: %s' % (B, same)]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for rnd in range(5):
    for name, fn in (('one launch, halo blocks recomputed', run1), ('two launches, sample planes in a workspace', run2)):
        torch.cuda.synchronize(); torch.mm(busy, busy); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        lines.append('round %d  %-44s %8.1f us' % (rnd, name, e0.elapsed_time(e1) * 1e3))
text = '\n'.join(lines) + '\n'
print(text, end='')
open(sys.argv[2], 'w').write(text)
