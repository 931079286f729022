"""Regime table of the uint8 input path (csrc/preprocess.hip, rtm3d_preprocess_batch): one named case per regime of the
kernels' schedule, the smallest shapes that reach it, and what the schedule must be for the case to be the case it names.

A case:
  canvas   (H, W)
  images   [(h, w, rh, rw)]: source size and size after Resize (equal: no resize)
  offsets  byte offset of every image's first byte from a 256-byte boundary (None: all 0)
  border   P of the fp16 NHWC4 run (every case also runs as fp32 NCHW)
  content  how the bytes are made (``make_images``): ('random', seed) or a named rule
  second   (replay only) the images of a second call into the same buffers
  expect   'refused': the call returns 1 and the error names this;  otherwise
           'plan': one tuple per sub-batch of 64, the fields of rtm3d_preprocess_plan in order
                   (first, count, col_bytes, stage_bytes, band_rows, bands, grid_x, border_grid_x),
           'bands': {(staged, unstaged, misaligned, short): number of images} - per image, over the bands of band_rows resized
                   rows: how many are staged in LDS / gather from global memory, how many staged ones start off a 16-byte
                   boundary, how many staged ones hold no whole 16-byte chunk at all,
           'upscale' / 'downscale': image axes that grow / shrink, 'full_canvas_images', 'odd_pad_images', 'multiband' (some
           workgroup takes more than one band), 'border_colours': what else the regime is about (checked in tests/test_preprocess_regimes.py).
The numbers are the launcher's arithmetic at the time the table was written; tests/test_preprocess_regimes.py compares them with
rtm3d_preprocess_batch_plan and with a count made from the oracle's own row coefficients, so a case that no longer runs in the
regime it is named after fails."""
import numpy as np

from oracle import preprocess_ref

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL16 = 0x7BCD            # a finite fp16 (62880) no table entry comes near; sentinel of the NHWC4 buffer


def _same(h, w):
    return (h, w, h, w)


CASES = {
    'multiband_up2': dict(
        canvas=(544, 16), images=[(265, 5, 530, 10), _same(530, 8)] * 32, border=3, content=('random', 101),
        expect=dict(plan=[(0, 64, 80, 49152, 16, 34, 32, 18)], bands={(34, 0, 33, 0): 32, (34, 0, 0, 0): 32}, multiband=True, upscale=64)),
    'unstaged_wide': dict(
        canvas=(64, 1504), images=[(300, 9000, 50, 1500), (40, 60, 50, 75)], border=3, content=('random', 102),
        expect=dict(plan=[(0, 2, 12000, 45344, 1, 50, 50, 256)], bands={(0, 50, 0, 0): 1, (50, 0, 39, 0): 1}, upscale=2, downscale=2)),
    'widest_table': dict(
        canvas=(2, 7500), images=[_same(1, 7500)], border=1, content=('random', 103),
        expect=dict(plan=[(0, 1, 60000, 0, 1, 1, 1, 30)], bands={(0, 1, 0, 0): 1}, odd_pad_images=1)),
    'table_refused': dict(
        canvas=(2, 7504), images=[_same(1, 7501)], border=1, content=('random', 104),
        expect=dict(refused='resized width 7501 exceeds')),
    'subbatches_70': dict(
        canvas=(16, 24), images=[_same(3 + i % 9, 3 + i % 17) for i in range(70)], border=1, content=('random', 105),
        expect=dict(plan=[(0, 64, 160, 49152, 16, 1, 1, 2), (64, 6, 160, 49152, 16, 1, 1, 2)], bands={(1, 0, 0, 0): 70})),
    'anisotropic': dict(
        canvas=(64, 96), images=[(37, 53, 61, 40), (90, 31, 30, 93), (20, 200, 64, 96)], border=0, content=('random', 106),
        expect=dict(plan=[(0, 3, 768, 49152, 16, 4, 4, 15)], bands={(4, 0, 3, 0): 1, (2, 0, 2, 0): 1, (4, 0, 1, 0): 1}, upscale=3, downscale=3,
                    full_canvas_images=1)),
    'misaligned': dict(
        canvas=(24, 32), images=[_same(1, 1), (2, 2, 5, 7), _same(1, 5), (23, 37, 11, 19), _same(9, 21), (13, 7, 20, 29)],
        offsets=[1, 3, 7, 8, 13, 15], border=3, content=('random', 107),
        expect=dict(plan=[(0, 6, 240, 49152, 16, 2, 2, 3)], bands={(1, 0, 1, 1): 3, (1, 0, 1, 0): 2, (2, 0, 2, 0): 1}, upscale=4,
                    downscale=2)),
    'odd_pads': dict(
        canvas=(17, 22), images=[_same(10, 15), _same(17, 9), _same(6, 22), (30, 40, 12, 17)], border=1, content=('random', 108),
        expect=dict(plan=[(0, 4, 176, 49152, 16, 2, 2, 1)], bands={(1, 0, 0, 0): 3, (2, 0, 0, 0): 1}, odd_pad_images=4,
                    downscale=2)),
    'mean_edges': dict(
        canvas=(8, 12), images=[_same(4, 6)] * 4, border=0, content='mean_edges',
        expect=dict(plan=[(0, 4, 48, 49152, 16, 1, 1, 1)], bands={(1, 0, 0, 0): 4},
                    border_colours=[(255, 255, 255), (80, 0, 174), (7, 100, 200), (7, 100, 200)])),
    'full_canvas_all': dict(
        canvas=(12, 20), images=[_same(12, 20), (5, 9, 12, 20), (30, 50, 12, 20)], border=1, content=('random', 110),
        expect=dict(plan=[(0, 3, 160, 49152, 16, 1, 1, 0)], bands={(1, 0, 0, 0): 3}, full_canvas_images=3, upscale=2, downscale=2)),
    'replay': dict(
        canvas=(16, 24), images=[_same(10, 14), (6, 20, 12, 9)], second=[_same(4, 5), (16, 24, 8, 12)], border=0, content='replay',
        expect=dict(plan=[(0, 2, 112, 49152, 16, 1, 1, 2)], plan_second=[(0, 2, 96, 49152, 16, 1, 1, 2)], bands={(1, 0, 0, 0): 2}, upscale=1, downscale=1)),
}
# the fp16 NHWC4 runs use every border the network's input tensors have had
assert {c['border'] for c in CASES.values()} == {0, 1, 3}
assert all(CASES[n]['border'] == 3 for n in ('multiband_up2', 'unstaged_wide', 'misaligned'))

PLAN_FIELDS = ('first', 'count', 'col_bytes', 'stage_bytes', 'band_rows', 'bands', 'grid_x', 'border_grid_x')


def offsets(case):
    return case.get('offsets') or [0] * len(case['images'])


def make_images(case, call=0):
    """The uint8 (h, w, 3) source images of a case (of its second call: call=1), as numpy arrays."""
    shapes = case['second'] if call else case['images']
    rule = case['content']
    if rule == 'mean_edges':
        (h, w), n = shapes[0][:2], shapes[0][0] * shapes[0][1]
        ramp = (np.arange(n) * 7 % 256).astype(np.uint8).reshape(h, w)
        one_zero = np.stack([ramp, np.zeros_like(ramp), 255 - ramp], 2)                      # sums 1932, 0, 4188 over 24 pixels
        k = np.array([7, 100, 200], np.int64)
        exact = np.empty((h, w, 3), np.uint8)                                                # sum = k * npix exactly
        exact.reshape(n, 3)[0::2] = k - 5
        exact.reshape(n, 3)[1::2] = k + 5
        below = np.empty((h, w, 3), np.uint8)                                                # sum = (k + 1) * npix - 1
        below[:] = k + 1
        below[h // 2, w // 2] = k
        return [np.full((h, w, 3), 255, np.uint8), one_zero, exact, below]
    if rule == 'replay':            # bright first, dark second: a channel sum left over from the first call would show in the border
        rng = np.random.Generator(np.random.PCG64(109 + call))
        lo, hi = ((0, 56) if call else (200, 256))
        return [rng.integers(lo, hi, size=(h, w, 3), dtype=np.uint8) for h, w, _, _ in shapes]
    rng = np.random.Generator(np.random.PCG64(int(rule[1])))
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w, _, _ in shapes]


def pack(case, imgs):
    """One uint8 buffer holding every image at (a multiple of 256) + its offset, and the positions.  The caller puts the buffer
    on a 256-byte boundary (any fresh device allocation), then image i is ``buf[pos[i] : pos[i] + h * w * 3].view(h, w, 3)``."""
    pos, at = [], 0
    for img, o in zip(imgs, offsets(case)):
        pos.append(at + o)
        at = (at + o + img.size + 255) // 256 * 256
    buf = np.zeros(max(at, 1), np.uint8)
    for img, p in zip(imgs, pos):
        buf[p:p + img.size] = img.reshape(-1)
    return buf, pos


def band_stats(shape, offset, band_rows, stage_bytes):
    """(staged, unstaged, misaligned, short) band counts of one image (see the module docstring), from the plan's numbers and the
    oracle's row coefficients: the band of resized rows r0 .. r1 - 1 reads source rows y0[r0] .. y1[r1 - 1], one contiguous span."""
    h, w, rh, rw = shape
    if (rh, rw) == (h, w):
        y0 = y1 = np.arange(h)
    else:
        y0, y1, _, _ = preprocess_ref._resize_coef(rh, h)
    staged = unstaged = misaligned = short = 0
    for r0 in range(0, rh, band_rows):
        r1 = min(r0 + band_rows, rh)
        ylo, yhi = int(y0[r0]), int(y1[r1 - 1])
        span = (yhi - ylo + 1) * w * 3
        if span + 15 <= stage_bytes:
            staged += 1
            a = (offset + ylo * w * 3) % 16
            misaligned += a != 0
            short += (a + 15) // 16 * 16 + 16 > a + span             # no 16-byte chunk lies wholly inside the span
        else:
            unstaged += 1
    return staged, unstaged, misaligned, short


def oracle_canvases(case, imgs, call=0):
    """Per image: (uint8 (H, W, 3) letterboxed canvas, integer channel sums of the resized image) - the oracle alone."""
    H, W = case['canvas']
    out = []
    for img, (h, w, rh, rw) in zip(imgs, case['second'] if call else case['images']):
        small = preprocess_ref.resize_bilinear_u8(img, (rh, rw))
        canvas, _, _ = preprocess_ref.apply_padding(small, (W, H))
        out.append((canvas, small.reshape(-1, 3).astype(np.int64).sum(0)))
    return out
