"""The case table of the pixel-format tests and a seeded builder of source planes (padding bytes hold random data; a plane's
buffer ends with the last row's own bytes: no pitch padding behind it).

The thread mapping the sizes are chosen against (rtm3d_frames_convert_plan; tests/test_pixfmt_cpu.py pins these numbers): a
thread takes G = 8 pixels of R = 2 rows, a workgroup T = 256 such runs in row-major order of the frame's runs, a launch 32
frames."""
import numpy as np

from tests import pixfmt_ref as ref

G, R, T, CHUNK = 8, 2, 256, 32

# the issue's list
SMALL = [(1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (7, 33), (2, 129)]
# either side of the run: widths around G (and two runs plus one), heights around R
RUN_EDGES = [(h, w) for h in (R - 1, R, R + 1) for w in (G - 1, G, G + 1, 2 * G + 1)]
# either side of the workgroup: 255, 256, 257 runs in one row pair, and as 255, 256, 257 row pairs of one run
BLOCK_EDGES = [(2, G * T - G), (2, G * T), (2, G * T + 1), (2 * T - 2, G), (2 * T, G), (2 * T + 1, G)]
# rows whose every run is whole and aligned at base offset 0 (the wide loads and stores), next to one that is not
WIDE = [(4, 16), (3, 24), (5, 40), (7, 33)]
SIZES = SMALL + RUN_EDGES + BLOCK_EDGES
# the store of a run (csrc/rgb_runs.h) at the destination addresses base_offsets() leaves to the luck of an odd width: a row of
# three whole runs is 72 bytes, so every run keeps the base's alignment - 2 modulo 4 (the shifted store), 4 modulo 8 (dword
# but not 8-byte stores) - and a row of 21 pixels ends in a partial run and walks the addresses through every residue
STORE_SIZES = [(3, 24), (3, 21)]
STORE_OFFSETS = (2, 4)

MATRIX_RANGE = [(m, r) for m in ('bt601', 'bt709') for r in ('limited', 'full')]


def variants(fmt):
    """(matrix, range) combinations that matter for a format."""
    return MATRIX_RANGE if fmt in ref.YUV else [('bt601', 'limited')]


def pitch_steps(fmt):
    """minimal, minimal + 1 (P010: + 2, its pitch must be even), minimal + 64"""
    return (0, 2, 64) if fmt == 'p010' else (0, 1, 64)


def base_offsets(fmt):
    return (0, 2) if fmt == 'p010' else (0, 1, 3)


def build_source(fmt, h, w, rng, extra_pitch=0, matrix='bt601', range='limited'):
    """A source dict of tests/pixfmt_ref.py with random bytes everywhere, the padding included."""
    planes, pitches = [], []
    for row_bytes, rows in ref.layout(fmt, h, w):
        pitch = row_bytes + extra_pitch
        planes.append(rng.integers(0, 256, (rows - 1) * pitch + row_bytes, dtype=np.uint8))
        pitches.append(pitch)
    return {'format': fmt, 'h': h, 'w': w, 'planes': planes, 'pitches': pitches, 'matrix': matrix, 'range': range}


def expected_runs(h, w):
    return ((w + G - 1) // G) * ((h + R - 1) // R)
