#!/usr/bin/env python3
"""Golden vectors for the label half of the training augmentation, produced by RUNNING the reference's own code:
`TrainAugmentation` (preprocess/data_preprocess.py), `ParamList` (utils/ParamList.py), `DatasetReader._transform_obj_label`
and `DatasetReader._apply_padding` (datasets/dataset_reader.py).  Run only where the reference tree is at hand:

    cd /tmp && python -B <repo>/tests/golden/make_golden_augment.py <reference root>

Modules the image lacks are stubbed in sys.modules (no reference source is copied): torchvision, the external KITTI devkit,
albumentations - identity callables, which draw nothing - and cv2, whose `mean`, `resize` and `warpAffine` do size bookkeeping
only (the pixels are not pinned: OpenCV is absent); the `warpAffine` stub records the matrix it is given, which is how the
reference's own (scale, offset) reach the file.  numpy.random is seeded, the chain is run, then the generator is re-seeded and
the draws are replayed in the chain's order (RandomAffine: randint(2), then uniform(1, 1.2) and random_sample(2) if it fired;
RandomMirror: randint(2)) to recover (affine fired, scale, flip).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit('usage: make_golden_augment.py <reference root>')
sys.path.insert(0, sys.argv[1])

import numpy as np  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


WARPS = []


def _warp(image, M, dsize, borderValue=None):
    WARPS.append(np.array(M, np.float64))
    return np.zeros((dsize[1], dsize[0], image.shape[2]), image.dtype)


def _identity(p=0.5):
    return lambda image: {'image': image}


tv = _stub('torchvision'); tvt = _stub('torchvision.transforms', ToTensor=lambda: None); tv.transforms = tvt
_stub('albumentations', RandomBrightnessContrast=_identity, GaussNoise=_identity)
_stub('cv2', mean=lambda img: tuple(np.asarray(img, np.float64).reshape(-1, img.shape[2]).mean(axis=0)) + (0.0,) * (4 - img.shape[2]),
      INTER_LINEAR=1, resize=lambda src, dsize, interpolation: np.zeros((dsize[1], dsize[0], src.shape[2]), src.dtype), warpAffine=_warp)
for n in ('datasets.data', 'datasets.data.kitti', 'datasets.data.kitti.devkit_object', 'datasets.data.kitti.devkit_object.utils'):
    _stub(n)
sys.modules['datasets.data.kitti.devkit_object'].utils = sys.modules['datasets.data.kitti.devkit_object.utils']

from preprocess.data_preprocess import TrainAugmentation   # noqa: E402 (reference)
from datasets.dataset_reader import DatasetReader          # noqa: E402 (reference)
from utils.ParamList import ParamList                      # noqa: E402 (reference)

# the numbering of the type names is this file's (the devkit that owns the reference's is absent); OBJs and RELATE_OBJs are the
# reference's defaults (models/configs/detault.py)
NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck', 'Person_sitting', 'Tram', 'Misc', 'DontCare']
OBJS, RELATE = ['Car', 'Pedestrian', 'Cyclist'], [['Van', 'Truck'], ['Person_sitting'], ['Person_sitting']]
MEAN = [0.485, 0.456, 0.406]
K0 = np.array([721.5377, 0, 609.5593, 0, 721.5377, 172.854, 0, 0, 1.0])


def rows_for(case, h, w, rng):
    """(n, 15) float64: type index, truncated, occluded, alpha, x1 y1 x2 y2, h w l, x y z, ry."""
    rows = []

    def add(t, x1, y1, x2, y2, ry):
        rows.append([NAMES.index(t), 0.0, 0.0, float(rng.uniform(-3, 3)), x1, y1, x2, y2, *rng.uniform(1.2, 4.5, 3), float(rng.uniform(-20, 20)),
                     float(rng.uniform(0.5, 2.0)), float(rng.uniform(4, 60)), ry])

    def box(cx, cy, bw, bh):
        return cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2

    types_ = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck', 'Person_sitting', 'Tram', 'DontCare']
    for k in range(int(rng.integers(2, 6))):
        t = types_[int(rng.integers(0, len(types_)))]
        add(t, *box(rng.uniform(0.15, 0.85) * w, rng.uniform(0.2, 0.8) * h, rng.uniform(6, 0.2 * w), rng.uniform(6, 0.3 * h)), float(rng.uniform(-np.pi, np.pi)))
    add('Car', *box(0.5 * w, 0.5 * h, 0.1 * w, 0.2 * h), [0.0, 1.25, -2.5][case % 3])            # Ry of both signs and 0; always survives
    add('Van', *box(0.4 * w, 0.6 * h, 0.12 * w, 0.2 * h), float(rng.uniform(-np.pi, np.pi)))     # a noise row of class 0 (RELATE_OBJs)
    add('Person_sitting', *box(0.6 * w, 0.55 * h, 0.05 * w, 0.25 * h), float(rng.uniform(-np.pi, np.pi)))   # in two lists: the row is doubled
    if case % 2 == 0:
        add('Car', *box(0.3 * w, 0.4 * h, 1.5, 0.2 * h), 0.3)                                    # narrower than 2 px
        add('Pedestrian', *box(0.7 * w, 0.4 * h, 8.0, 2.0), -0.3)                                # exactly 2 px high: removed too
    if case % 4 < 2:
        add('Cyclist', *box(0.004 * w, 0.5 * h, 0.006 * w + 3, 0.2 * h), 2.0)                    # its centre leaves under any zoom > 1.01
    add('Car', *box(0.5 * w, 0.012 * h, 0.1 * w, 0.02 * h + 3), -1.0)                            # the same through the top edge
    return np.array(rows, np.float64)


# (h, w, resize_to, (H, W)): frames that need Resize (up and down) and frames that do not
FRAMES = [(375, 1242, 1280, (1280, 1280)), (370, 1280, 1280, (384, 1280)), (376, 1241, 640, (640, 640)), (96, 320, 320, (128, 352)),
          (480, 640, 416, (416, 416)), (370, 1224, 1224, (384, 1280))]
out = {'names': np.array(NAMES), 'objs': np.array(OBJS), 'mean': np.array(MEAN), 'K0': K0,
       'relate': np.array(['|'.join(r) for r in RELATE])}
combos, n_cases = set(), 24
for case in range(n_cases):
    h, w, resize_to, (H, W) = FRAMES[case % len(FRAMES)]
    seed = 1000 + case
    rows = rows_for(case, h, w, np.random.Generator(np.random.PCG64(seed)))
    fake = types.SimpleNamespace(_classes=[NAMES.index(n) for n in OBJS], _relate_classes=[[NAMES.index(n) for n in r] for r in RELATE],
                                 _img_size=(W, H))
    cls, noise, repeats = DatasetReader._transform_obj_label(fake, rows[:, 0].copy())
    lab = np.repeat(rows, repeats=repeats, axis=0)
    N = len(cls)
    tgt = ParamList((w, h))
    tgt.add_field('class', cls)
    tgt.add_field('img_id', np.zeros((N,), dtype=np.int64))
    tgt.add_field('bbox', lab[:, 4:8].copy())
    tgt.add_field('dimension', lab[:, 8:11].copy())
    tgt.add_field('alpha', lab[:, 3].copy())
    tgt.add_field('Ry', lab[:, 14].copy())
    tgt.add_field('location', lab[:, 11:14].copy())
    mask = np.ones((N,), dtype=np.int64)
    mask[cls == -1] = 0
    tgt.add_field('mask', mask)
    tgt.add_field('noise_mask', noise)
    tgt.add_field('K', np.repeat(K0.copy().reshape(1, 9), repeats=N, axis=0))
    del WARPS[:]
    np.random.seed(seed)
    img, tgt = TrainAugmentation(resize_to, MEAN)(np.zeros((h, w, 3), np.uint8), targets=tgt)
    rh, rw = img.shape[:2]
    _, tgt = DatasetReader._apply_padding(fake, [np.ascontiguousarray(img)], [tgt])
    # replay
    np.random.seed(seed)
    fired = int(np.random.randint(2))
    scale, u = 1.0, np.zeros(2)
    if fired:
        scale = np.random.uniform(1., 1.2)
        u = np.random.random_sample((2,))
    flip = int(np.random.randint(2))
    assert len(WARPS) == fired
    offset = np.zeros(2)
    if fired:
        assert WARPS[0][0, 0] == scale and WARPS[0][1, 1] == scale and WARPS[0][0, 1] == 0 and WARPS[0][1, 0] == 0
        offset = WARPS[0][:, 2].copy()
    combos.add((fired, flip))
    p = 'c%02d_' % case
    out[p + 'frame'] = np.array([h, w, resize_to, H, W, rh, rw])
    out[p + 'rows'] = rows
    out[p + 'draw'] = np.array([fired, scale, offset[0], offset[1], flip])
    for f in ('bbox', 'K', 'Ry', 'location', 'mask', 'class', 'noise_mask', 'dimension'):
        out[p + f] = np.asarray(tgt.get_field(f))
    assert len(out[p + 'bbox']) >= 1
out['n_cases'] = np.array(n_cases)
assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}, combos
path = os.path.join(HERE, 'augment_cases.npz')
np.savez_compressed(path, **out)
print('ok', n_cases, 'cases', os.path.getsize(path), 'bytes', sorted(combos))
