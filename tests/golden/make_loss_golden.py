#!/usr/bin/env python
"""Reference-run fixture of the validation loss: tests/golden/loss_cases.npz.

    python tests/golden/make_loss_golden.py <root of the reference checkout>

RUNS the reference on the CPU for every case of tests/loss_cases.FIXTURE_CASES and stores what it returns; this script
contains no reference source and derives no target field itself.  Per image it hands the case's label arrays to the
reference's own DatasetReader._build_targets (datasets/dataset_reader.py:215-291, called unbound on a stand-in for the reader:
the method reads four attributes of it), joins the images the way a batch is joined (concatenation, img_id = the image), and
gives the result to the reference's RTM3DLoss.__call__ (models/rtm3d_loss.py:268-340) - once with fp32 tensors, as train.py
does, and once with every tensor .double().  The distance between the two runs is the reference's own precision on the case.
bbox_center and dynamic_radius (utils/data_utils.py) are called once more for the centres, sigma and radius, which
_build_targets does not return.

What has to stand in for missing pieces: modules the reference imports but never reaches on this path are empty stubs
(torchvision + .ops, .models, .transforms, cv2, albumentations); the aliases np.long and np.float, which the reference's numpy
had, are set; and the KITTI devkit module, which the reference's tree does not contain, is a stub whose one function
_build_targets calls, calc_proj2d_bbox3d, is answered from the reference's own utils/model_utils.py: the corners of the box
centred at Y - h / 2 through calc_proj_corners, mask_3d as "all eight of create_corners' corners have z > 0".  That function
is therefore the one place where the fixture holds this project's reading and not the reference's behaviour (the header says
"parity unpinned")."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import loss_cases  # noqa: E402


def import_reference(root):
    for n in ('torchvision', 'torchvision.ops', 'torchvision.models', 'torchvision.transforms', 'cv2', 'albumentations',
              'datasets.data.kitti.devkit_object'):
        sys.modules[n] = types.ModuleType(n)
    for sub in ('ops', 'models', 'transforms'):
        setattr(sys.modules['torchvision'], sub, sys.modules['torchvision.' + sub])
    devkit = types.ModuleType('utils')
    sys.modules['datasets.data.kitti.devkit_object'].utils = devkit
    for alias, t in (('long', np.int64), ('float', float)):
        if not hasattr(np, alias):
            setattr(np, alias, t)
    sys.path.insert(0, root)
    from utils import data_utils, model_utils
    from utils.ParamList import ParamList
    from models.rtm3d_loss import RTM3DLoss
    from datasets.dataset_reader import DatasetReader

    def calc_proj2d_bbox3d(dimensions, locations, Rys, Ks):
        """The missing devkit call: (N, 2, 9) projected corners (the ninth is the centre), None, (N,) mask_3d."""
        n = len(Rys)
        verts, front = np.zeros((n, 2, 9)), np.zeros(n, bool)
        for i in range(n):
            centre = np.asarray(locations[i], np.float64) - np.array([0.0, dimensions[i][0] / 2, 0.0])
            verts[i] = np.asarray(model_utils.calc_proj_corners(dimensions[i], centre, Rys[i], Ks[i])).T
            front[i] = bool((np.asarray(model_utils.create_corners(dimensions[i], centre, model_utils.rotation_matrix(Rys[i])))[2, :8] > 0).all())
        return verts, None, front

    devkit.calc_proj2d_bbox3d = calc_proj2d_bbox3d
    return data_utils, ParamList, RTM3DLoss, DatasetReader


def config(alpha, beta):
    ns = types.SimpleNamespace
    return ns(MODEL=ns(FOCAL_LOSS_ALPHA=alpha, FOCAL_LOSS_BEDA=beta, DOWN_SAMPLE=4.),
              DATASET=ns(GAUSSIAN_SIGMA_MAX=19, GAUSSIAN_SIGMA_MIN=3, BBOX_AREA_MAX=1e5, BBOX_AREA_MIN=10, VERTEX_OFFSET_INFER=[0.75, 0.57],
                         GAUSSIAN_GEN_TYPE='dynamic_radius'),
              TRAINING=ns(W_MKF=1., W_VKF=1., W_VFM=1., W_M_OFF=0.5, W_V_OFF=0.5))


FIELDS = ('m_proj', 'm_off', 'v_proj', 'v_off', 'v_coor_off', 'v_mask', 'mask_3d', 'm_hm')


def main(root):
    data_utils, ParamList, RTM3DLoss, DatasetReader = import_reference(root)
    out = {}
    for name in loss_cases.FIXTURE_CASES:
        c = loss_cases.make(name)
        B, H, W, N = c['B'], c['H'], c['W'], len(c['cls'])
        cfg = config(c['alpha'], c['beta'])
        reader = types.SimpleNamespace(_img_size=(W * 4, H * 4), _config=cfg, _classes=list(range(c['C'])), is_training=False)
        parts = {f: [] for f in FIELDS}
        for b in range(B):
            rows = np.flatnonzero(c['img_id'] == b)
            labels = ParamList(reader._img_size, is_training=False)
            for field, v in (('img_id', c['img_id'][rows]), ('mask', (c['cls'][rows] >= 0).astype(np.int64)),
                             ('noise_mask', c['noise'][rows].astype(np.int64)), ('class', c['cls'][rows].astype(np.int64)),
                             ('bbox', c['bbox'][rows].copy()), ('dimension', c['dim'][rows].copy()), ('location', c['loc'][rows].copy()),
                             ('Ry', c['ry'][rows].copy()), ('K', np.tile(c['K'][b], (len(rows), 1)))):
                labels.add_field(field, v)
            built = DatasetReader._build_targets(reader, labels)
            for f in FIELDS:
                parts[f].append(np.asarray(built.get_field(f)))
        tg = {f: np.concatenate(parts[f], 0) for f in FIELDS}
        tg.update(img_id=c['img_id'], mask=c['cls'] >= 0, noise_mask=c['noise'] != 0)
        boxes = c['bbox'] / cfg.MODEL.DOWN_SAMPLE
        centers = data_utils.bbox_center(boxes) if N else np.zeros((0, 2))
        sigma, radius = data_utils.dynamic_radius(boxes) if N else (np.zeros(0), np.zeros(0))
        logits = loss_cases.logits(c)
        items = {}
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            t = ParamList(reader._img_size)
            for k, v in tg.items():
                v = torch.from_numpy(np.ascontiguousarray(v))
                t.add_field(k, v.to(dt) if v.is_floating_point() else v)
            pred = [torch.from_numpy(a).to(dt).clone() for a in logits]
            loss, li = RTM3DLoss(cfg)(pred, t)
            assert torch.equal(loss.detach().to(li.dtype), li[4]) or (torch.isnan(loss) and torch.isnan(li[4]))
            items[tag] = li.double().numpy()
        out.update({name + '/' + f: tg[f] for f in FIELDS})
        out.update({name + '/centers': centers, name + '/sigma': sigma, name + '/radius': radius, name + '/items_f32': items['f32'],
                    name + '/items_f64': items['f64']})
        print(name, 'N', N, 'f32', items['f32'], 'f64', items['f64'], '|f32 - f64|', np.abs(items['f32'] - items['f64']))
    path = os.path.join(HERE, 'loss_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
