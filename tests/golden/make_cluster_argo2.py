"""Generates tests/golden/cluster_argo2.npz: ``ClusterAssigner.forward`` as the REFERENCE computes it on the tables of
configs/argo2/argo_onestage_12e.py - list-valued ``cluster_voxel_size`` / ``connected_dist`` and the 26 ``class_names`` over
SIX point lists (data only).  Those tables work in the reference because ``multi_apply`` stops at the shortest of its lists and
the first six names index the six table rows.

Needs the reference tree (oracle.ref_loader) and scipy; run from the repository root:  python tests/golden/make_cluster_argo2.py

Executed from their source text on the CPU (mmdet3d/models/detectors/single_stage_fsd.py): the class ClusterAssigner,
filter_almost_empty, find_connected_componets, find_connected_componets_single_batch, modify_cluster_by_class.  Stood in for:
  multi_apply   mmdet's: map the function over the zipped lists, transpose the results
  scatter_v2    ('avg', return_inv) the mean of the rows of every group of torch.unique(coors, dim=0), in float64 rounded to
                float32 - with the inputs below (multiples of 1/64, below 256 in magnitude) every float32 sum is exact in any
                order, so this is also what any float32 summation gives
The tables come from the fixture tests/golden/configs/argo2/argo_onestage_12e.model.py."""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SS_PY = 'mmdet3d/models/detectors/single_stage_fsd.py'
# (votes, objects, scatter in metres) per group: dense enough that voxels of 5 cm keep two votes
GROUPS = [(1500, 40, 0.35), (700, 30, 0.03), (600, 30, 0.05), (900, 12, 0.6), (500, 20, 0.06), (40, 3, 0.05)]
SAMPLES = 3


def multi_apply(func, *args, **kwargs):
    results = map(func, *args)
    return tuple(map(list, zip(*results)))


def scatter_avg(feat, coors, mode, return_inv=True):
    assert mode == 'avg' and return_inv
    new_coors, inv = torch.unique(coors, return_inverse=True, dim=0)
    sums = torch.zeros((new_coors.size(0), feat.size(1)), dtype=torch.float64).index_add_(0, inv, feat.double())
    cnt = torch.bincount(inv, minlength=new_coors.size(0)).double()
    return (sums / cnt[:, None]).float(), new_coors, inv


def reference_assigner(cfg):
    from scipy.sparse.csgraph import connected_components
    from oracle import ref_loader
    glb = {'connected_components': connected_components}
    fns = {name: ref_loader.load_reference_function(SS_PY, name, glb)
           for name in ('filter_almost_empty', 'find_connected_componets', 'find_connected_componets_single_batch',
                        'modify_cluster_by_class')}
    cls = ref_loader.load_reference_class(SS_PY, 'ClusterAssigner', dict(fns, multi_apply=multi_apply, scatter_v2=scatter_avg))
    a = cls(**cfg)
    a.num_classes = len(cfg['class_names'])          # the detector sets it (single_stage_fsd.py:418)
    return a


def votes(seed):
    rng = np.random.default_rng(seed)
    pts, bat = [], []
    for n, objects, sigma in GROUPS:
        centres = rng.uniform(-100, 100, (SAMPLES, objects, 2))
        b = np.sort(rng.integers(0, SAMPLES, n))
        xy = centres[b, rng.integers(0, objects, n)] + rng.normal(0, sigma, (n, 2))
        p = np.concatenate([xy, rng.uniform(-1, 1, (n, 1))], 1)
        pts.append((np.round(p * 64) / 64).astype(np.float32).reshape(-1, 3))
        bat.append(b.astype(np.int64))
    return pts, bat


def main():
    model = ast.literal_eval(open(os.path.join(ROOT, 'tests', 'golden', 'configs', 'argo2', 'argo_onestage_12e.model.py')).read())
    cfg = model['cluster_assigner']
    assert isinstance(cfg['cluster_voxel_size'], list) and isinstance(cfg['connected_dist'], list) and len(cfg['class_names']) == 26
    a = reference_assigner(cfg)
    pts, bat = votes(26)
    assert all(float(np.abs(p).max()) < 256 for p in pts if len(p))
    out = {}
    for g, (p, b) in enumerate(zip(pts, bat)):
        out[f'in_points_{g}'], out[f'in_batch_{g}'] = p, b
    for mode in ('train', 'eval'):
        a.train(mode == 'train')
        inds, masks = a([torch.from_numpy(p) for p in pts], [torch.from_numpy(b) for b in bat], None, None, [None] * len(pts))
        assert len(inds) == len(masks) == 6
        for g in range(6):
            out[f'{mode}_inds_{g}'], out[f'{mode}_mask_{g}'] = inds[g].numpy(), masks[g].numpy()
        print(mode, 'kept', [int(m.sum()) for m in masks], 'clusters', [int(i[:, 2].max()) + 1 if len(i) else 0 for i in inds])
    path = os.path.join(ROOT, 'tests', 'golden', 'cluster_argo2.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
