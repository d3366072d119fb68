"""GPU: ``ClusterAssigner.forward`` on the tables of configs/argo2/argo_onestage_12e.py - list-valued cluster_voxel_size /
connected_dist, 26 class_names over six point lists - against the reference's own function (tests/golden/cluster_argo2.npz,
tests/golden/make_cluster_argo2.py), on the per-class path and with ``class_batched``.  The votes are multiples of 1/64, so
the centroids are the same bits whatever the order of a sum: every comparison is exact."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def assigner_cfg():
    path = os.path.join(ROOT, 'tests', 'golden', 'configs', 'argo2', 'argo_onestage_12e.model.py')
    return ast.literal_eval(open(path).read())['cluster_assigner']


@pytest.mark.parametrize('batched', [False, True])
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_cluster_assigner_on_the_argo2_tables_matches_the_reference(mode, batched):
    import sst_amd
    g = load_golden('cluster_argo2.npz')
    a = sst_amd.ClusterAssigner(**assigner_cfg())
    a.num_classes = len(a.class_names)
    assert len(a.class_names) == 26 and isinstance(a.cluster_voxel_size, list) and isinstance(a.connected_dist, list)
    a.train(mode == 'train')
    assert sst_amd.enable_class_batched(a, batched) == 1
    pts = [torch.from_numpy(g[f'in_points_{k}']).to(DEV) for k in range(6)]
    bat = [torch.from_numpy(g[f'in_batch_{k}']).to(DEV) for k in range(6)]
    inds, masks = a(pts, bat, None, None, origin_points=pts)
    assert len(inds) == len(masks) == 6                       # cut to the six lists, as the reference's multi_apply does
    for k in range(6):
        np.testing.assert_array_equal(masks[k].cpu().numpy(), g[f'{mode}_mask_{k}'])
        np.testing.assert_array_equal(inds[k].cpu().numpy(), g[f'{mode}_inds_{k}'])
        np.testing.assert_array_equal(masks[k]._sst_keep.cpu().numpy(), np.flatnonzero(g[f'{mode}_mask_{k}']))
