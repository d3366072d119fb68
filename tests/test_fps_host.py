"""Furthest point sampling and the SSG / hybrid assigners without a GPU: the float32 restatements of tests/fps_ref.py
against a thread-by-thread simulation of the reference kernel (the tie rule) and against the reference's own Python flow,
the golden file, the shim namespace, and the detector's three-way assigner dispatch."""
import copy
import glob
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as R  # noqa: E402

REF = '/root/reference'
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'mmdet3d')), reason='reference tree not present')


def test_thread_count_is_the_power_of_two_below_n():
    """the reference takes floor(log2 n) from a floating-point log; it is exact for every n that matters (the count is
    capped at 1024), so the kernel may use the position of the leading bit"""
    for n in range(1, 4097):
        assert R.n_threads(n) == min(1 << (n.bit_length() - 1), 1024), n


@pytest.mark.parametrize('n', [1, 2, 3, 5, 37, 64, 65, 100])
def test_rank_restatement_equals_the_literal_kernel(n):
    pts = R.lattice(n, seed=n)
    for m in sorted({1, 2, min(n, 7), n}):
        assert (R.fps(pts, m) == R.fps_literal(pts, m)).all(), (n, m)
    rnd = np.random.default_rng(n).standard_normal((n, 3)).astype(np.float32)
    assert (R.fps(rnd, n) == R.fps_literal(rnd, n)).all()
    mat = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(2).astype(np.float32)
    assert (R.fps_with_dist(mat, n) == R.fps_with_dist_literal(mat, n)).all()
    assert (R.fps_with_dist(mat, n) == R.fps(pts, n)).all()      # small integers: the sum is exact in any order


def test_rank_restatement_equals_the_literal_kernel_at_1500():
    pts = R.lattice(1500, seed=1500)
    assert (R.fps(pts, 6) == R.fps_literal(pts, 6)).all()


def test_ties_are_not_won_by_the_lowest_index():
    differs = {}
    for n in (37, 100, 1500):
        pts = R.lattice(n, seed=n)
        m = 6 if n == 1500 else n
        differs[n] = bool((R.fps(pts, m) != R.fps(pts, m, rank=R.lowest_index_rank(n))).any())
    assert any(differs.values()), differs


def test_more_samples_than_points_repeats_the_first_point():
    pts = np.random.default_rng(0).standard_normal((5, 3)).astype(np.float32)
    idx = R.fps(pts, 9)
    assert sorted(idx[:5]) == [0, 1, 2, 3, 4] and (idx[5:] == 0).all()
    assert (idx == R.fps_literal(pts, 9)).all()


def test_pruning_is_any_earlier_not_greedy():
    """keypoints on a line at 0, 3, 6 with thr2 = 4.01: 1 falls to 0, and 2 falls to the FALLEN 1 (a greedy filter would
    keep 2, which is 6 away from 0)"""
    pts = np.array([[0, 0, 0], [3, 0, 0], [6, 0, 0]], np.float32)
    ids, n_clusters, status = R.ssg_assign(pts, [0, 3], [[0, 1, 2]], [3], 4.01, 2.0)
    assert n_clusters == 1 and list(ids) == [0, -1, -1] and status == 0


# ----------------------------------------------------------------------------------------------------------------------
# the reference's own Python
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def reference():
    return R.load_reference_ssg()


@needs_reference
@pytest.mark.parametrize('name', list(R.FAMILIES))
def test_reference_ssg_equals_the_restated_flow_and_the_golden_file(reference, name):
    import torch
    pts, batch, num_fps, radius = R.family(name)
    g = load_golden('ssg.npz')
    assert (g[f'{name}_points'] == pts).all() and (g[f'{name}_batch'] == batch).all()
    want = reference.ssg(torch.from_numpy(pts), torch.from_numpy(batch), num_fps, radius).numpy()
    got, status = R.ssg(pts, batch, num_fps, radius)
    assert status == 0 and (got == want).all() and (g[f'{name}_ssg'] == want).all()
    # one sample on its own, and the sampled rows themselves
    one = pts[batch == 1]
    want1 = reference.ssg_single_sample(torch.from_numpy(one), num_fps, radius).numpy()
    got1, _ = R.ssg(one, np.zeros(len(one), np.int64), num_fps, radius)
    assert (got1 == want1).all()
    k = min(num_fps, len(one))
    assert (reference.fps(torch.from_numpy(one), k).numpy() == one[R.fps(one, k)]).all()


@needs_reference
@pytest.mark.parametrize('tag', ['ssgassigner', 'hybrid'])
def test_reference_assigners_equal_the_restated_flow_and_the_golden_file(reference, tag):
    import torch
    g = load_golden('ssg.npz')
    cls, cfg = {'ssgassigner': (reference.SSGAssigner, R.SSG_ASSIGNER), 'hybrid': (reference.HybridAssigner, R.HYBRID_ASSIGNER)}[tag]
    module = cls(**copy.deepcopy(cfg))
    for class_name, fam in R.CLASS_FAMILY.items():
        pts, batch, _, _ = R.family(fam)
        rows, mask = module.forward_single_class(torch.from_numpy(pts), torch.from_numpy(batch), class_name, None)
        assert (rows.numpy() == g[f'{tag}_{class_name}_rows']).all() and (mask.numpy() == g[f'{tag}_{class_name}_mask']).all()
        if tag == 'hybrid' and cfg['cfg_per_class'][class_name]['assigner_type'] == 'ccl':
            continue                                     # the ccl branch is ClusterAssigner's flow (tests/test_gpu_cluster.py)
        if tag == 'ssgassigner':
            want = R.ssg_assigner_single_class(pts, batch, cfg['cluster_voxel_size'][class_name], R.PC_RANGE,
                                               cfg['num_fps'][class_name], cfg['radius'][class_name], per_sample=False)
        else:
            c = cfg['cfg_per_class'][class_name]
            want = R.ssg_assigner_single_class(pts, batch, c['cluster_voxel_size'], R.PC_RANGE, c['num_fps'], c['radius'],
                                               per_sample=True)
        assert (rows.numpy() == want[0]).all() and (mask.numpy() == want[1]).all()


def test_golden_file_is_small_and_complete():
    g = load_golden('ssg.npz')
    assert sum(len(g[f'{name}_points']) for name in R.FAMILIES) < 5000
    assert len(g['short_points']) < R.FAMILIES['short'][3]            # takes the `num_fps >= len(points)` branch
    for name in R.FAMILIES:
        assert g[f'{name}_ssg'].max() > 10 and g[f'{name}_ssg'].min() >= -1
    for tag in ('ssgassigner', 'hybrid'):
        for class_name in R.CLASS_FAMILY:
            assert g[f'{tag}_{class_name}_rows'].shape[0] == g[f'{tag}_{class_name}_mask'].sum() > 100


# ----------------------------------------------------------------------------------------------------------------------
# library side, no GPU
# ----------------------------------------------------------------------------------------------------------------------
def test_ops_fail_loudly_on_cpu_tensors():
    import torch
    import sst_amd
    with pytest.raises(RuntimeError):
        sst_amd.furthest_point_sample(torch.zeros(1, 8, 3), 4)
    with pytest.raises(RuntimeError):
        sst_amd.furthest_point_sample_with_dist(torch.zeros(1, 8, 8), 4)
    with pytest.raises(RuntimeError):
        sst_amd.fps_segmented(torch.zeros(8, 3), torch.tensor([0, 8], dtype=torch.int32), 4)
    with pytest.raises(RuntimeError):
        sst_amd.ssg(torch.zeros(8, 3), torch.zeros(8, dtype=torch.long), 4, 1.0)


def test_shim_namespace_has_what_the_reference_module_uses():
    import re
    import sst_amd.native_shims as shims
    ns = shims.furthest_point_sample_ext
    for name in ('furthest_point_sampling_wrapper', 'furthest_point_sampling_with_dist_wrapper'):
        assert callable(getattr(ns, name))
    path = os.path.join(REF, 'mmdet3d', 'ops', 'furthest_point_sample', 'furthest_point_sample.py')
    if not os.path.exists(path):
        return
    used = set(re.findall(r'furthest_point_sample_ext\.(\w+)', open(path).read()))
    assert used and all(hasattr(ns, name) for name in used), used
    # the reference's file imports, unmodified, with the shim installed
    saved = {k: sys.modules.get(k) for k in ('_fps_pkg', '_fps_pkg.furthest_point_sample_ext')}
    try:
        pkg = types.ModuleType('_fps_pkg')
        pkg.__path__ = []
        sys.modules['_fps_pkg'] = pkg
        sys.modules['_fps_pkg.furthest_point_sample_ext'] = ns
        pkg.furthest_point_sample_ext = ns
        spec = importlib.util.spec_from_file_location('_fps_pkg.furthest_point_sample', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert callable(mod.furthest_point_sample) and callable(mod.furthest_point_sample_with_dist)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _fsd_model():
    import ast
    for path in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'configs', 'fsd', '*.model.py'))):
        model = ast.literal_eval(open(path).read())
        if model['type'] in ('SingleStageFSD', 'FSD'):
            return model
    raise AssertionError('no SingleStageFSD fixture')


def test_detector_builds_the_ssg_and_hybrid_assigners():
    import sst_amd
    model = _fsd_model()
    assert isinstance(sst_amd.build_detector(copy.deepcopy(model)).cluster_assigner, sst_amd.ClusterAssigner)
    names = model['cluster_assigner'].get('class_names', ['Car', 'Cyclist', 'Pedestrian'])
    radius = dict(cluster_voxel_size={n: [0.5, 0.5, 6] for n in names}, point_cloud_range=model['cluster_assigner']['point_cloud_range'],
                  radius={n: 1.0 for n in names}, num_fps={n: 256 for n in names}, class_names=names)
    det = sst_amd.build_detector(dict(copy.deepcopy(model), cluster_assigner=radius))
    assert type(det.cluster_assigner) is sst_amd.SSGAssigner and det.cluster_assigner.num_classes == model['bbox_head']['num_classes']
    assert det.cluster_assigner.num_fps == radius['num_fps']
    hybrid = dict(hybrid=True, point_cloud_range=model['cluster_assigner']['point_cloud_range'], class_names=names, cfg_per_class={
        n: (dict(assigner_type='ssg', cluster_voxel_size=[0.5, 0.5, 6], radius=1.0, num_fps=256) if i == 0 else
            dict(assigner_type='ccl', cluster_voxel_size=[0.5, 0.5, 6], min_points=2, connected_dist=0.6))
        for i, n in enumerate(names)})
    det = sst_amd.build_detector(dict(copy.deepcopy(model), cluster_assigner=hybrid))
    assert type(det.cluster_assigner) is sst_amd.HybridAssigner and not hasattr(det.cluster_assigner, 'hybrid')
    assert det.cluster_assigner.cfg_per_class[names[0]]['assigner_type'] == 'ssg'
