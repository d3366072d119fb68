"""Host: the class-batched cluster assignment refuses what it does not cover before anything is launched (no GPU needed: the
argument checks of csrc/cluster_classes.hip and of sst_amd/cluster.py come first), and the opt-in switch reaches the assigners."""
import ctypes

import pytest
import torch


def params(n_classes=2, offs=(0, 3, 5), cell=1.0, dist=0.6):
    from sst_amd import _lib
    p = _lib.ClusterClassesParams()
    p.n_classes, p.per_sample, p.min_points = n_classes, 1, 2
    for i, o in enumerate(offs):
        p.class_off[i] = o
    for c in range(min(n_classes, 32)):
        for d in range(3):
            p.cell[c][d] = cell
        p.dist[c] = dist
    return p


def test_struct_matches_the_header():
    from sst_amd import _lib
    # int32 x 4, int32[33], float[32][3], float[32], float[3], int32
    assert ctypes.sizeof(_lib.ClusterClassesParams) == 4 * (4 + 33 + 96 + 32 + 3 + 1)
    assert _lib.load().sst_cluster_classes_max() == 32


def test_key_layout_fits_the_sorted_unique():
    from sst_amd import _lib
    lib = _lib.load()
    mins, ext = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    assert lib.sst_cluster_classes_key_layout(32, mins, ext) == 0
    assert list(mins) == [0, 0, -65536, -65536, -16384] and list(ext) == [32, 256, 131072, 131072, 32768]
    total = 1
    for e in ext:
        total *= e
    assert total == 1 << 62                                     # keys 1 .. 2^62: inside the 63 bits sst_unique_rows packs
    assert lib.sst_cluster_classes_key_layout(33, mins, ext) == _lib.SST_ERR_UNSUPPORTED
    assert lib.sst_cluster_classes_key_layout(0, mins, ext) == _lib.SST_ERR_ARG


@pytest.mark.parametrize('bad, code', [
    (dict(n_classes=0), 'ARG'), (dict(n_classes=33), 'UNSUPPORTED'), (dict(offs=(1, 3, 5)), 'ARG'), (dict(offs=(0, 3, 4)), 'ARG'),
    (dict(offs=(0, 6, 5)), 'ARG'), (dict(cell=0.0), 'ARG'), (dict(cell=float('nan')), 'ARG'), (dict(dist=float('nan')), 'ARG')])
def test_c_entry_points_check_their_arguments_first(bad, code):
    """every pointer is NULL: a call that got past its checks would fault, a checked one answers with the error code"""
    from sst_amd import _lib
    lib = _lib.load()
    want = getattr(_lib, 'SST_ERR_' + code)
    p = params(**bad)
    assert lib.sst_cluster_classes_keys_f32(None, 3, None, 5, ctypes.byref(p), None, None, None) == want
    assert lib.sst_cluster_classes_f32(None, None, None, None, None, None, 5, ctypes.byref(p), None, None, None, None, None, None,
                                       None) == want


def test_c_entry_points_refuse_null_buffers():
    from sst_amd import _lib
    lib = _lib.load()
    p = params()
    assert lib.sst_cluster_classes_keys_f32(None, 3, None, 5, ctypes.byref(p), None, None, None) == _lib.SST_ERR_ARG
    assert lib.sst_cluster_classes_keys_f32(None, 3, None, 5, None, None, None, None) == _lib.SST_ERR_ARG
    assert lib.sst_cluster_classes_f32(None, None, None, None, None, None, 5, ctypes.byref(p), None, None, None, None, None, None,
                                       None) == _lib.SST_ERR_ARG
    assert lib.sst_cluster_classes_workspace_bytes(0) > 0
    assert lib.sst_cluster_classes_workspace_bytes(100000) >= 12 * 4 * 100000      # twelve int32 / float vectors and the scan's


def test_python_refusals_by_name():
    from sst_amd import cluster
    p, b = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='at most 32'):
        cluster.cluster_assign_classes([p] * 33, [b] * 33, [[1, 1, 1]] * 33, [1.0] * 33, 1, [0, 0, 0], True)
    with pytest.raises(ValueError, match='sample-index lists'):
        cluster.cluster_assign_classes([p, p], [b], [[1, 1, 1]] * 2, [1.0] * 2, 1, [0, 0, 0], True)
    with pytest.raises(ValueError, match='cell size of class 1'):
        cluster.cluster_assign_classes([p, p], [b, b], [[1, 1, 1], [1, -1, 1]], [1.0] * 2, 1, [0, 0, 0], True)
    with pytest.raises(ValueError, match='not a number'):
        cluster.cluster_assign_classes([p], [b], [[1, 1, 1]], [float('nan')], 1, [0, 0, 0], True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        cluster.cluster_assign_classes([p], [b], [[1, 1, 1]], [1.0], 1, [0, 0, 0], True)


def test_enable_class_batched_reaches_every_assigner_and_nothing_else():
    import sst_amd
    from sst_amd import cluster
    rng = [-10, -10, -2, 10, 10, 2]
    a = sst_amd.ClusterAssigner((0.3, 0.3, 6), 2, rng, 0.6)
    h = sst_amd.HybridAssigner(rng, {})
    assert a.class_batched is False and not hasattr(h, 'class_batched')
    holder = torch.nn.ModuleDict(dict(a=a, h=h, inner=torch.nn.ModuleList([sst_amd.ClusterAssigner((0.3, 0.3, 6), 2, rng, 0.6)])))
    assert cluster.enable_class_batched(holder) == 2
    assert a.class_batched and holder['inner'][0].class_batched and not hasattr(h, 'class_batched')
    assert cluster.enable_class_batched(holder, on=False) == 2 and not a.class_batched
    assert sst_amd.enable_class_batched is cluster.enable_class_batched
    assert sst_amd.cluster_assign_classes is cluster.cluster_assign_classes
