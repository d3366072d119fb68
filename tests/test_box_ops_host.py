"""Rotated-box ops without a GPU: the float32 restatement of the reference's BEV polygon arithmetic (tests/box_ops_ref.py)
against an independent float64 clip and analytic cases, the reference's own known-answer values
(tests/golden/box_ops_kat.npz), and the shim namespaces that stand for iou3d_cuda / roiaware_pool3d_ext / TorchEx."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_ops_ref as R  # noqa: E402

F32 = np.float32


def box(cx, cy, w, h, r=0.0):
    return np.array([[cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, r]], F32)


def test_f32_restatement_agrees_with_float64_clip():
    a, b = R.random_pairs(2500, 0)
    got = R.bev_iou_f32(a, b)
    want = np.array([R.bev_iou_f64(x, y) for x, y in zip(a.astype(np.float64), b.astype(np.float64))])
    gap = np.abs(got.astype(np.float64) - want)
    assert (want > 0.05).sum() > 1000  # the pairs really overlap
    print(f'largest float32 - float64 BEV IoU gap over {len(a)} pairs: {gap.max():.3e}')
    assert gap.max() <= R.F32_IOU_NOISE
    # overlap areas too (relative to the smaller box)
    area = R.bev_overlap_f32(a, b)
    want_area = np.array([R.bev_overlap_f64(x, y) for x, y in zip(a.astype(np.float64), b.astype(np.float64))])
    small = np.minimum((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    assert (np.abs(area - want_area) / small).max() < 1e-4


def test_early_out_never_changes_a_result():
    """the kernel returns 0 at once for pairs whose circumscribed circles are apart by more than 1 cm + 0.1 %; the full
    algorithm (the restatement has no early out) gives exactly 0 for every such pair, also just beyond the margin"""
    rng = np.random.default_rng(1)
    n = 4000
    sa, sb = rng.uniform(0.3, 20, (n, 2)), rng.uniform(0.3, 20, (n, 2))
    ra, rb = 0.5 * np.hypot(sa[:, 0], sa[:, 1]), 0.5 * np.hypot(sb[:, 0], sb[:, 1])
    ca = rng.uniform(-75, 75, (n, 2))
    phi = rng.uniform(-np.pi, np.pi, n)
    dist = (ra + rb) * rng.uniform(0.97, 1.01, n) + rng.uniform(0, 2e-2, n)
    cb = ca + dist[:, None] * np.column_stack([np.cos(phi), np.sin(phi)])
    a = np.column_stack([ca - sa / 2, ca + sa / 2, rng.uniform(-np.pi, np.pi, n)]).astype(F32)
    b = np.column_stack([cb - sb / 2, cb + sb / 2, rng.uniform(-np.pi, np.pi, n)]).astype(F32)
    # the kernel's test, in float32
    wa, ha, wb, hb = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    r = F32(0.5) * (np.sqrt(wa * wa + ha * ha) + np.sqrt(wb * wb + hb * hb))
    reach = r * F32(1.001) + F32(1e-2)
    dx = (a[:, 0] + a[:, 2]) / F32(2) - (b[:, 0] + b[:, 2]) / F32(2)
    dy = (a[:, 1] + a[:, 3]) / F32(2) - (b[:, 1] + b[:, 3]) / F32(2)
    apart = dx * dx + dy * dy > reach * reach
    assert 100 < apart.sum() < n
    assert (R.bev_overlap_f32(a[apart], b[apart]) == 0).all()


def test_analytic_cases():
    # axis-aligned closed form
    a, b = box(0, 0, 4, 2), box(1, 0.5, 4, 2)
    inter = 3 * 1.5
    assert abs(R.bev_overlap_f32(a, b)[0] - inter) < 1e-5
    assert abs(R.bev_iou_f32(a, b)[0] - inter / (16 - inter)) < 1e-6
    assert abs(R.axis_iou_f32(a, b)[0] - inter / (16 - inter)) < 1e-6
    # identical boxes
    for r in (0.0, 0.3, -2.1, 3.0):
        q = box(5.5, -3.2, 4.1, 1.7, r)
        assert abs(R.bev_iou_f32(q, q)[0] - 1) < 1e-5
    # a square rotated by 90 degrees is itself
    assert abs(R.bev_iou_f32(box(2, 3, 3, 3, 0), box(2, 3, 3, 3, np.pi / 2))[0] - 1) < 1e-5
    # containment: area ratio
    assert abs(R.bev_iou_f32(box(0, 0, 10, 8, 0.4), box(0.5, -0.3, 2, 1, 1.1))[0] - 2 / 80) < 1e-6
    # disjoint
    assert R.bev_iou_f32(box(0, 0, 2, 2, 0.2), box(10, 0, 2, 2, 0.7))[0] == 0
    # shared edge / touching corner: finite, (near) zero
    for q in (box(2, 0, 2, 2), box(2, 2, 2, 2)):
        v = R.bev_iou_f32(box(0, 0, 2, 2), q)[0]
        assert np.isfinite(v) and v < 1e-5
    # zero-area box
    assert R.bev_iou_f32(box(0, 0, 0, 2), box(0, 0, 2, 2))[0] < 1e-6
    # rotation sign: the kernel rotates corners by x' = dx cos + dy sin, y' = -dx sin + dy cos (clockwise for r > 0).
    # A 4 x 1 box at the origin turned by +45 degrees runs along y = -x, so a small box at (1, -1) lies on it and one
    # at (1, 1) does not.
    long_box = box(0, 0, 4, 1, np.pi / 4)
    on = R.bev_overlap_f32(long_box, box(1, -1, 0.4, 0.4))[0]
    off = R.bev_overlap_f32(long_box, box(1, 1, 0.4, 0.4))[0]
    assert abs(on - 0.16) < 1e-5 and off == 0


def _lidar_bev_xyxyr(b7):
    b = np.asarray(b7, F32)[:, [0, 1, 3, 4, 6]]
    half_w, half_h = b[:, 2] / F32(2), b[:, 3] / F32(2)
    return np.column_stack([b[:, 0] - half_w, b[:, 1] - half_h, b[:, 0] + half_w, b[:, 1] + half_h, b[:, 4]]).astype(F32)


def overlaps_3d_host(b1, b2, mode):
    """BaseInstance3DBoxes.overlaps (base_box3d.py:395-450) for LiDAR boxes on the host restatement"""
    bev = R.pairwise(R.bev_overlap_f32, _lidar_bev_xyxyr(b1), _lidar_bev_xyxyr(b2))
    top = np.minimum((b1[:, 2] + b1[:, 5])[:, None], (b2[:, 2] + b2[:, 5])[None])
    bottom = np.maximum(b1[:, 2][:, None], b2[:, 2][None])
    o3 = bev * np.maximum(top - bottom, 0)
    v1, v2 = b1[:, 3:6].prod(1)[:, None], b2[:, 3:6].prod(1)[None]
    return o3 / np.maximum(v1 + v2 - o3, 1e-8) if mode == 'iou' else o3 / np.maximum(v1, 1e-8)


def test_restatement_reproduces_the_reference_iou_fixture():
    g = load_golden('box_ops_kat.npz')
    for mode, key in (('iou', 'iou_expected'), ('iof', 'iof_expected')):
        got = overlaps_3d_host(g['iou_boxes1'], g['iou_boxes2'], mode)
        np.testing.assert_allclose(got, g[key], rtol=1e-4, atol=1e-7)


def test_host_nms_reproduces_the_reference_multi_class_nms():
    g = load_golden('box_ops_kat.npz')
    probs, preds = g['mcn_probs'], g['mcn_preds']
    bev = _lidar_bev_xyxyr(preds)
    selected = []
    for k in range(probs.shape[1]):  # parta2_bbox_head.py:601-620: score >= 0.1, rotated NMS at 0.001
        idx = np.nonzero(probs[:, k] >= F32(0.1))[0]
        if len(idx) == 0:
            continue
        order = np.argsort(-probs[idx, k], kind='stable')
        keep = R.nms_host(bev[idx][order], 0.001, rotated=True)
        selected.append(idx[order[keep]])
    assert np.concatenate(selected).tolist() == g['mcn_expected'].tolist()


def test_host_nms_pairs_filter_is_exact():
    """nms_host only evaluates pairs whose circles meet: the same keep list as evaluating every pair"""
    rng = np.random.default_rng(5)
    c = rng.uniform(-10, 10, (300, 2))
    s = rng.uniform(0.5, 4, (300, 2))
    b = np.column_stack([c - s / 2, c + s / 2, rng.uniform(-3, 3, 300)]).astype(F32)
    for rotated in (True, False):
        full = R.nms_host(b, 0.1, rotated, pairs=np.triu_indices(300, 1))
        assert full.tolist() == R.nms_host(b, 0.1, rotated).tolist()


def _reference_attrs(rel, module):
    path = os.path.join(os.environ.get('SST_REFERENCE_ROOT', '/root/reference'), rel)
    if not os.path.exists(path):
        pytest.skip('reference tree not present')
    return set(re.findall(rf'\b{module}\.([A-Za-z_][A-Za-z0-9_]*)', open(path).read()))


def test_shims_provide_every_attribute_the_reference_uses():
    from sst_amd import native_shims as S
    used = {}
    for rel in ('mmdet3d/ops/iou3d/iou3d_utils.py', 'mmdet3d/core/bbox/structures/base_box3d.py',
                'mmdet3d/core/bbox/structures/lidar_box3d.py'):
        used.setdefault('iou3d_cuda', set()).update(_reference_attrs(rel, 'iou3d_cuda'))
    used['roiaware_pool3d_ext'] = _reference_attrs('mmdet3d/ops/roiaware_pool3d/points_in_boxes.py',
                                                   'roiaware_pool3d_ext')
    assert {'nms_gpu', 'nms_normal_gpu', 'boxes_iou_bev_gpu', 'boxes_overlap_bev_gpu'} <= used['iou3d_cuda']
    for mod, names in used.items():
        ns = getattr(S, mod)
        missing = [n for n in names if not callable(getattr(ns, n, None))]
        assert not missing, f'{mod}: {missing}'
    # TorchEx: lidar_box3d.py imports boxes_overlap_1to1 from it
    src = open(os.path.join(os.environ.get('SST_REFERENCE_ROOT', '/root/reference'),
                            'mmdet3d/core/bbox/structures/lidar_box3d.py')).read()
    assert 'boxes_overlap_1to1' in src and callable(S.torchex.boxes_overlap_1to1)


def test_torchex_shim_keeps_connected_components_absent(monkeypatch):
    from sst_amd import native_shims as S
    monkeypatch.setitem(sys.modules, 'torchex', S.torchex)
    with pytest.raises(ImportError):
        from torchex import connected_components  # noqa: F401
    from torchex import boxes_overlap_1to1  # noqa: F401


def test_shims_and_ops_refuse_cpu_tensors():
    import torch
    import sst_amd
    from sst_amd import native_shims as S
    a = torch.zeros(3, 5)
    with pytest.raises(RuntimeError):
        S.iou3d_cuda.boxes_iou_bev_gpu(a, a, torch.zeros(3, 3))
    with pytest.raises(RuntimeError):
        S.iou3d_cuda.nms_gpu(a, torch.zeros(3, dtype=torch.long), 0.5, 0)
    with pytest.raises(RuntimeError):
        sst_amd.boxes_iou_bev(a, a)
    with pytest.raises(RuntimeError):
        sst_amd.points_in_boxes_gpu(torch.zeros(1, 4, 3), torch.zeros(1, 2, 7))
    with pytest.raises(RuntimeError):
        S.roiaware_pool3d_ext.points_in_boxes_cpu(torch.zeros(2, 7), torch.zeros(4, 3), torch.zeros(2, 4))
    with pytest.raises(RuntimeError):
        S.roiaware_pool3d_ext.forward()


def test_library_exports_the_box_ops():
    from sst_amd import _lib
    lib = _lib.load()
    assert lib.sst_nms_bev_workspace_bytes(0) >= 256
    assert lib.sst_nms_bev_workspace_bytes(20000) >= 20000 * 313 * 8
    # empty problems and argument errors need no device
    assert lib.sst_boxes_overlap_bev_f32(None, 0, None, 5, 1, None, None) == 0
    assert lib.sst_boxes_overlap_bev_f32(None, 1, None, 1, 7, None, None) == _lib.SST_ERR_ARG
    assert lib.sst_points_in_boxes_f32(None, None, 1, 3, 0, 0, None, None) == 0
    assert lib.sst_points_in_boxes_f32(None, None, 1, 3, 5, 2, None, None) == _lib.SST_ERR_ARG
    assert lib.sst_nms_bev_f32(None, None, 10, 0.5, None, 0, 1, None, None, None, None) == _lib.SST_ERR_ARG
    assert ROOT


def test_reference_box_modules_import_with_the_shims(monkeypatch):
    """route B's three sys.modules lines let the reference's iou3d_utils.py, points_in_boxes.py and
    lidar_box3d.py (with base_box3d.py / utils.py under it) import unmodified, with no reference CUDA extension and no
    TorchEx; their native calls land in the shims (which refuse CPU tensors, as CHECK_INPUT does).  The packages above
    them are bare namespaces here: the other native extensions mmdet3d/ops/__init__.py imports are not route B's."""
    import importlib.util
    import types
    import torch
    from sst_amd import native_shims as S
    ref = os.environ.get('SST_REFERENCE_ROOT', '/root/reference')
    if not os.path.exists(os.path.join(ref, 'mmdet3d/ops/iou3d/iou3d_utils.py')):
        pytest.skip('reference tree not present')

    def pkg(name, rel=None):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref, rel)] if rel else []
        monkeypatch.setitem(sys.modules, name, m)
        return m

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
        mod = importlib.util.module_from_spec(spec)
        monkeypatch.setitem(sys.modules, name, mod)
        spec.loader.exec_module(mod)
        return mod

    for name in ('mmdet3d', 'mmdet3d.ops', 'mmdet3d.core', 'mmdet3d.core.bbox'):
        pkg(name)
    pkg('mmdet3d.ops.iou3d', 'mmdet3d/ops/iou3d')
    pib_pkg = pkg('mmdet3d.ops.roiaware_pool3d', 'mmdet3d/ops/roiaware_pool3d')
    pkg('mmdet3d.core.bbox.structures', 'mmdet3d/core/bbox/structures')
    pkg('mmdet3d.core.points').BasePoints = type('BasePoints', (), {})
    monkeypatch.delitem(sys.modules, 'torchex', raising=False)
    # the binding of INTEGRATION.md section B
    monkeypatch.setitem(sys.modules, 'mmdet3d.ops.iou3d.iou3d_cuda', S.iou3d_cuda)
    monkeypatch.setitem(sys.modules, 'mmdet3d.ops.roiaware_pool3d.roiaware_pool3d_ext', S.roiaware_pool3d_ext)
    monkeypatch.setitem(sys.modules, 'torchex', S.torchex)

    iou = load('mmdet3d.ops.iou3d.iou3d_utils', 'mmdet3d/ops/iou3d/iou3d_utils.py')
    pib = load('mmdet3d.ops.roiaware_pool3d.points_in_boxes', 'mmdet3d/ops/roiaware_pool3d/points_in_boxes.py')
    pib_pkg.points_in_boxes_gpu = pib.points_in_boxes_gpu  # what roiaware_pool3d/__init__.py re-exports
    load('mmdet3d.core.bbox.structures.utils', 'mmdet3d/core/bbox/structures/utils.py')
    base = load('mmdet3d.core.bbox.structures.base_box3d', 'mmdet3d/core/bbox/structures/base_box3d.py')
    lidar = load('mmdet3d.core.bbox.structures.lidar_box3d', 'mmdet3d/core/bbox/structures/lidar_box3d.py')
    assert iou.iou3d_cuda is S.iou3d_cuda and base.iou3d_cuda is S.iou3d_cuda and lidar.iou3d_cuda is S.iou3d_cuda
    assert pib.roiaware_pool3d_ext is S.roiaware_pool3d_ext
    assert lidar.boxes_overlap_1to1 is S.torchex.boxes_overlap_1to1  # not None: the TorchEx import succeeded
    with pytest.raises(RuntimeError):
        iou.boxes_iou_bev(torch.zeros(2, 5), torch.zeros(3, 5))
    with pytest.raises(RuntimeError):
        iou.nms_gpu(torch.zeros(2, 5), torch.rand(2), 0.5)
