"""Rotated-box ops on the MI355X (csrc/box_ops.hip through sst_amd.box_ops and the shims) against the host restatement
(tests/box_ops_ref.py), an independent float64 clip, the reference's known-answer values (tests/golden/box_ops_kat.npz)
and the reference-pinned membership fixture (tests/golden/point_pool.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = 'cuda:0'


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


_cluster_boxes = R.cluster_boxes
_nms_inputs = R.nms_inputs


# ---------------------------------------------------------------------------------------------------------------------
# matrix and aligned kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_iou_matrix_matches_the_restatement():
    import sst_amd
    a = _cluster_boxes(300, 0, 12.0)
    b = _cluster_boxes(200, 1, 12.0)
    for fn, ref in ((sst_amd.boxes_iou_bev, R.bev_iou_f32), (sst_amd.boxes_overlap_bev, R.bev_overlap_f32),
                    (sst_amd.box_ops.boxes_iou_bev_axis, R.axis_iou_f32)):
        got = fn(_t(a), _t(b)).cpu().numpy()
        want = R.pairwise(ref, a, b)
        assert got.shape == (300, 200)
        tol = 1e-5 if ref is not R.bev_overlap_f32 else 1e-4  # areas up to 36 m^2
        assert np.abs(got - want).max() <= tol
        assert (want > 0).sum() > 500
    # run to run
    x = sst_amd.boxes_iou_bev(_t(a), _t(b))
    assert torch.equal(x, sst_amd.boxes_iou_bev(_t(a), _t(b)))


def test_iou_within_float32_noise_of_float64_and_aligned_is_the_diagonal():
    import sst_amd
    a, b = R.random_pairs(2500, 0)
    got = sst_amd.box_ops.boxes_iou_bev(_t(a[:300]), _t(b[:300])).diagonal().cpu().numpy()
    want = np.array([R.bev_iou_f64(x, y) for x, y in zip(a[:300].astype(np.float64), b[:300].astype(np.float64))])
    assert np.abs(got - want).max() <= R.F32_IOU_NOISE
    # aligned over all pairs: within 1e-5 of the restatement, within the noise of float64
    area = sst_amd.boxes_overlap_1to1(_t(a), _t(b)).cpu().numpy()
    assert np.abs(area - R.bev_overlap_f32(a, b)).max() <= 1e-4
    # bit-identical to the matrix diagonal
    diag = sst_amd.boxes_overlap_bev(_t(a[:400]), _t(b[:400])).diagonal().cpu().numpy()
    assert np.array_equal(area[:400].view(np.int32), diag.view(np.int32))


def test_reference_3d_iou_fixture():
    import sst_amd
    g = load_golden('box_ops_kat.npz')
    b1, b2 = _t(g['iou_boxes1']), _t(g['iou_boxes2'])
    iou = sst_amd.boxes3d_overlaps_lidar(b1, b2).cpu()
    iof = sst_amd.boxes3d_overlaps_lidar(b1, b2, mode='iof').cpu()
    assert torch.allclose(torch.from_numpy(g['iou_expected']), iou, rtol=1e-4, atol=1e-7)
    assert torch.allclose(torch.from_numpy(g['iof_expected']), iof, rtol=1e-4, atol=1e-7)


def test_empty_and_zero_area():
    import sst_amd
    e = torch.zeros(0, 5, device=DEV)
    b = _t(_cluster_boxes(5, 2))
    assert sst_amd.boxes_iou_bev(e, b).shape == (0, 5)
    assert sst_amd.boxes_iou_bev(b, e).shape == (5, 0)
    assert sst_amd.boxes_overlap_1to1(e, e).shape == (0,)
    assert sst_amd.boxes3d_overlaps_lidar(torch.zeros(0, 7, device=DEV), torch.zeros(3, 7, device=DEV)).shape == (0, 3)
    flat = _t([[0, 0, 0, 2, 0.3], [1, 1, 1, 1, 0.0]])
    sq = _t([[-1, -1, 1, 1, 0.1], [0, 0, 2, 2, 0.0]])
    v = sst_amd.boxes_iou_bev(flat, sq).cpu()
    assert torch.isfinite(v).all() and v.abs().max() < 1e-6
    touch = sst_amd.boxes_iou_bev(_t([[0, 0, 2, 2, 0]]), _t([[2, 0, 4, 2, 0], [2, 2, 4, 4, 0]])).cpu()
    assert torch.isfinite(touch).all() and touch.max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rotated', [True, False])
def test_nms_keep_lists_equal_the_host_sweep(rotated):
    from sst_amd import box_ops
    thresh = 0.25
    for n in (0, 1, 63, 64, 65, 500, 4096, 20000):
        b = _nms_inputs(n, thresh, rotated, n + 7)
        assert len(b) == n
        keep, k = box_ops.nms_sorted(_t(b.reshape(-1, 5)), thresh, rotated=rotated)
        want = R.nms_host(b, thresh, rotated)
        assert k == len(want) and keep.cpu().numpy().tolist() == want.tolist(), n
        if n >= 500:
            assert 0 < k < n  # suppression really happened
            again, _ = box_ops.nms_sorted(_t(b), thresh, rotated=rotated)
            assert torch.equal(again, keep)


def test_grouped_nms_equals_per_group_runs():
    from sst_amd import box_ops
    b = _nms_inputs(3000, [0.3, 0.6], True, 11)
    rng = np.random.default_rng(3)
    groups = rng.integers(0, 3, len(b))
    thr = [0.3, None, 0.6]
    keep, _ = box_ops.nms_sorted(_t(b), 0.0, rotated=True, groups=_t(groups, torch.int32), group_thresh=thr)
    want = []
    for g, t in enumerate(thr):
        idx = np.nonzero(groups == g)[0]
        if t is None:
            want.extend(idx.tolist())
            continue
        sub, _ = box_ops.nms_sorted(_t(b[idx]), t, rotated=True)
        want.extend(idx[sub.cpu().numpy()].tolist())
    assert keep.cpu().numpy().tolist() == sorted(want)
    assert keep.cpu().numpy().tolist() == R.nms_host(b, 0.0, True, groups=groups, group_thresh=thr).tolist()


def test_reference_multi_class_nms_fixture():
    import sst_amd
    g = load_golden('box_ops_kat.npz')
    probs, preds = _t(g['mcn_probs']), _t(g['mcn_preds'])
    bev = sst_amd.box_ops.xywhr2xyxyr(sst_amd.box_ops.lidar_bev(preds))
    selected = []
    for k in range(probs.shape[1]):  # parta2_bbox_head.py:601-620
        keep = probs[:, k] >= 0.1
        if keep.int().sum() > 0:
            idx = keep.nonzero(as_tuple=False).view(-1)
            sel = sst_amd.nms_gpu(bev[keep], probs[keep, k], 0.001)
            selected.append(idx[sel])
    assert torch.cat(selected).cpu().tolist() == g['mcn_expected'].tolist()
    # the same through the shim, with the reference's iou3d_utils.nms_gpu data flow (CPU keep filled in place)
    from sst_amd import native_shims as S
    order = probs[:, 2].sort(0, descending=True)[1]
    boxes = bev[order].contiguous()
    keep = torch.zeros(boxes.size(0), dtype=torch.long)
    num = S.iou3d_cuda.nms_gpu(boxes, keep, 0.001, 0)
    assert isinstance(num, int)
    assert order[keep[:num].to(DEV)].cpu().tolist() == g['mcn_expected'].tolist()


def test_nms_gpu_caps_and_nms_normal():
    import sst_amd
    b = _nms_inputs(600, 0.2, True, 5)
    scores = torch.rand(600, generator=torch.Generator().manual_seed(0))
    order = scores.sort(0, descending=True)[1].numpy()
    got = sst_amd.nms_gpu(_t(b), scores.to(DEV), 0.2, pre_maxsize=400, post_max_size=50).cpu().numpy()
    want = order[:400][R.nms_host(b[order[:400]], 0.2, True)][:50]
    assert got.tolist() == want.tolist() and got.dtype == np.int64
    b2 = _nms_inputs(600, 0.2, False, 6)
    got = sst_amd.nms_normal_gpu(_t(b2), scores.to(DEV), 0.2).cpu().numpy()
    assert got.tolist() == order[R.nms_host(b2[order], 0.2, False)].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# box3d_multiclass_nms
# ---------------------------------------------------------------------------------------------------------------------
def _mc_inputs(n=400, seed=0):
    rng = np.random.default_rng(seed)
    bev = _cluster_boxes(n, seed, 15.0)
    b = np.concatenate([bev, rng.normal(size=(n, 4)).astype(F32)], 1)
    scores = rng.permutation(n * 4).reshape(n, 4).astype(F32) / F32(n * 4)  # distinct
    return b, bev, scores, rng


@pytest.mark.parametrize('case', ['scalar', 'lists', 'none_class', 'all_none', 'max_num', 'empty', 'all_outputs'])
def test_box3d_multiclass_nms_matches_the_reference_flow(case):
    import sst_amd
    b, bev, scores, rng = _mc_inputs()
    score_thr, nms_thr, max_num, rotated = 0.3, 0.2, 1000, True
    extra = {}
    if case == 'lists':
        score_thr, nms_thr = [0.2, 0.4, 0.3], [0.1, 0.45, 0.3]
    elif case == 'none_class':
        nms_thr = [0.2, None, 0.3]
    elif case == 'all_none':
        nms_thr = None  # FSD's proposal config: no NMS launch, candidates in index order class by class
    elif case == 'max_num':
        max_num = 40
    elif case == 'empty':
        score_thr = 2.0
    elif case == 'all_outputs':
        rotated = False
        extra = dict(mlvl_dir_scores=rng.normal(size=len(b)).astype(F32),
                     mlvl_attr_scores=rng.normal(size=len(b)).astype(F32),
                     mlvl_bboxes2d=rng.normal(size=(len(b), 4)).astype(F32))
    cfg = dict(nms_thr=nms_thr, use_rotate_nms=rotated)
    got = sst_amd.box3d_multiclass_nms(_t(b), _t(bev), _t(scores), score_thr, max_num, cfg,
                                       **{k: _t(v) for k, v in extra.items()})
    want = R.multiclass_nms_host(b, bev, scores, score_thr, max_num, nms_thr, rotated,
                                 extra.get('mlvl_dir_scores'), extra.get('mlvl_attr_scores'), extra.get('mlvl_bboxes2d'))
    assert len(got) == 3 + len(extra)
    if want is None:
        assert got[0].shape == (0, b.shape[1]) and got[1].shape == (0,) and got[2].shape == (0,)
        assert got[2].dtype == torch.long
        return
    assert got[2].dtype == torch.long
    assert np.array_equal(got[2].cpu().numpy(), want['labels'])
    assert np.array_equal(got[1].cpu().numpy(), want['scores'])
    assert np.array_equal(got[0].cpu().numpy(), want['bboxes'])
    for i, k in enumerate(('dir', 'attr', 'b2d')[:len(extra)]):
        assert np.array_equal(got[3 + i].cpu().numpy(), want[k])
    if case == 'max_num':
        assert len(want['scores']) == 40
    if case == 'none_class':
        lab = want['labels']
        assert (lab == 1).sum() == (scores[:, 1] > F32(0.3)).sum()


# ---------------------------------------------------------------------------------------------------------------------
# points in boxes
# ---------------------------------------------------------------------------------------------------------------------
def _host_membership(boxes, pts):
    from oracle import point_pool_oracle as O
    r = np.asarray(boxes, F32)
    lx, ly, lz = O.local_coords(r, pts)
    inside = O.inside(lx, ly, lz, r[:, 3], r[:, 4], r[:, 5])
    clear = O.face_clearance(r, pts, np.zeros(3, F32))
    return inside, clear  # [T, N]


@pytest.mark.parametrize('tag', ['veh', 'ped'])
def test_points_in_boxes_on_the_reference_membership_fixture(tag):
    import sst_amd
    g = load_golden('point_pool.npz')
    rois, pts = g[f'in::{tag}::rois'], g[f'in::{tag}::pts']
    member = sst_amd.points_in_boxes_batch(_t(pts[None]), _t(rois[None])).cpu().numpy()[0]  # [N, T]
    first = sst_amd.points_in_boxes_gpu(_t(pts[None]), _t(rois[None])).cpu().numpy()[0]
    ref = np.zeros((len(pts), len(rois)), bool)
    pr = g[f'out::{tag}::pairs_in_box']
    ref[pr[:, 1], pr[:, 0]] = True
    _, clear = _host_membership(rois, pts)
    diff = (member == 1) != ref
    assert member.sum() > 500 and np.all(clear.T[diff] < 1e-5)
    # first box = the smallest index of the membership row, exactly
    any_in = member.any(1)
    assert np.array_equal(first, np.where(any_in, member.argmax(1), -1))


def test_points_in_boxes_batch_of_two_with_different_boxes():
    import sst_amd
    g = load_golden('point_pool.npz')
    boxes = np.stack([g['in::veh::rois'][:100], g['in::ped::rois'][:100]])
    pts = np.stack([g['in::veh::pts'][:6000], g['in::ped::pts'][:6000]])
    member = sst_amd.points_in_boxes_batch(_t(pts), _t(boxes)).cpu().numpy()
    first = sst_amd.points_in_boxes_gpu(_t(pts), _t(boxes)).cpu().numpy()
    assert member.shape == (2, 6000, 100) and first.shape == (2, 6000)
    for s in range(2):
        inside, clear = _host_membership(boxes[s], pts[s])
        diff = (member[s] == 1) != inside.T
        assert member[s].sum() > 100 and np.all(clear.T[diff] < 1e-5)
        assert np.array_equal(first[s], np.where(member[s].any(1), member[s].argmax(1), -1))


def test_points_in_boxes_overlapping_boxes_and_empty_shapes():
    import sst_amd
    boxes = _t([[[0, 0, 0, 4, 4, 2, 0.0], [0, 0, 0, 2, 2, 2, 0.3], [0, 0, 0, 8, 8, 4, 1.0]]])
    pts = _t([[[0.1, 0.2, 1.0], [1.9, 1.9, 1.0], [3.5, 0.0, 3.0], [50, 50, 1]]])
    first = sst_amd.points_in_boxes_gpu(pts, boxes).cpu().tolist()
    assert first == [[0, 0, 2, -1]]
    member = sst_amd.points_in_boxes_batch(pts, boxes).cpu().tolist()
    assert member == [[[1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0]]]
    # reversed order: the smallest index wins
    assert sst_amd.points_in_boxes_gpu(pts, boxes.flip(1).contiguous()).cpu().tolist() == [[0, 0, 0, -1]]
    # T = 0, N = 0
    none = torch.zeros(1, 0, 7, device=DEV)
    assert sst_amd.points_in_boxes_gpu(pts, none).cpu().tolist() == [[-1, -1, -1, -1]]
    assert sst_amd.points_in_boxes_batch(pts, none).shape == (1, 4, 0)
    nopts = torch.zeros(1, 0, 3, device=DEV)
    assert sst_amd.points_in_boxes_gpu(nopts, boxes).shape == (1, 0)
    assert sst_amd.points_in_boxes_batch(nopts, boxes).shape == (1, 0, 3)
    # more boxes than one LDS tile (first-box mode tiles T by 256): the answer is the smallest index
    many = boxes[:, :1].repeat(1, 600, 1).contiguous()
    many[0, :299, 0] += 100.0
    assert sst_amd.points_in_boxes_gpu(pts, many).cpu().tolist()[0][:2] == [299, 299]


def test_points_in_boxes_reference_fixture():
    import sst_amd
    g = load_golden('box_ops_kat.npz')
    got = sst_amd.points_in_boxes_gpu(_t(g['pib_gpu_pts']), _t(g['pib_gpu_boxes'])).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, g['pib_gpu_expected'])
    got = sst_amd.points_in_boxes_batch(_t(g['pib_batch_pts']), _t(g['pib_batch_boxes'])).cpu().numpy()
    assert np.array_equal(got, g['pib_batch_expected'])


# ---------------------------------------------------------------------------------------------------------------------
# shims: the reference's argument orders and in / out conventions
# ---------------------------------------------------------------------------------------------------------------------
def test_shims_with_reference_conventions():
    import sst_amd
    from sst_amd import native_shims as S
    g = load_golden('box_ops_kat.npz')
    # roiaware_pool3d_ext: boxes first, output pre-filled by the caller
    pts, boxes = _t(g['pib_gpu_pts']), _t(g['pib_gpu_boxes'])
    out = torch.full(tuple(pts.shape[:2]), -1, dtype=torch.int32, device=DEV)
    S.roiaware_pool3d_ext.points_in_boxes_gpu(boxes, pts, out)
    assert np.array_equal(out.cpu().numpy(), g['pib_gpu_expected'])
    pts, boxes = _t(g['pib_batch_pts']), _t(g['pib_batch_boxes'])
    out = torch.zeros(pts.shape[0], pts.shape[1], boxes.shape[1], dtype=torch.int32, device=DEV)
    S.roiaware_pool3d_ext.points_in_boxes_batch(boxes, pts, out)
    assert np.array_equal(out.cpu().numpy(), g['pib_batch_expected'])
    # iou3d_cuda: caller's device output filled in place
    a, b = _t(_cluster_boxes(40, 8, 5.0)), _t(_cluster_boxes(30, 9, 5.0))
    ans = a.new_zeros((40, 30))
    S.iou3d_cuda.boxes_iou_bev_gpu(a, b, ans)
    assert torch.equal(ans, sst_amd.boxes_iou_bev(a, b))
    S.iou3d_cuda.boxes_overlap_bev_gpu(a, b, ans)
    assert torch.equal(ans, sst_amd.boxes_overlap_bev(a, b))
    # nms: CPU keep filled, count returned
    keep = torch.full((40,), -7, dtype=torch.long)
    num = S.iou3d_cuda.nms_normal_gpu(a, keep, 0.1, 0)
    want = R.nms_host(a.cpu().numpy(), 0.1, False)
    assert num == len(want) and keep[:num].tolist() == want.tolist() and (keep[num:] == -7).all()
    # torchex.boxes_overlap_1to1
    assert torch.equal(S.torchex.boxes_overlap_1to1(a[:30], b), sst_amd.boxes_overlap_bev(a[:30], b).diagonal())
    # CPU or non-contiguous input raises, as CHECK_INPUT does
    with pytest.raises(RuntimeError):
        S.iou3d_cuda.boxes_iou_bev_gpu(a.cpu(), b, ans)
    with pytest.raises(RuntimeError):
        S.iou3d_cuda.boxes_iou_bev_gpu(a.t().contiguous().t(), b, ans)
    with pytest.raises(RuntimeError):
        S.iou3d_cuda.nms_gpu(a[:, :5:1].t().contiguous().t(), keep, 0.1, 0)
    with pytest.raises(RuntimeError):
        S.roiaware_pool3d_ext.points_in_boxes_gpu(boxes.cpu(), pts, out)


def test_mismatched_shapes_raise_before_any_launch():
    import sst_amd
    from sst_amd import box_ops
    from sst_amd import native_shims as S
    pts, boxes = torch.zeros(2, 10, 3, device=DEV), torch.zeros(2, 4, 7, device=DEV)
    for p, b in ((pts, boxes[:1]), (pts[..., :2].contiguous(), boxes), (pts, boxes[..., :6].contiguous()),
                 (pts[0], boxes)):
        with pytest.raises(RuntimeError):
            S.roiaware_pool3d_ext.points_in_boxes_gpu(b, p, torch.zeros(2, 10, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        S.roiaware_pool3d_ext.points_in_boxes_batch(boxes, pts, torch.zeros(2, 10, 5, dtype=torch.int32, device=DEV))
    b5 = _t(_cluster_boxes(8, 3, 4.0))
    with pytest.raises(RuntimeError):
        box_ops.nms_sorted(b5[:, :4].contiguous(), 0.5)
    with pytest.raises(RuntimeError):
        box_ops.nms_sorted(b5, 0.0, groups=torch.zeros(7, dtype=torch.int32, device=DEV), group_thresh=[0.5])
    with pytest.raises(RuntimeError):
        box_ops.nms_sorted(b5, 0.0, groups=torch.zeros(8, dtype=torch.int32, device=DEV), group_thresh=[0.5] * 65)
    with pytest.raises(RuntimeError):
        sst_amd.boxes_iou_bev(b5[:, :4].contiguous(), b5)
    with pytest.raises(RuntimeError):
        sst_amd.boxes_overlap_1to1(b5, b5[:7])
    with pytest.raises(RuntimeError):
        S.iou3d_cuda.boxes_iou_bev_gpu(b5, b5, b5.new_zeros(8, 7))
