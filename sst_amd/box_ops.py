"""Rotated-box ops of the heads and the FSD training step: BEV overlap / IoU, rotated and axis-aligned NMS, points in
boxes, the 3D overlaps of LiDAR boxes and the multi-class NMS of the heads.

Names, signatures and return conventions are the reference's (mmdet3d/ops/iou3d/iou3d_utils.py,
ops/roiaware_pool3d/points_in_boxes.py, core/post_processing/box3d_nms.py, BaseInstance3DBoxes.overlaps); the Python
around each native call is kept, so sorting, caps and dtypes behave as there.  The work runs in csrc/box_ops.hip
behind the C ABI of include/sst_amd.h.  fp32 inputs only, as in the reference; CPU or non-contiguous tensors raise.
"""
import torch

from . import _lib

BOX_OVERLAP, BOX_IOU, BOX_IOU_AXIS = 0, 1, 2
PIB_FIRST, PIB_MEMBERSHIP = 0, 1


def _check_f32(*tensors):
    _lib.require_cuda(*tensors)
    for t in tensors:
        if t.dtype != torch.float32:
            raise RuntimeError(f'sst_amd.box_ops: float32 tensors expected, got {t.dtype}')


def _check_boxes(t, width, what):
    """[N, width] device fp32, contiguous; the kernels read exactly this many floats per box"""
    _check_f32(t)
    if t.dim() != 2 or t.size(1) != width:
        raise RuntimeError(f'{what}: boxes of shape [N, {width}] expected, got {tuple(t.shape)}')


def _pairwise(a, b, mode):
    _check_boxes(a, 5, 'boxes_overlap_bev')
    _check_boxes(b, 5, 'boxes_overlap_bev')
    out = a.new_zeros((a.size(0), b.size(0)))
    if out.numel():
        _lib.check(_lib.load().sst_boxes_overlap_bev_f32(_lib.ptr(a), a.size(0), _lib.ptr(b), b.size(0), mode,
                                                         _lib.ptr(out), _lib.stream_ptr()), 'boxes_overlap_bev')
    return out


def boxes_overlap_bev(boxes_a, boxes_b):
    """[M, 5] x [N, 5] ([x1, y1, x2, y2, ry]) -> [M, N] rotated overlap areas (iou3d_cuda.boxes_overlap_bev_gpu)"""
    return _pairwise(boxes_a.contiguous(), boxes_b.contiguous(), BOX_OVERLAP)


def boxes_iou_bev(boxes_a, boxes_b):
    """[M, 5] x [N, 5] -> [M, N] rotated BEV IoU (iou3d_utils.py:12-28)"""
    return _pairwise(boxes_a.contiguous(), boxes_b.contiguous(), BOX_IOU)


def boxes_iou_bev_axis(boxes_a, boxes_b):
    """[M, 5] x [N, 5] -> [M, N] axis-aligned IoU, ry ignored (the pairwise form of the reference's iou_normal)"""
    return _pairwise(boxes_a.contiguous(), boxes_b.contiguous(), BOX_IOU_AXIS)


def boxes_overlap_1to1(boxes_a, boxes_b):
    """[N, 5] x [N, 5] -> [N] overlap area of pair i: TorchEx boxes_overlap_1to1 as lidar_box3d.py calls it
    (aligned_iou_3d / aligned_iou_bev); bit-identical to the diagonal of boxes_overlap_bev"""
    a, b = boxes_a.contiguous(), boxes_b.contiguous()
    _check_boxes(a, 5, 'boxes_overlap_1to1')
    _check_boxes(b, 5, 'boxes_overlap_1to1')
    if a.size(0) != b.size(0):
        raise RuntimeError('boxes_overlap_1to1: both inputs need the same number of boxes')
    out = a.new_zeros((a.size(0),))
    if out.numel():
        _lib.check(_lib.load().sst_boxes_overlap_aligned_f32(_lib.ptr(a), _lib.ptr(b), a.size(0), BOX_OVERLAP,
                                                             _lib.ptr(out), _lib.stream_ptr()), 'boxes_overlap_1to1')
    return out


def nms_sorted(boxes, thresh, rotated=True, groups=None, group_thresh=None):
    """NMS over boxes already sorted by descending score -> (keep [K] int64 positions on the device, K).

    groups: optional int32 / int64 [N] device group ids (boxes suppress only within their group); group_thresh: one
    threshold per group id (at most 64 groups), None = no suppression in that group.  The thresholds travel as kernel
    arguments; K is the one value read back to the host."""
    _check_boxes(boxes, 5, 'nms')
    n = boxes.size(0)
    dev = boxes.device
    keep = torch.empty(max(n, 1), dtype=torch.long, device=dev)
    num = torch.zeros(1, dtype=torch.int32, device=dev)
    gptr = thr = None
    n_groups = 0
    if groups is not None:
        _lib.require_cuda(groups)
        if groups.dim() != 1 or groups.numel() != n:
            raise RuntimeError(f'nms: {n} boxes need {n} group ids, got shape {tuple(groups.shape)}')
        groups = groups.to(dtype=torch.int32).contiguous()
        n_groups = len(group_thresh)
        if not 0 < n_groups <= 64:
            raise RuntimeError(f'nms: 1 to 64 group thresholds expected, got {n_groups}')
        thr = _lib.farray([float('inf') if t is None else float(t) for t in group_thresh])
        gptr = _lib.ptr(groups)
    ws = _lib.workspace(_lib.load().sst_nms_bev_workspace_bytes(n), dev)
    _lib.check(_lib.load().sst_nms_bev_f32(_lib.ptr(boxes), gptr, n, float(thresh if thresh is not None else 0.0), thr,
                                           n_groups, 1 if rotated else 0, _lib.ptr(keep), _lib.ptr(num), _lib.ptr(ws),
                                           _lib.stream_ptr()), 'nms_bev')
    k = int(num.item())
    return keep[:k], k


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """Rotated NMS (iou3d_utils.py:31-59): boxes [N, 5] ([x1, y1, x2, y2, ry]), scores [N] -> indices kept, as a device
    LongTensor in descending score order"""
    order = scores.sort(0, descending=True)[1]

    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    boxes = boxes[order].contiguous()

    keep, _ = nms_sorted(boxes, thresh, rotated=True)
    keep = order[keep].contiguous()
    if post_max_size is not None:
        keep = keep[:post_max_size]
    return keep


def nms_normal_gpu(boxes, scores, thresh):
    """Axis-aligned NMS (iou3d_utils.py:103-124): the angle of the boxes is ignored"""
    order = scores.sort(0, descending=True)[1]

    boxes = boxes[order].contiguous()

    keep, _ = nms_sorted(boxes, thresh, rotated=False)
    return order[keep].contiguous()


def _points_in_boxes(points, boxes, mode):
    assert boxes.shape[0] == points.shape[0], \
        f'Points and boxes should have the same batch size, got {boxes.shape[0]} and {points.shape[0]}'
    assert boxes.shape[2] == 7, f'boxes dimension should be 7, got unexpected shape {boxes.shape[2]}'
    assert points.shape[2] == 3, f'points dimension should be 3, got unexpected shape {points.shape[2]}'
    batch_size, num_points, _ = points.shape
    num_boxes = boxes.shape[1]
    if mode == PIB_FIRST:
        out = points.new_zeros((batch_size, num_points), dtype=torch.int).fill_(-1)
    else:
        out = points.new_zeros((batch_size, num_points, num_boxes), dtype=torch.int)
    _points_in_boxes_into(boxes.contiguous(), points.contiguous(), out, mode)
    return out


def _points_in_boxes_into(boxes, pts, out, mode):
    _check_f32(boxes, pts)
    _lib.require_cuda(out)
    if out.dtype != torch.int32:
        raise RuntimeError('points_in_boxes: the output must be int32')
    if boxes.dim() != 3 or boxes.size(2) != 7 or pts.dim() != 3 or pts.size(2) != 3 or boxes.size(0) != pts.size(0):
        raise RuntimeError(f'points_in_boxes: boxes [B, T, 7] and points [B, N, 3] expected, got {tuple(boxes.shape)} '
                           f'and {tuple(pts.shape)}')
    if not out.is_contiguous():
        raise RuntimeError('points_in_boxes: the output must be contiguous')
    b, n, t = pts.size(0), pts.size(1), boxes.size(1)
    if mode == PIB_FIRST and tuple(out.shape) != (b, n) or mode == PIB_MEMBERSHIP and tuple(out.shape) != (b, n, t):
        raise RuntimeError(f'points_in_boxes: output of shape {tuple(out.shape)} for {b} x {n} points and {t} boxes')
    _lib.check(_lib.load().sst_points_in_boxes_f32(_lib.ptr(boxes), _lib.ptr(pts), b, t, n, mode, _lib.ptr(out),
                                                   _lib.stream_ptr()), 'points_in_boxes')


def points_in_boxes_gpu(points, boxes):
    """points [B, M, 3], boxes [B, T, 7] ([x, y, z_bottom, w, l, h, ry], LiDAR) -> [B, M] int32, the smallest index of
    a box holding the point, -1 for background (points_in_boxes.py:6-47)"""
    return _points_in_boxes(points, boxes, PIB_FIRST)


def points_in_boxes_batch(points, boxes):
    """points [B, M, 3], boxes [B, T, 7] -> [B, M, T] int32 membership, background 0 (points_in_boxes.py:79-123)"""
    return _points_in_boxes(points, boxes, PIB_MEMBERSHIP)


def xywhr2xyxyr(boxes_xywhr):
    """core/bbox/structures/utils.py:85: [x, y, w, h, r] -> [x1, y1, x2, y2, r]"""
    boxes = torch.zeros_like(boxes_xywhr)
    half_w = boxes_xywhr[:, 2] / 2
    half_h = boxes_xywhr[:, 3] / 2
    boxes[:, 0] = boxes_xywhr[:, 0] - half_w
    boxes[:, 1] = boxes_xywhr[:, 1] - half_h
    boxes[:, 2] = boxes_xywhr[:, 0] + half_w
    boxes[:, 3] = boxes_xywhr[:, 1] + half_h
    boxes[:, 4] = boxes_xywhr[:, 4]
    return boxes


def lidar_bev(boxes):
    """LiDARInstance3DBoxes.bev (lidar_box3d.py:117-120): [N, 7] -> [N, 5] ([x, y, w, l, ry])"""
    return boxes[:, [0, 1, 3, 4, 6]]


def boxes3d_overlaps_lidar(boxes1, boxes2, mode='iou'):
    """BaseInstance3DBoxes.overlaps (base_box3d.py:395-450) for [N, 7] / [M, 7] LiDAR boxes (z = bottom): height
    overlap x rotated BEV overlap, divided by the union volume ('iou') or by the volume of boxes1 ('iof')"""
    assert mode in ['iou', 'iof']
    rows, cols = boxes1.size(0), boxes2.size(0)
    if rows * cols == 0:
        return boxes1.new_zeros((rows, cols))
    # height overlap (LiDARInstance3DBoxes: bottom = z, top = z + h)
    top1 = (boxes1[:, 2] + boxes1[:, 5]).view(-1, 1)
    top2 = (boxes2[:, 2] + boxes2[:, 5]).view(1, -1)
    bottom1 = boxes1[:, 2].view(-1, 1)
    bottom2 = boxes2[:, 2].view(1, -1)
    overlaps_h = torch.clamp(torch.min(top1, top2) - torch.max(bottom1, bottom2), min=0)
    overlaps_bev = boxes_overlap_bev(xywhr2xyxyr(lidar_bev(boxes1)).contiguous(),
                                     xywhr2xyxyr(lidar_bev(boxes2)).contiguous())
    overlaps_3d = overlaps_bev * overlaps_h
    # BaseInstance3DBoxes.volume (base_box3d.py:69-72): (w * l) * h, one rounding per product.  prod(dim=1) multiplies in an order
    # of the reduction kernel's choosing (one ulp apart on some boxes); the RoI head's assignment kernel (csrc/roi_head.hip) has
    # to produce these values bit for bit
    volume1 = (boxes1[:, 3] * boxes1[:, 4] * boxes1[:, 5]).view(-1, 1)
    volume2 = (boxes2[:, 3] * boxes2[:, 4] * boxes2[:, 5]).view(1, -1)
    if mode == 'iou':
        return overlaps_3d / torch.clamp(volume1 + volume2 - overlaps_3d, min=1e-8)
    return overlaps_3d / torch.clamp(volume1, min=1e-8)


def _cfg_get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def box3d_multiclass_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores, score_thr, max_num, cfg,
                         mlvl_dir_scores=None, mlvl_attr_scores=None, mlvl_bboxes2d=None):
    """Multi-class NMS of 3D boxes with the signature and outputs of core/post_processing/box3d_nms.py:10-143.

    Where the reference loops over the classes (per class an `.any()`, three boolean selections and an NMS count
    read-back: five host stalls), the candidate (box, class) pairs of all classes go through ONE grouped NMS launch
    sequence (group = class, per-class threshold; a class with nms_thr None keeps all its candidates in their original
    index order).  The kept pairs are then laid out class by class, each class in its own descending-score order, as the
    reference concatenates them; the `max_num` cut is the reference's score sort.  Host stalls per call: the candidate
    list's size (nonzero) and the kept count - only the first when every class has nms_thr None, as then no NMS is
    launched.  No host-to-device copy: thresholds are compared as scalars and passed to the kernels as arguments."""
    num_classes = mlvl_scores.shape[1] - 1
    dev = mlvl_scores.device
    score_thrs = list(score_thr) if isinstance(score_thr, (list, tuple)) else [score_thr] * num_classes
    assert len(score_thrs) == num_classes
    nms_thr = _cfg_get(cfg, 'nms_thr')
    nms_thrs = list(nms_thr) if isinstance(nms_thr, (list, tuple)) else [nms_thr] * num_classes
    assert len(nms_thrs) == num_classes
    rotated = bool(_cfg_get(cfg, 'use_rotate_nms'))

    # candidates [C, N]: the reference's `mlvl_scores[:, i] > cls_score_thr` per class (scalar compare in the scores'
    # dtype); (box, class) pairs in class-major order, class c's candidates in ascending box index
    cand = torch.stack([mlvl_scores[:, i] > score_thrs[i] for i in range(num_classes)], 0) if num_classes else \
        mlvl_scores.new_zeros((0, mlvl_scores.size(0)), dtype=torch.bool)
    cls_of, box_of = cand.nonzero(as_tuple=True)
    pair_scores = mlvl_scores[box_of, cls_of]
    if all(t is None for t in nms_thrs):
        # no NMS in any class (FSD's proposal config): every candidate, class by class, in index order
        labels, boxes_idx, scores = cls_of, box_of, pair_scores
    else:
        # one score sort of all pairs; a sort by class afterwards restores the per-class descending order
        order = pair_scores.sort(0, descending=True)[1]
        s_cls, s_box = cls_of[order], box_of[order]
        keep, _ = nms_sorted(mlvl_bboxes_for_nms[s_box].contiguous().float(), 0.0, rotated=rotated, groups=s_cls,
                             group_thresh=nms_thrs)
        k_cls, k_box, k_pos = s_cls[keep], s_box[keep], order[keep]
        k_rank = torch.arange(k_cls.numel(), device=dev)
        none_classes = [i for i, t in enumerate(nms_thrs) if t is None]
        if none_classes:
            # classes without NMS (box3d_nms.py:78-80): position in the class-major pair list = original index order
            no_nms = k_cls == none_classes[0]
            for i in none_classes[1:]:
                no_nms |= k_cls == i
            k_rank = torch.where(no_nms, k_pos, k_rank)
        # class by class; inside a class: score order (NMS classes) or index order (no-NMS classes)
        key = k_cls * (pair_scores.numel() + 1) + k_rank
        sel = key.sort(0)[1]
        labels, boxes_idx = k_cls[sel], k_box[sel]
        scores = pair_scores[k_pos[sel]]

    bboxes = mlvl_bboxes[boxes_idx]
    dir_scores = mlvl_dir_scores[boxes_idx] if mlvl_dir_scores is not None else None
    attr_scores = mlvl_attr_scores[boxes_idx] if mlvl_attr_scores is not None else None
    bboxes2d = mlvl_bboxes2d[boxes_idx] if mlvl_bboxes2d is not None else None

    if labels.numel() > 0:
        if bboxes.shape[0] > max_num:
            _, inds = scores.sort(descending=True)
            inds = inds[:max_num]
            bboxes = bboxes[inds, :]
            labels = labels[inds]
            scores = scores[inds]
            if mlvl_dir_scores is not None:
                dir_scores = dir_scores[inds]
            if mlvl_attr_scores is not None:
                attr_scores = attr_scores[inds]
            if mlvl_bboxes2d is not None:
                bboxes2d = bboxes2d[inds]
    else:
        bboxes = mlvl_scores.new_zeros((0, mlvl_bboxes.size(-1)))
        scores = mlvl_scores.new_zeros((0, ))
        labels = mlvl_scores.new_zeros((0, ), dtype=torch.long)
        if mlvl_dir_scores is not None:
            dir_scores = mlvl_scores.new_zeros((0, ))
        if mlvl_attr_scores is not None:
            attr_scores = mlvl_scores.new_zeros((0, ))
        if mlvl_bboxes2d is not None:
            bboxes2d = mlvl_scores.new_zeros((0, 4))

    results = (bboxes, scores, labels)
    if mlvl_dir_scores is not None:
        results = results + (dir_scores, )
    if mlvl_attr_scores is not None:
        results = results + (attr_scores, )
    if mlvl_bboxes2d is not None:
        results = results + (bboxes2d, )
    return results
