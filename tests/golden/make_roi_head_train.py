"""Generates tests/golden/roi_head_train.npz: the training and decoding side of GroupCorrectionHead / FullySparseBboxHead as the
REFERENCE computes it (data only).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_roi_head_train.py

Executed from their source text: GroupCorrectionHead._assign_and_sample (roi_heads/fsd_roi_head.py), IoUNegPiecewiseSampler
(core/bbox/samplers/iou_neg_piecewise_sampler.py), BboxOverlaps3D / bbox_overlaps_3d (iou_calculators/iou3d_calculator.py),
BaseInstance3DBoxes and LiDARInstance3DBoxes with overlaps and corners (structures/base_box3d.py, lidar_box3d.py),
rotation_3d_in_axis, limit_period, xywhr2xyxyr (structures/utils.py), DeltaXYZWLHRBBoxCoder
(coders/delta_xyzwhlr_bbox_coder.py) and FullySparseBboxHead.get_targets / _get_target_single / get_multi_class_soft_label /
get_class_wise_box_weights / loss / filter_pos_assigned_but_empty_rois / get_corner_loss_lidar / get_bboxes / multi_class_nms
(bbox_heads/fsd_bbox_head.py).  What the reference imports from packages that are not in its tree, or runs on CUDA only, is
stood in for here:
  mmdet MaxIoUAssigner          assign_wrt_overlaps as mmdet 2.x has it: background where 0 <= max < neg_iou_thr, positive (arg-max)
                                where max >= pos_iou_thr, then for every box in index order whose largest IoU is >= min_pos_iou
                                every proposal whose IoU equals it goes to that box (gt_max_assign_all); labels -1 off the
                                positives; without boxes everything is background with IoU 0
  mmdet RandomSampler           the constructor's fields; random_choice(gallery, k) = the k entries with the smallest recorded
                                key, ties by proposal index (the distribution of randperm(n)[:k]).  _sample_neg hands it
                                positions within the negatives; they are mapped to their proposals for the keys
  mmdet SamplingResult          the fields of mmdet 2.x; without boxes pos_gt_bboxes is an empty [0, box columns] tensor (mmdet
                                views it as [0, 4], which the reference's own assert in _get_target_single would refuse)
  mmdet AssignResult            a plain record
  mmdet CrossEntropyLoss        use_sigmoid: binary_cross_entropy_with_logits(pred, label, 'none') * weight, summed / avg_factor
  mmdet L1Loss                  (|pred - target| * weight).sum() / avg_factor * loss_weight
  mmdet SmoothL1Loss            the same with 0.5 d^2 / beta below beta, |d| - 0.5 beta above
  mmdet multi_apply, reduce_mean, bbox3d2roi      map / zip, the identity (one process), the sample index as column 0
  iou3d_cuda.boxes_overlap_bev_gpu                tests/box_ops_ref.py (float32: the reference's polygon algorithm operation by
                                                  operation; float64: an independent clip); Tensor.cuda() is the identity
  nms_gpu                       tests/box_ops_ref.nms_host over the boxes sorted by descending score
Every case runs in float32 and in float64; the float64 run executes the same source text with ``torch.float32`` read as
``torch.float64`` and ``Tensor.float()`` as ``Tensor.double()`` (the box class casts what it is given to float32, the soft labels
are built with ``.float()``).  noise_* is the gap between the two runs.  The scene is
re-drawn (proposal by proposal, prediction row by prediction row) until, in float64, no IoU lies within max(1e-4, 10 noise_iou)
of a threshold in use, no canonical yaw within 0.05 rad of pi / 2, pi or 3 pi / 2, and no corner distance within 1e-3 of the Huber
knee or of a flip tie.
"""
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import box_ops_ref as B  # noqa: E402
import roi_head_ref as R  # noqa: E402
from test_roi_head_host import LOSS_CASES, loss_kwargs  # noqa: E402

ROI_PY = 'mmdet3d/models/roi_heads/fsd_roi_head.py'
HEAD_PY = 'mmdet3d/models/roi_heads/bbox_heads/fsd_bbox_head.py'
SAMPLER_PY = 'mmdet3d/core/bbox/samplers/iou_neg_piecewise_sampler.py'
IOU_PY = 'mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py'
BASE_PY = 'mmdet3d/core/bbox/structures/base_box3d.py'
LIDAR_PY = 'mmdet3d/core/bbox/structures/lidar_box3d.py'
UTILS_PY = 'mmdet3d/core/bbox/structures/utils.py'
CODER_PY = 'mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py'
THRESHOLDS = (0.45, 0.35, 0.55, 0.1, 0.8, 0.65, 0.2, 0.15)


class Cfg(dict):
    """mmcv's ConfigDict as far as the head uses it: cfg.key and cfg.get(key, default)"""
    __getattr__ = dict.__getitem__


class TorchAsFloat64(object):
    """``torch`` for the float64 run: float32 reads as float64"""

    def __getattr__(self, name):
        return torch.float64 if name == 'float32' else getattr(torch, name)


class AssignResult(object):
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class MaxIoUAssigner(object):
    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, iou_calculator=None, ignore_iof_thr=-1, type=None):
        assert ignore_iof_thr <= 0
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou, self.iou_calculator = pos_iou_thr, neg_iou_thr, min_pos_iou, iou_calculator

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        overlaps = self.iou_calculator(gt_bboxes, bboxes)
        num_gts, num_bboxes = overlaps.size(0), overlaps.size(1)
        assigned = overlaps.new_full((num_bboxes,), -1, dtype=torch.long)
        labels = assigned.new_full((num_bboxes,), -1)
        if num_gts == 0 or num_bboxes == 0:
            if num_gts == 0:
                assigned[:] = 0
            return AssignResult(num_gts, assigned, overlaps.new_zeros((num_bboxes,)), labels)
        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
        gt_max_overlaps, _ = overlaps.max(dim=1)
        assigned[(max_overlaps >= 0) & (max_overlaps < self.neg_iou_thr)] = 0
        pos = max_overlaps >= self.pos_iou_thr
        assigned[pos] = argmax_overlaps[pos] + 1
        for i in range(num_gts):
            if gt_max_overlaps[i] >= self.min_pos_iou:
                assigned[overlaps[i, :] == gt_max_overlaps[i]] = i + 1
        pos_inds = torch.nonzero(assigned > 0, as_tuple=False).squeeze(-1)
        labels[pos_inds] = gt_labels[assigned[pos_inds] - 1]
        return AssignResult(num_gts, assigned, max_overlaps, labels)


class SamplingResult(object):
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        if gt_bboxes.numel() == 0:
            assert self.pos_assigned_gt_inds.numel() == 0
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, gt_bboxes.size(-1))
        else:
            self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds, :]
        self.pos_gt_labels = assign_result.labels[pos_inds]

    @property
    def bboxes(self):
        return torch.cat([self.pos_bboxes, self.neg_bboxes])


class RandomSampler(object):
    def __init__(self, num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=True, **kwargs):
        self.num, self.pos_fraction, self.neg_pos_ub, self.add_gt_as_proposals = num, pos_fraction, neg_pos_ub, add_gt_as_proposals
        self.pos_sampler = self.neg_sampler = self
        self.keys, self.position_to_proposal, self.pool_sizes = None, None, []

    def random_choice(self, gallery, num):
        ids = gallery if self.position_to_proposal is None else self.position_to_proposal[gallery]
        order = np.lexsort((ids.numpy(), self.keys[ids.numpy()]))
        return gallery[torch.as_tensor(order[:num])]


def weight_reduce(loss, weight, avg_factor):
    return (loss * weight).sum() / avg_factor


def make_losses(case):
    kw = loss_kwargs(case)
    beta = kw['beta']

    def loss_cls(pred, label, weight, avg_factor):
        return kw['loss_weights'][0] * weight_reduce(F.binary_cross_entropy_with_logits(pred, label.to(pred.dtype), reduction='none'),
                                                     weight, avg_factor)

    def loss_bbox(pred, target, weight, avg_factor):
        d = (pred - target).abs()
        elem = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) if beta > 0 else d
        return kw['loss_weights'][1] * weight_reduce(elem, weight, avg_factor)

    return loss_cls, loss_bbox, kw


def multi_apply(func, *args, **kwargs):
    return tuple(map(list, zip(*map(partial(func, **kwargs) if kwargs else func, *args))))


def bbox3d2roi(bbox_list):
    return torch.cat([torch.cat([b.new_full((b.size(0), 1), i), b], dim=-1) for i, b in enumerate(bbox_list)], dim=0)


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    order = torch.sort(scores, dim=0, descending=True, stable=True)[1]
    keep = B.nms_host(boxes[order].detach().numpy().astype(np.float32), thresh)
    return order[torch.as_tensor(keep, dtype=torch.long)]


class patched(object):
    """Tensor.cuda() as the identity; in the float64 run Tensor.float() as Tensor.double()"""

    def __init__(self, f64):
        self.f64 = f64

    def __enter__(self):
        self.saved = (torch.Tensor.cuda, torch.Tensor.float)
        torch.Tensor.cuda = lambda t, *a, **k: t
        if self.f64:
            torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        torch.Tensor.cuda, torch.Tensor.float = self.saved


def reference_parts(f64):
    """the reference's classes and methods, executed from their source text under ``torch`` (float32 run) or its float64 reading"""
    from oracle import ref_loader as L
    tm = TorchAsFloat64() if f64 else torch
    np_dtype = np.float64 if f64 else np.float32
    iou3d_cuda = types.SimpleNamespace()

    def boxes_overlap_bev_gpu(a, b, out):
        out.copy_(torch.as_tensor(R.bev_matrix(a.numpy().astype(np_dtype), b.numpy().astype(np_dtype), np_dtype, cap=False)))

    iou3d_cuda.boxes_overlap_bev_gpu = boxes_overlap_bev_gpu
    utils = {k: L.load_reference_function(UTILS_PY, k, {'np': np, 'torch': tm}) for k in ('limit_period', 'rotation_3d_in_axis', 'xywhr2xyxyr')}
    from abc import abstractmethod
    base = L.load_reference_class(BASE_PY, 'BaseInstance3DBoxes', dict(utils, np=np, torch=tm, abstractmethod=abstractmethod,
                                                                        iou3d_cuda=iou3d_cuda))
    lidar = L.load_reference_class(LIDAR_PY, 'LiDARInstance3DBoxes', dict(utils, np=np, torch=tm, BaseInstance3DBoxes=base,
                                                                          iou3d_cuda=iou3d_cuda, BasePoints=None,
                                                                          points_in_boxes_gpu=None, boxes_overlap_1to1=None))
    overlaps_fn = L.load_reference_function(IOU_PY, 'bbox_overlaps_3d', {'get_box_type': lambda c: (lidar, None), 'torch': tm})
    calc = L.load_reference_class(IOU_PY, 'BboxOverlaps3D', {'bbox_overlaps_3d': overlaps_fn, 'torch': tm})
    sampler_cls = L.load_reference_class(SAMPLER_PY, 'IoUNegPiecewiseSampler', {'RandomSampler': RandomSampler,
                                                                               'SamplingResult': SamplingResult, 'torch': tm})

    class Sampler(sampler_cls):
        def _sample_neg(self, assign_result, num_expected, **kwargs):
            self.position_to_proposal = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).view(-1)
            try:
                return super()._sample_neg(assign_result, num_expected, **kwargs)
            finally:
                self.position_to_proposal = None

    coder = L.load_reference_class(CODER_PY, 'DeltaXYZWLHRBBoxCoder', {'BaseBBoxCoder': object, 'torch': tm})
    glb = dict(utils, np=np, torch=tm, F=F, LiDARInstance3DBoxes=lidar, AssignResult=AssignResult, multi_apply=multi_apply,
               reduce_mean=lambda t: t, nms_gpu=nms_gpu, nms_normal_gpu=None)
    methods = {name: L.load_reference_method(HEAD_PY, 'FullySparseBboxHead', name, glb)
               for name in ('get_targets', '_get_target_single', 'get_multi_class_soft_label', 'get_class_wise_box_weights', 'loss',
                            'filter_pos_assigned_but_empty_rois', 'get_corner_loss_lidar', 'get_bboxes', 'multi_class_nms')}
    assign_and_sample = L.load_reference_method(ROI_PY, 'GroupCorrectionHead', '_assign_and_sample', glb)
    return dict(lidar=lidar, calc=calc, sampler=Sampler, coder=coder, methods=methods, assign_and_sample=assign_and_sample,
                dtype=torch.float64 if f64 else torch.float32)


def train_cfg(case='main'):
    kw = loss_kwargs(case)
    cfg = Cfg(cls_pos_thr=R.WAYMO_CFG['cls_pos_thr'], cls_neg_thr=R.WAYMO_CFG['cls_neg_thr'], sync_reg_avg_factor=True,
              sync_cls_avg_factor=True, corner_loss_only_car=kw['car_index'] >= 0, class_names=R.WAYMO_NAMES)
    if kw['code_weight'] is not None:
        cfg['rcnn_code_weights'] = kw['code_weight']
    return cfg


def make_head(parts, case='main'):
    head = types.SimpleNamespace(num_classes=3, with_corner_loss=True, corner_loss_weight=loss_kwargs(case)['loss_weights'][2],
                                 bbox_coder=parts['coder'](), train_cfg=train_cfg(case), print_info={},
                                 test_cfg=Cfg(use_rotate_nms=True, nms_pre=-1, nms_thr=0.25, score_thr=0.1, min_bbox_size=0, max_num=500))
    head.loss_cls, head.loss_bbox, _ = make_losses(case)
    for name, fn in parts['methods'].items():
        setattr(head, name, types.MethodType(fn, head))
    return head


def run_assign(parts, scene, keys):
    """_assign_and_sample of the reference -> its sampling results, the assignment in the library's convention, the pool sizes"""
    props, plabels, gts, glabels = scene
    dt = parts['dtype']
    cfg = R.WAYMO_CFG
    roi_head = types.SimpleNamespace()
    roi_head.bbox_assigner = [MaxIoUAssigner(cfg['pos_iou_thr'][c], cfg['neg_iou_thr'][c], cfg['min_pos_iou'][c], parts['calc']('lidar'))
                              for c in range(3)]
    sampler = parts['sampler'](num=cfg['num'], pos_fraction=cfg['pos_fraction'], neg_piece_fractions=cfg['neg_iou_piece_thrs'] and
                               cfg['neg_piece_fractions'], neg_iou_piece_thrs=cfg['neg_iou_piece_thrs'], neg_pos_ub=-1,
                               add_gt_as_proposals=False, return_iou=True)
    roi_head.bbox_sampler = sampler
    results, assigned, mats = [], [], []
    p0 = g0 = 0
    with patched(False):
        for s in range(len(props)):
            n = max(len(props[s]), 1)
            sampler.keys = keys[p0:p0 + n]
            boxes = parts['lidar'](torch.as_tensor(props[s]).to(dt), box_dim=props[s].shape[1])
            proposal = (boxes, torch.zeros(len(props[s])), torch.as_tensor(plabels[s]))
            gt = parts['lidar'](torch.as_tensor(gts[s]).to(dt), box_dim=gts[s].shape[1])
            res = parts['assign_and_sample'](roi_head, [proposal], [gt], [torch.as_tensor(glabels[s])])[0]
            gt_inds = res_assign_inds(roi_head, parts, proposal, gt, torch.as_tensor(glabels[s]))
            assigned.append(np.where(gt_inds > 0, gt_inds - 1 + g0, np.where(gt_inds == 0, -1, -2)))
            results.append(res)
            if len(gts[s]) and len(props[s]):
                mats.append(parts['calc']('lidar')(boxes.tensor[:, :7], gt.tensor[:, :7]).numpy())
            p0, g0 = p0 + n, g0 + len(gts[s])
    return results, np.concatenate(assigned).astype(np.int32), mats


def res_assign_inds(roi_head, parts, proposal, gt, gt_labels):
    """gt_inds of the merged AssignResult (the sampling result does not keep it): the assigner loop of _assign_and_sample is run
    once more with a sampler that records what it is handed"""
    seen = {}

    class Spy(object):
        def sample(self, assign_result, *args, **kwargs):
            seen['gt_inds'] = assign_result.gt_inds.clone().numpy()
            return None

    spy_head = types.SimpleNamespace(bbox_assigner=roi_head.bbox_assigner, bbox_sampler=Spy())
    parts['assign_and_sample'](spy_head, [proposal], [gt], [gt_labels])
    return seen['gt_inds']


def rows_of(results, scene):
    """the reference's sampling results in the library's row layout (positives, then negatives, per sample)"""
    props, _ = R.with_fake_boxes(scene[0], scene[1])
    out = dict(src=[], gt_index=[], labels=[], reg_mask=[], iou=[], counts=[])
    p0 = g0 = 0
    for s, res in enumerate(results):
        n_pos, n_neg = len(res.pos_inds), len(res.neg_inds)
        out['src'].append(torch.cat([res.pos_inds, res.neg_inds]).numpy() + p0)
        out['gt_index'].append(np.concatenate([res.pos_assigned_gt_inds.numpy() + g0, np.full(n_neg, -1)]))
        out['labels'].append(np.concatenate([res.pos_gt_labels.numpy(), np.full(n_neg, -1)]))
        out['reg_mask'].append(np.concatenate([np.ones(n_pos), np.zeros(n_neg)]))
        out['iou'].append(res.iou.numpy())
        out['counts'].append((n_pos, n_neg))
        p0, g0 = p0 + len(props[s]), g0 + len(scene[2][s])
    res = {k: np.concatenate(v) for k, v in out.items() if k != 'counts'}
    res['counts'] = np.asarray(out['counts'], np.int32)
    return res


def run_targets(parts, results, case='main'):
    head = make_head(parts, case)
    with patched(parts['dtype'] == torch.float64):
        return head, head.get_targets(results, head.train_cfg)


def run_loss(parts, results, case, cls_score, bbox_pred, nonempty):
    head, targets = run_targets(parts, results, case)
    dt = parts['dtype']
    z = torch.as_tensor(cls_score).to(dt).requires_grad_(True)
    bp = torch.as_tensor(bbox_pred).to(dt).requires_grad_(True)
    rois = bbox3d2roi([r.bboxes for r in results])
    with patched(parts['dtype'] == torch.float64):
        losses = head.loss(z, bp, torch.as_tensor(nonempty), rois, *targets)
    total = losses['loss_rcnn_cls'] + losses['loss_rcnn_bbox'] + losses['loss_rcnn_corner']
    total.backward()
    grad = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()                 # noqa: E731
    return dict(loss_cls=float(losses['loss_rcnn_cls'].detach()), loss_bbox=float(losses['loss_rcnn_bbox'].detach()),
                loss_corner=float(losses['loss_rcnn_corner'].detach()), num_pos=int(losses['num_pos_rois']),
                num_neg=int(losses['num_neg_rois']), d_cls=grad(z), d_bbox=grad(bp))


# ---- the scene -------------------------------------------------------------------------------------------------------

def draw_scene(rng):
    g = R.random_boxes(rng, 14, 7, 22.0)
    g[:, 6] = rng.uniform(-np.pi, np.pi, 14)
    gl = np.array([0, 0, 1, 2, 0, 1, -1, 0, 2, 1, 0, 0, 2, 1], np.int64)
    g[gl == 1, 3:5] = rng.uniform(0.6, 1.0, (int((gl == 1).sum()), 2))
    # box 11 overlaps box 10 (both cars): a proposal on box 10 is the best box 11 gets
    g[10, 3:7] = np.float32([2.0, 4.5, 1.6, 0.3])
    g[11] = g[10] + np.float32([0.4, 0.3, 0.05, 0.1, 0.1, 0.0, 0.05])
    g[12, 0:2] = np.float32([60, 60])          # a cyclist nobody proposes
    n = 420
    of = rng.integers(0, 11, n)
    scale = rng.choice([0.05, 0.15, 0.35, 0.7, 1.2], n, p=[0.2, 0.25, 0.25, 0.2, 0.1])[:, None]
    p = g[of] + (rng.normal(0, 1, (n, 7)) * np.array([0.8, 0.8, 0.3, 0.3, 0.5, 0.2, 0.3]) * scale).astype(np.float32)
    p[:, 6] += rng.choice([0, np.pi, 2 * np.pi, -np.pi], n).astype(np.float32)      # headings of either sense, beyond +-pi
    pl = np.where(gl[of] >= 0, gl[of], 0)
    wrong = rng.random(n) < 0.1
    pl[wrong] = rng.integers(0, 3, int(wrong.sum()))
    far = rng.random(n) < 0.25
    p[far] = R.random_boxes(rng, int(far.sum()), 7, 22.0)
    p[:, 3:6] = np.maximum(p[:, 3:6], 0.3)
    pl[5], pl[6] = 4, -1                        # labels outside the classes
    # one weak proposal on box 9 alone: positive by low-quality matching only
    lone = of == 9
    p[lone] = R.random_boxes(rng, int(lone.sum()), 7, 22.0)
    p[7], pl[7] = g[9] + np.float32([0.35, 0.3, 0.0, 0.1, 0.1, 0.0, 0.2]), 1
    # one proposal sits between boxes 10 and 11: its best box is 10, and it is the best box 11 gets - every proposal that
    # overlaps box 11 as much is moved away
    p[8], pl[8] = g[10] + np.float32([0.12, 0.08, 0.0, 0.0, 0.0, 0.0, 0.02]), 0
    to11 = R.overlaps3d(p, g[11:12], np.float64)[:, 0]
    p[(to11 >= to11[8] - 0.02) & (np.arange(n) != 8), 0:2] += np.float32(120)
    p[9], pl[9] = p[8].copy(), 0               # an exact duplicate: a bit-equal tie
    props = [p.astype(np.float32), np.zeros((0, 7), np.float32), R.random_boxes(rng, 40, 7, 22.0)]
    plabels = [pl.astype(np.int64), np.zeros(0, np.int64), rng.integers(0, 3, 40).astype(np.int64)]
    gts = [g, R.random_boxes(rng, 3, 7, 22.0), np.zeros((0, 7), np.float32)]
    glabels = [gl, np.array([0, 1, 2], np.int64), np.zeros(0, np.int64)]
    return props, plabels, gts, glabels


def settle_scene(rng, scene, margin):
    """re-draw the proposals of sample 0 whose float64 IoU lies near a threshold or whose canonical yaw lies near an edge"""
    props, plabels, gts, glabels = scene
    for _ in range(200):
        iou = R.overlaps3d(props[0], gts[0], np.float64)
        near = np.zeros(len(props[0]), bool)
        for thr in THRESHOLDS:
            near |= ((np.abs(iou - thr) <= 2 * margin) & (iou > 0)).any(1)
        best = iou.argmax(1)
        yaw = R.canonical_yaw(props[0][:, :7], gts[0][best])
        for k in range(len(gts[0])):        # any box the proposal may be sent to
            y = R.canonical_yaw(props[0][:, :7], np.repeat(gts[0][k:k + 1], len(props[0]), 0))
            for edge in (np.pi / 2, np.pi, 3 * np.pi / 2):
                near |= (np.abs(y - edge) <= 0.06) & (iou[:, k] > 0.05)
        del yaw
        if not near.any():
            return scene
        idx = np.nonzero(near)[0]
        props[0][idx, 6] += rng.uniform(0.13, 0.3, len(idx)).astype(np.float32)
        props[0][idx, 0] += rng.uniform(-0.05, 0.05, len(idx)).astype(np.float32)
        if near[8] or near[9]:
            props[0][9] = props[0][8]
    raise RuntimeError('the scene does not settle')


def f16(x):
    return x.astype(np.float16).astype(np.float32)


def settle_predictions(rng, bbox_pred, rows, gts):
    """re-draw prediction rows whose corner distances lie near the Huber knee or a flip tie (float64)"""
    pos = np.nonzero(rows['reg_mask'] == 1)[0]
    gt = torch.as_tensor(gts[rows['gt_index'][pos], :7].astype(np.float64))
    roi = torch.as_tensor(rows['rois'][pos, 1:8].astype(np.float64))
    for _ in range(200):
        d0, d1 = R.corner_distances(R.decode_rows(roi, torch.as_tensor(bbox_pred[pos].astype(np.float64))), gt)
        bad = (((torch.min(d0, d1) - 1).abs() <= 2e-3) | ((d0 - d1).abs() <= 2e-3)).any(1).numpy()
        if not bad.any():
            return bbox_pred
        bbox_pred[pos[bad]] = f16(rng.normal(0, 1, (int(bad.sum()), 7)) * np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2, 0.4]))
    raise RuntimeError('the predictions do not settle')


def main():
    rng = np.random.default_rng(20315)
    p32, p64 = reference_parts(False), reference_parts(True)
    scene = draw_scene(rng)
    keys = R.make_keys(77, scene[0])
    noise_iou = 1e-5
    for attempt in range(5):
        scene = settle_scene(rng, scene, max(1e-4, 10 * noise_iou))
        res32, assigned32, mats32 = run_assign(p32, scene, keys)
        res64, assigned64, mats64 = run_assign(p64, scene, keys)
        noise_iou = max(float(np.abs(a - b).max()) for a, b in zip(mats32, mats64))
        used = np.concatenate([m[m > 0] for m in mats64])
        if all(np.abs(used - thr).min() > max(1e-4, 10 * noise_iou) for thr in THRESHOLDS):
            break
    else:
        raise RuntimeError('no scene found')
    rows32, rows64 = rows_of(res32, scene), rows_of(res64, scene)
    assert np.array_equal(assigned32, assigned64)
    assert np.array_equal(scene[0][0][8], scene[0][0][9]) and assigned64[8] == assigned64[9] == 11      # re-routed from box 10, a tie
    for k in ('src', 'gt_index', 'labels', 'reg_mask', 'counts'):
        assert np.array_equal(rows32[k], rows64[k]), k
    out = {'keys': keys, 'noise_iou': np.float64(noise_iou), 'assigned': assigned32, 'counts': rows32['counts'],
           'gts': np.concatenate(scene[2]), 'duplicate_pair': np.array([8, 9])}
    for s in range(3):
        out[f'props{s}'], out[f'plabels{s}'], out[f'gts{s}'], out[f'glabels{s}'] = (part[s] for part in scene)
    # the sampler's pools of sample 0: positives, then the two negative pieces, from the merged assignment
    a0 = assigned64[:len(scene[0][0])]
    mx = np.zeros(len(a0))
    mx_rows = dict(zip(rows64['src'], rows64['iou']))
    restated = R.assign_sample(*scene, R.WAYMO_CFG, keys, np.float64)
    out['pool_sizes0'] = np.asarray(restated['pool_sizes'][0], np.int64)
    del mx, mx_rows, a0
    props_f, _ = R.with_fake_boxes(scene[0], scene[1])
    all_props = np.concatenate(props_f)
    rois = np.concatenate([rows32['src'][:, None] * 0, all_props[rows32['src']]], 1).astype(np.float32)
    sample_of = np.repeat(np.arange(3), rows32['counts'].sum(1))
    rois[:, 0] = sample_of
    for k in ('src', 'gt_index'):
        out['rows_' + k] = rows32[k].astype(np.int32)
    out['rows_labels'], out['rows_reg_mask'], out['rows_rois'] = rows32['labels'].astype(np.int64), rows32['reg_mask'].astype(np.uint8), rois
    out['rows_iou_f32'], out['rows_iou_f64'] = rows32['iou'].astype(np.float32), rows64['iou'].astype(np.float64)
    # targets and soft labels: get_targets of the reference
    for tag, parts, results in (('f32', p32, res32), ('f64', p64, res64)):
        _, tg = run_targets(parts, results)
        label, bbox_targets, batch_idx, pos_gt_bboxes, pos_gt_labels, reg_mask = tg[:6]
        assert torch.equal(reg_mask, torch.as_tensor(rows32['reg_mask']).long()) and torch.equal(pos_gt_labels, torch.as_tensor(
            rows32['labels'][rows32['reg_mask'] == 1]))
        full = np.zeros((len(rois), 7), np.float64)
        full[rows32['reg_mask'] == 1] = bbox_targets.numpy()
        out[f'rows_soft_label_{tag}'] = label.numpy().astype(np.float32 if tag == 'f32' else np.float64)
        out[f'rows_targets_{tag}'] = full.astype(np.float32 if tag == 'f32' else np.float64)
        assert np.array_equal(pos_gt_bboxes.numpy(), out['gts'][rows32['gt_index'][rows32['reg_mask'] == 1]].astype(pos_gt_bboxes.numpy().dtype))
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))   # noqa: E731
    out['noise_soft_label'] = np.float64(rel(out['rows_soft_label_f32'], out['rows_soft_label_f64']))
    out['noise_targets'] = np.float64(rel(out['rows_targets_f32'], out['rows_targets_f64']))
    out['noise_iou_rows'] = np.float64(np.abs(out['rows_iou_f32'] - out['rows_iou_f64']).max())

    # predictions exactly representable in float16 (stored as such)
    n = len(rois)
    cls_score = f16(rng.normal(-1, 2, (n, 1)))
    bbox_pred = f16(rng.normal(0, 1, (n, 7)) * np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2, 0.4]))
    rows = dict(reg_mask=out['rows_reg_mask'], gt_index=out['rows_gt_index'], rois=rois)
    bbox_pred = settle_predictions(rng, bbox_pred, rows, out['gts'])
    out['cls_score'], out['bbox_pred'] = cls_score.astype(np.float16), bbox_pred.astype(np.float16)
    pos, car = out['rows_reg_mask'] == 1, out['rows_labels'] == 0
    base = rng.random(n) < 0.85
    base[np.nonzero(pos)[0][:3]] = False            # positive RoIs the extractor leaves empty
    base[np.nonzero(pos & car)[0][3:8]] = True
    masks = dict(main=base, smooth=base, nopos=base & ~pos, nocar=base & ~(pos & car))
    for case in LOSS_CASES:
        nonempty = masks[case]
        out[f'{case}_nonempty'] = nonempty
        r32 = run_loss(p32, res32, case, cls_score, bbox_pred, nonempty)
        r64 = run_loss(p64, res64, case, cls_score, bbox_pred, nonempty)
        kw = loss_kwargs(case)
        out[f'{case}_num_pos'], out[f'{case}_num_neg'] = np.int64(r64['num_pos']), np.int64(r64['num_neg'])
        out[f'{case}_corner_rows'] = np.int64((pos & nonempty & (car | (kw['car_index'] < 0))).sum())
        for k in ('loss_cls', 'loss_bbox', 'loss_corner'):
            out[f'{case}_f32_{k}'], out[f'{case}_f64_{k}'] = np.float32(r32[k]), np.float64(r64[k])
            out[f'noise_{case}_{k}'] = np.float64(abs(r32[k] - r64[k]) / abs(r64[k]) if r64[k] else abs(r32[k]))
        for k in ('d_cls', 'd_bbox'):
            out[f'{case}_f64_{k}'] = r64[k]
            out[f'noise_{case}_{k}'] = np.float64(rel(r32[k], r64[k]) if np.abs(r64[k]).max() else np.abs(r32[k]).max())
        print(case, {k: v for k, v in r64.items() if not k.startswith('d_')}, 'corner rows', int(out[f'{case}_corner_rows']))

    # decoding and get_bboxes: one sample, the first 220 proposals of sample 0 as RoIs
    m = 220
    t_rois = np.concatenate([np.zeros((m, 1), np.float32), scene[0][0][:m]], 1)
    t_z, t_bp = f16(rng.normal(0, 2, (m, 1))), f16(rng.normal(0, 1, (m, 7)) * np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2, 0.4]))
    t_valid = rng.random(m) < 0.9
    t_labels = np.clip(scene[1][0][:m], 0, 2)
    t_scores = (rng.random(m).astype(np.float32) * 0.9 + 0.05).astype(np.float32)
    t_scores = (t_scores + np.arange(m, dtype=np.float32) * 1e-4).astype(np.float32)       # no two scores equal
    sel = {}
    for tag, parts in (('f32', p32), ('f64', p64)):
        head = make_head(parts)
        dt = parts['dtype']
        metas = [dict(box_type_3d=parts['lidar'])]
        with patched(dt == torch.float64):
            res = head.get_bboxes(torch.as_tensor(t_rois).to(dt), torch.as_tensor(t_z).to(dt), torch.as_tensor(t_bp).to(dt),
                                  torch.as_tensor(t_valid), [torch.as_tensor(t_labels)], [torch.as_tensor(t_scores)], metas,
                                  cfg=head.test_cfg)
        boxes, scores, labels = res[0]
        # the decoded boxes of all RoIs: the same call with nothing filtered and nothing suppressed
        every = make_head(parts)
        every.test_cfg = Cfg(every.test_cfg, nms_thr=2.0, score_thr=0.0)
        with patched(dt == torch.float64):
            full = every.get_bboxes(torch.as_tensor(t_rois).to(dt), torch.as_tensor(t_z).to(dt), torch.as_tensor(t_bp).to(dt),
                                    torch.ones(m, dtype=torch.bool), [torch.as_tensor(t_labels)],
                                    [torch.as_tensor(-np.arange(m, dtype=np.float32) + m)], metas, cfg=every.test_cfg)[0]
        order = np.concatenate([np.nonzero(t_labels == k)[0] for k in range(3)])
        decoded = np.zeros((m, 7))
        decoded[order] = full[0].tensor.numpy()
        valid = np.nonzero(t_valid)[0]
        selected = np.asarray([int(np.nonzero((decoded[valid] == b).all(1))[0][0]) for b in boxes.tensor.numpy()], np.int64)
        sel[tag] = (decoded, selected)
    assert np.array_equal(sel['f32'][1], sel['f64'][1])
    out.update(test_rois=t_rois, test_cls_score=t_z.astype(np.float16), test_bbox_pred=t_bp.astype(np.float16), test_valid=t_valid,
               test_labels=t_labels.astype(np.int64), test_scores=t_scores, test_boxes_f64=sel['f64'][0],
               test_selected=sel['f64'][1], noise_test_boxes=np.float64(rel(sel['f32'][0], sel['f64'][0])))
    path = os.path.join(ROOT, 'tests', 'golden', 'roi_head_train.npz')
    np.savez_compressed(path, **out)
    print('counts', out['counts'].tolist(), 'pools', out['pool_sizes0'], 'noise_iou', noise_iou, 'kept', len(out['test_selected']))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
