"""Generates tests/golden/anchor_head_train.npz: Anchor3DHead's anchors, targets, losses and box extraction as the REFERENCE
computes them (data only).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_anchor_head_train.py

Executed from their source text: Anchor3DRangeGenerator / AlignedAnchor3DRangeGenerator (mmdet3d/core/anchor/
anchor_3d_generator.py), AnchorTrainMixin and get_direction_target (mmdet3d/models/dense_heads/train_mixins.py), Anchor3DHead.loss
/ loss_single / add_sin_difference / get_bboxes / get_bboxes_single (dense_heads/anchor3d_head.py), bbox_overlaps_nearest_3d and
BboxOverlapsNearest3D (core/bbox/iou_calculators/iou3d_calculator.py), BaseInstance3DBoxes / LiDARInstance3DBoxes with
nearest_bev and bev (core/bbox/structures), limit_period and xywhr2xyxyr (core/bbox/structures/utils.py),
DeltaXYZWLHRBBoxCoder (core/bbox/coders/delta_xyzwhlr_bbox_coder.py), box3d_multiclass_nms (core/post_processing/box3d_nms.py).
What the reference imports from packages that are not in its tree is stood in for here:
  mmdet bbox_overlaps           areas (x2 - x1) * (y2 - y1), intersection clamp(min(x2) - max(x1), 0) * clamp(...), union
                                max(a1 + a2 - inter, 1e-6), inter / union (mmdet 2.x, mode 'iou', not aligned)
  mmdet MaxIoUAssigner          assign / assign_wrt_overlaps with match_low_quality and gt_max_assign_all at their defaults
  mmdet AssignResult, SamplingResult, PseudoSampler   the fields the mixin reads
  mmdet FocalLoss               py_sigmoid_focal_loss (tests/anchor_head_ref.py) x loss_weight, reduction 'mean' with avg_factor
  mmdet L1Loss / SmoothL1Loss   (|d| or smooth L1(beta)) * weight, summed / avg_factor x loss_weight
  mmdet CrossEntropyLoss        F.cross_entropy(reduction='none') * weight, summed / avg_factor x loss_weight
  mmdet images_to_levels        stack, then split by the level sizes
  mmdet multi_apply             tuple(map(list, zip(*map(partial(func, **kwargs), *args))))
  mmcv.is_list_of               all(isinstance(x, type))
  nms_gpu                       tests/box_ops_ref.nms_host over the boxes sorted by descending score
Every loss case is run in float32 and in float64 (the float64 run must reproduce the float32 run's assignment); noise_* is the
gap between the two runs: relative for the loss scalars, relative to the tensor's maximum for the gradients.
"""
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import anchor_head_ref as R  # noqa: E402
import box_ops_ref as B  # noqa: E402

GEN_PY = 'mmdet3d/core/anchor/anchor_3d_generator.py'
MIXIN_PY = 'mmdet3d/models/dense_heads/train_mixins.py'
HEAD_PY = 'mmdet3d/models/dense_heads/anchor3d_head.py'
IOU_PY = 'mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py'
UTILS_PY = 'mmdet3d/core/bbox/structures/utils.py'
BASE_PY = 'mmdet3d/core/bbox/structures/base_box3d.py'
LIDAR_PY = 'mmdet3d/core/bbox/structures/lidar_box3d.py'
CODER_PY = 'mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py'
NMS_PY = 'mmdet3d/core/post_processing/box3d_nms.py'

NMS_MARGIN = 1e-3      # >= max(1e-4, 10 x the float32 noise of an IoU, ~1e-6)


class Cfg(dict):
    """a config dict with attribute access (mmcv ConfigDict)"""
    __getattr__ = dict.get


class AssignResult(object):
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


MAX_LOG = []           # (max_overlaps per anchor) of every assign call, in call order


class MaxIoUAssigner(object):
    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, iou_calculator=None, ignore_iof_thr=-1, type=None):
        assert ignore_iof_thr <= 0
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou, self.iou_calculator = pos_iou_thr, neg_iou_thr, min_pos_iou, iou_calculator

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        overlaps = self.iou_calculator(gt_bboxes, bboxes)
        num_gts, num_bboxes = overlaps.size(0), overlaps.size(1)
        assigned = overlaps.new_full((num_bboxes,), -1, dtype=torch.long)
        labels = assigned.new_full((num_bboxes,), -1)
        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
        gt_max_overlaps, _ = overlaps.max(dim=1)
        MAX_LOG.append(max_overlaps.clone())
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
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds, :]


class PseudoSampler(object):
    def sample(self, assign_result, bboxes, gt_bboxes, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result)


def bbox_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False, eps=1e-6):
    assert mode == 'iou' and not is_aligned
    area1 = (bboxes1[..., 2] - bboxes1[..., 0]) * (bboxes1[..., 3] - bboxes1[..., 1])
    area2 = (bboxes2[..., 2] - bboxes2[..., 0]) * (bboxes2[..., 3] - bboxes2[..., 1])
    lt = torch.max(bboxes1[..., :, None, :2], bboxes2[..., None, :, :2])
    rb = torch.min(bboxes1[..., :, None, 2:], bboxes2[..., None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1[..., None] + area2[..., None, :] - overlap
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


def multi_apply(func, *args, **kwargs):
    return tuple(map(list, zip(*map(partial(func, **kwargs) if kwargs else func, *args))))


def images_to_levels(target, num_levels):
    target = torch.stack(target, 0)
    out, start = [], 0
    for n in num_levels:
        out.append(target[:, start:start + n])
        start += n
    return out


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    order = torch.sort(scores, dim=0, descending=True, stable=True)[1]
    keep = B.nms_host(boxes[order].detach().numpy().astype(np.float32), thresh)
    return order[torch.as_tensor(keep, dtype=torch.long)]


_PARTS = {}


def reference_parts():
    if _PARTS:
        return _PARTS
    import types
    from abc import abstractmethod
    from oracle import ref_loader as L
    utils = {k: L.load_reference_function(UTILS_PY, k, {'np': np}) for k in ('limit_period', 'rotation_3d_in_axis', 'xywhr2xyxyr')}
    base = L.load_reference_class(BASE_PY, 'BaseInstance3DBoxes', dict(utils, np=np, abstractmethod=abstractmethod, iou3d_cuda=None))
    lidar = L.load_reference_class(LIDAR_PY, 'LiDARInstance3DBoxes', dict(utils, np=np, BaseInstance3DBoxes=base, BasePoints=None,
                                                                          points_in_boxes_gpu=None, boxes_overlap_1to1=None))
    nearest = L.load_reference_function(IOU_PY, 'bbox_overlaps_nearest_3d', {'get_box_type': lambda c: (lidar, None),
                                                                             'bbox_overlaps': bbox_overlaps})
    calc = L.load_reference_class(IOU_PY, 'BboxOverlapsNearest3D', {'bbox_overlaps_nearest_3d': nearest})
    mmcv = types.SimpleNamespace(is_list_of=lambda seq, t: isinstance(seq, list) and all(isinstance(x, t) for x in seq))
    gen = L.load_reference_class(GEN_PY, 'Anchor3DRangeGenerator', {'mmcv': mmcv})
    aligned = L.load_reference_class(GEN_PY, 'AlignedAnchor3DRangeGenerator', {'Anchor3DRangeGenerator': gen})
    direction = L.load_reference_function(MIXIN_PY, 'get_direction_target', {'np': np, 'limit_period': utils['limit_period']})
    mixin = L.load_reference_class(MIXIN_PY, 'AnchorTrainMixin', {'np': np, 'limit_period': utils['limit_period'],
                                                                  'images_to_levels': images_to_levels, 'multi_apply': multi_apply,
                                                                  'get_direction_target': direction})
    coder = L.load_reference_class(CODER_PY, 'DeltaXYZWLHRBBoxCoder', {'BaseBBoxCoder': object})
    nms = L.load_reference_function(NMS_PY, 'box3d_multiclass_nms', {'nms_gpu': nms_gpu, 'nms_normal_gpu': None})
    glb = {'np': np, 'multi_apply': multi_apply, 'limit_period': utils['limit_period'], 'xywhr2xyxyr': utils['xywhr2xyxyr'],
           'box3d_multiclass_nms': nms, 'box3d_multiclass_wnms': None}
    methods = {k: L.load_reference_method(HEAD_PY, 'Anchor3DHead', k, glb)
               for k in ('loss', 'loss_single', 'add_sin_difference', 'get_anchors', 'get_bboxes', 'get_bboxes_single')}
    methods['add_sin_difference'] = staticmethod(methods['add_sin_difference'])
    _PARTS.update(lidar=lidar, calc=calc, gens=dict(Anchor3DRangeGenerator=gen, AlignedAnchor3DRangeGenerator=aligned),
                  head=type('Head', (mixin,), methods), coder=coder)
    return _PARTS


def weight_reduce(loss, weight, avg_factor):
    return (loss * weight).sum() / avg_factor


def make_head(case):
    """a stand-in ``self`` for the reference's methods, with the case's settings"""
    parts, cfg = reference_parts(), R.CASES[case]
    head = parts['head']()
    head.num_classes, head.box_code_size = cfg['num_classes'], 7
    head.use_direction_classifier, head.diff_rad_by_sin = cfg['use_direction_classifier'], cfg['diff_rad_by_sin']
    head.dir_offset, head.dir_limit_offset = cfg['dir_offset'], cfg['dir_limit_offset']
    head.assign_per_class, head.sampling, head.use_sigmoid_cls = cfg['assign_per_class'], False, True
    head.train_cfg, head.test_cfg = Cfg(cfg['train_cfg']), Cfg(cfg['test_cfg'])
    gen = dict(cfg['anchor_generator'])
    head.anchor_generator = parts['gens'][gen.pop('type')](**gen)
    head.num_anchors = head.anchor_generator.num_base_anchors
    head.cls_out_channels = head.num_anchors * head.num_classes
    head.bbox_coder = parts['coder'](code_size=7)
    head.bbox_sampler = PseudoSampler()
    head.bbox_assigner = [MaxIoUAssigner(**dict(a, iou_calculator=parts['calc']())) for a in cfg['train_cfg']['assigner']]
    lc, lb, ld = cfg['loss_cls'], cfg['loss_bbox'], cfg['loss_dir']

    def loss_cls(pred, label, weight, avg_factor):
        c = pred.size(1)
        return lc.get('loss_weight', 1.0) * R.py_sigmoid_focal_loss(pred, F_.one_hot(label, c + 1)[:, :c], weight,
                                                                    lc.get('gamma', 2.0), lc.get('alpha', 0.25), avg_factor)

    def loss_bbox(pred, target, weight, avg_factor):
        return lb.get('loss_weight', 1.0) * R.box_loss(pred, target, weight, avg_factor,
                                                       lb.get('beta', 1.0) if lb['type'] == 'SmoothL1Loss' else None)

    def loss_dir(pred, label, weight, avg_factor):
        return ld.get('loss_weight', 1.0) * weight_reduce(F_.cross_entropy(pred, label, reduction='none'), weight, avg_factor)

    head.loss_cls, head.loss_bbox, head.loss_dir = loss_cls, loss_bbox, loss_dir
    return head


def make_scene(rng):
    """three samples of 7-column boxes and labels (0 car, 1 cyclist, 2 pedestrian); the middle one has no boxes"""
    sizes = np.float32([[2.08, 4.73, 1.77], [0.84, 1.81, 1.77], [0.84, 0.91, 1.74]])
    zs = np.float32([-0.0345, -0.1188, 0.0])

    def random_boxes(n):
        kind = rng.integers(0, 3, n)
        b = np.zeros((n, 7), np.float32)
        b[:, 0] = rng.uniform(R.RANGE_XY[0] + 0.5, R.RANGE_XY[2] - 0.5, n)
        b[:, 1] = rng.uniform(R.RANGE_XY[1] + 0.5, R.RANGE_XY[3] - 0.5, n)
        b[:, 3:6] = sizes[kind] * rng.uniform(0.85, 1.2, (n, 3))
        b[:, 2] = zs[kind] - b[:, 5] / 2 + rng.normal(0, 0.15, n)
        # yaws near the anchors' (0, pi / 2 and their opposites), as objects along the lanes are
        b[:, 6] = rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2], n) + rng.normal(0, 0.25, n)
        return b, kind.astype(np.int64)

    scenes = []
    for s in range(2):
        b, lab = random_boxes(14)
        if s == 0:
            b[0, :2], b[0, 3:6] = [R.RANGE_XY[2] + 4.0, 1.0], [0.85, 0.95, 1.7]   # outside the anchor range: matches nothing
            lab[0] = 2
            b[1, :2], b[2, :2] = [2.25, -3.1], [2.4, -2.95]               # two pedestrians, one cell
            b[1, 3:6], b[2, 3:6] = [0.8, 0.9, 1.7], [0.9, 0.85, 1.8]
            b[1, 6], b[2, 6] = 0.1, 1.4
            lab[1] = lab[2] = 2
            b[3, :2], b[3, 3:6], b[3, 6] = [-4.37, 3.3], [1.1, 2.6, 1.7], 0.05   # a cyclist 1.4 x the anchor: low quality only
            lab[3] = 1
            # on the corner between two cells in x (the float32 midpoint of their centres): two anchors tie, checked in main()
            xs = R.make_grid(R.generator_cfg(), R.H, R.W).xs[2]
            b[4, :2] = [np.float32((np.float64(xs[11]) + np.float64(xs[12])) / 2), -3.52]
            b[4, 3:6], b[4, 6] = [0.8, 0.9, 1.7], 0.02
            lab[4] = 2
        scenes.append((b, lab))
    empty = (np.zeros((0, 7), np.float32), np.zeros((0,), np.int64))
    return [scenes[0], empty, scenes[1]]


def scene_ok(scene):
    for b, _ in scene:
        if len(b) and (np.abs(np.abs(R.limit_period(b[:, 6].astype(np.float64), 0.5, np.pi)) - np.pi / 4) < 1e-3).any():
            return False
    return True


def boxes_of(parts, b, dtype):
    return parts['lidar'](torch.as_tensor(b).to(dtype), box_dim=7)


def reference_targets(head, boxes, labels, dtype=torch.float32):
    """-> (the reference's anchor_target_3d tuple, the per-anchor maxima [B, A], the anchors)"""
    parts = reference_parts()
    metas = [dict(box_type_3d=parts['lidar'])] * len(boxes)
    anchors = head.get_anchors([(R.H, R.W)], metas, device='cpu')
    anchors = [[a.to(dtype) for a in lvl] for lvl in anchors]
    del MAX_LOG[:]
    out = head.anchor_target_3d(anchors, [boxes_of(parts, b, dtype) for b in boxes], metas,
                                gt_labels_list=[torch.as_tensor(l) for l in labels], num_classes=head.num_classes,
                                label_channels=head.cls_out_channels, sampling=False)
    ns = len(head.bbox_assigner)
    nr = head.num_anchors // ns
    maxima, log = [], list(MAX_LOG)
    for b, l in zip(boxes, labels):
        m = torch.zeros((R.H * R.W, ns, nr), dtype=dtype)
        for i in range(ns):
            n_gt = int((np.asarray(l) == i).sum()) if head.assign_per_class else len(b)
            if n_gt > 0:
                m[:, i, :] = log.pop(0).reshape(R.H * R.W, nr)
        maxima.append(m.reshape(-1))
    assert not log
    return out, torch.stack(maxima), anchors[0][0]


def reference_loss(head, boxes, labels, maps, dtype):
    parts = reference_parts()
    metas = [dict(box_type_3d=parts['lidar'])] * len(boxes)
    ts = [torch.as_tensor(m).to(dtype).requires_grad_(True) for m in maps]
    saved = head.get_anchors
    head.get_anchors = lambda sizes, input_metas, device='cpu': [[a.to(dtype) for a in lvl] for lvl in saved(sizes, input_metas, 'cpu')]
    try:
        out = head.loss([ts[0]], [ts[1]], [ts[2]], [boxes_of(parts, b, dtype) for b in boxes], [torch.as_tensor(l) for l in labels],
                        metas)
    finally:
        del head.get_anchors
    total = out['loss_cls'][0] + out['loss_bbox'][0] + out['loss_dir'][0]
    total.backward()
    res = {k: out[k][0].detach().numpy() for k in ('loss_cls', 'loss_bbox', 'loss_dir')}
    res.update(d_cls=ts[0].grad.numpy(), d_bbox=ts[1].grad.numpy(), d_dir=ts[2].grad.numpy())
    return res


def exact_f16(a):
    """values that float16 holds exactly, as float32 (the golden stores them as float16)"""
    return a.astype(np.float16).astype(np.float32)


def make_maps(rng, n_a, c, hot):
    """loss and decode inputs of three samples: mostly low class logits with ``hot`` confident anchors per sample"""
    cls = rng.normal(-4.0, 1.0, (3, n_a * c, R.H, R.W))
    for s in range(3):
        at = rng.choice(n_a * R.H * R.W, hot, replace=False)
        a, cell = at // (R.H * R.W), at % (R.H * R.W)
        k = rng.integers(0, c, hot)
        cls[s].reshape(n_a * c, -1)[a * c + k, cell] = rng.normal(0.5, 1.5, hot)
    box = np.round(rng.normal(0, 0.25, (3, n_a * 7, R.H, R.W)) * 32) / 32     # on a coarse grid: the file stays small
    dirs = np.round(rng.normal(0, 1.0, (3, n_a * 2, R.H, R.W)) * 8) / 8
    return exact_f16(cls), exact_f16(box), exact_f16(dirs)


def settle_decode_inputs(case, cls, box, dirs):
    """lower the class logits of a candidate until no score is within 1e-4 of score_thr and no compared NMS pair's overlap is
    within NMS_MARGIN of nms_thr (the later box of such a pair leaves the candidates)"""
    cfg = R.CASES[case]
    grid = R.make_grid(cfg['anchor_generator'], R.H, R.W)
    tc, c = cfg['test_cfg'], cfg['num_classes']
    n_a = grid.ns * grid.nr
    for s in range(cls.shape[0]):
        for _ in range(50):
            inds, boxes, scores, _, bev = R.candidates(grid, cls[s], box[s], dirs[s], c, tc['nms_pre'])
            bad = set(np.nonzero((np.abs(scores[:, :c] - np.float32(tc['score_thr'])) < 1e-4).any(1))[0].tolist())
            for k in range(c):
                cand = np.nonzero(scores[:, k] > np.float32(tc['score_thr']))[0]
                cand = cand[np.argsort(-scores[cand, k], kind='stable')]
                if len(cand) > 1:
                    bad.update(cand[1:][np.diff(scores[cand, k]) == 0].tolist())      # a score tie: the later one leaves
                    ii, jj = B.near_pairs(bev[cand])
                    if len(ii):
                        iou = B.bev_iou_f32(bev[cand][ii], bev[cand][jj])
                        bad.update(cand[jj[np.abs(iou - np.float32(tc['nms_thr'])) < NMS_MARGIN]].tolist())
            if not bad:
                break
            for i in bad:
                a = inds[i]
                cell, t = a // n_a, a % n_a
                cls[s].reshape(n_a * c, -1)[t * c:(t + 1) * c, cell] = -6.0
        else:
            raise AssertionError('decode inputs did not settle')
    return cls


def main():
    parts = reference_parts()
    out = {}
    seed = 20262
    while True:
        rng = np.random.default_rng(seed)
        scene = make_scene(rng)
        if scene_ok(scene):
            break
        seed += 1
    for s, (b, lab) in enumerate(scene):
        out[f'boxes{s}'], out[f'labels{s}'] = b, lab
    maps = {}
    for case, cfg in R.CASES.items():
        head = make_head(case)
        sel = [R.case_labels(case, lab) for _, lab in scene]
        boxes = [b[k] for (b, _), (k, _) in zip(scene, sel)]
        labels = [l[k] for k, l in sel]
        tg, maxima, anchors = reference_targets(head, boxes, labels)
        n_a, c = head.num_anchors, head.num_classes
        if n_a not in maps:
            maps[n_a] = {}
        if case == 'shipped':
            out['anchors'] = anchors.numpy()
        names = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'dir_targets', 'dir_weights')
        for k, v in zip(names, tg[:6]):
            out[f'tgt_{case}_{k}'] = v[0].numpy()
        out[f'tgt_{case}_num_total_pos'], out[f'tgt_{case}_num_total_neg'] = np.int64(tg[6]), np.int64(tg[7])
        out[f'tgt_{case}_max_iou'] = maxima.numpy()
        grid = R.make_grid(cfg['anchor_generator'], R.H, R.W)
        assert np.array_equal(grid.anchors().reshape(anchors.shape), anchors.numpy()), 'the restated anchors differ'
        dense, per_sample, n_pos, n_neg = R.batch_targets(grid, boxes, labels, cfg)
        assigned = np.stack([p[0].reshape(-1) for p in per_sample])
        out[f'tgt_{case}_assigned'] = assigned
        assert (n_pos, n_neg) == (tg[6], tg[7]), (case, n_pos, n_neg, tg[6], tg[7])
        for k in ('labels', 'label_weights', 'bbox_weights', 'dir_targets', 'dir_weights'):
            assert np.array_equal(dense[k], out[f'tgt_{case}_{k}']), (case, k)
        assert np.array_equal(np.stack([p[1].reshape(-1) for p in per_sample]), out[f'tgt_{case}_max_iou']), case
        pos = assigned >= 0
        print(case, 'positives', pos.sum(1), 'ignored', (assigned == -2).sum(1), 'num_total_pos', tg[6])
        # no direction angle of a positive within 1e-3 of a bin edge
        an = grid.anchors().reshape(-1, 7)
        for s in range(3):
            if pos[s].any():
                off = R.direction_target(an[pos[s]], out[f'tgt_{case}_bbox_targets'][s][pos[s]], cfg['dir_offset'])[1].astype(np.float64)
                assert (np.minimum(np.abs(off - np.pi), np.minimum(off, 2 * np.pi - off)) > 1e-3).all(), 'a direction at a bin edge'
        if case == 'shipped':
            m0, a0 = per_sample[0][2], per_sample[0][0]
            assert (a0 == 0).sum() == 0 and m0[:, 0].max() == 0, 'the box outside the range must match nothing'
            cyc = m0[1, 3]
            assert np.float32(0.3) <= cyc < np.float32(0.5) and (a0 == 3).sum() >= 1, ('low-quality match', cyc)
            tie = (per_sample[0][1][:, :, 2, :] == m0[2, 4]) & (a0[:, :, 2, :] == 4)
            assert tie.sum() >= 2 and m0[2, 4] < np.float32(0.5), ('two anchors at exactly equal IoU', tie.sum(), m0[2, 4])
            cells = {tuple(np.floor((b[:2] - [R.X0, R.Y0]) / R.CELL).astype(int)) for b in scene[0][0][1:3]}
            assert len(cells) == 1, 'two boxes must share a cell'

        # loss inputs (one set per anchor count and class count) and the two runs
        key = (n_a, c)
        if key not in maps[n_a]:
            maps[n_a][key] = make_maps(np.random.default_rng(seed + 7 * c + n_a), n_a, c, hot=90)
            settle_decode_inputs(case, *maps[n_a][key])
            tag = f'{n_a}x{c}'
            for k, m in zip(('cls', 'box', 'dir'), maps[n_a][key]):
                out[f'maps_{tag}_{k}'] = m.astype(np.float16)
                assert np.array_equal(m, out[f'maps_{tag}_{k}'].astype(np.float32))
        cls, box, dirs = maps[n_a][key]
        r32 = reference_loss(head, boxes, labels, (cls, box, dirs), torch.float32)
        tg64, _, _ = reference_targets(head, boxes, labels, torch.float64)
        for k, v in zip(names, tg64[:6]):
            if k != 'bbox_targets':
                assert np.array_equal(v[0].numpy(), out[f'tgt_{case}_{k}']), ('the float64 run assigns differently', case, k)
        r64 = reference_loss(head, boxes, labels, (cls, box, dirs), torch.float64)
        for k in ('loss_cls', 'loss_bbox', 'loss_dir'):
            out[f'loss_{case}_f32_{k}'], out[f'loss_{case}_f64_{k}'] = r32[k], r64[k]
            out[f'noise_{case}_{k}'] = np.abs(r32[k].astype(np.float64) - r64[k]) / np.abs(r64[k])
        for k in ('d_cls', 'd_bbox', 'd_dir'):
            out[f'noise_{case}_{k}'] = np.abs(r32[k].astype(np.float64) - r64[k]).max() / np.abs(r64[k]).max()
        out[f'loss_{case}_f64_d_cls_8th'] = r64['d_cls'].reshape(-1)[::8]
        out[f'loss_{case}_f64_d_cls_abs'] = np.abs(r64['d_cls']).sum()
        out[f'loss_{case}_f64_d_bbox'], out[f'loss_{case}_f64_d_dir'] = r64['d_bbox'], r64['d_dir']
        print(case, {k: float(r64[k]) for k in ('loss_cls', 'loss_bbox', 'loss_dir')},
              'noise', {k: float(out[f'noise_{case}_{k}']) for k in ('loss_cls', 'loss_bbox', 'loss_dir', 'd_cls', 'd_bbox', 'd_dir')})

        # box extraction
        metas = [dict(box_type_3d=parts['lidar'])] * 3
        res = head.get_bboxes([torch.as_tensor(cls)], [torch.as_tensor(box)], [torch.as_tensor(dirs)], metas)
        for s, (bb, sc, lb) in enumerate(res):
            out[f'det_{case}_s{s}_bboxes'], out[f'det_{case}_s{s}_scores'] = bb.tensor.numpy(), sc.numpy()
            out[f'det_{case}_s{s}_labels'] = lb.numpy()
            got = R.get_bboxes_single(grid, cls[s], box[s], dirs[s], cfg)
            assert np.array_equal(got[2], lb.numpy()) and np.array_equal(got[1], sc.numpy()), (case, s)
            assert R.ulp_distance(got[0], bb.tensor.numpy()).max() <= 1, (case, s)
        print(case, 'detections', [len(r[1]) for r in res], 'of', n_a * R.H * R.W, 'anchors, nms_pre', cfg['test_cfg']['nms_pre'])
        assert all(0 < len(r[1]) < cfg['test_cfg']['max_num'] or case == 'smooth' for r in res)
    path = os.path.join(ROOT, 'tests', 'golden', 'anchor_head_train.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
