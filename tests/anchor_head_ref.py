"""Restatement of Anchor3DHead's targets, losses and decoding in numpy / torch on the host, float32 operation by operation where
bits matter (the nearest-BEV IoU, the thresholds, the plain regression targets), plus the scene constants shared by the golden
generator (tests/golden/make_anchor_head_train.py) and the tests.

Reference: mmdet3d/models/dense_heads/train_mixins.py, anchor3d_head.py, core/anchor/anchor_3d_generator.py,
core/bbox/iou_calculators/iou3d_calculator.py:94-140, core/bbox/structures/lidar_box3d.py:123-141,
core/bbox/coders/delta_xyzwhlr_bbox_coder.py; mmdet 2.x bbox_overlaps, MaxIoUAssigner.assign_wrt_overlaps, PseudoSampler,
py_sigmoid_focal_loss, L1Loss / SmoothL1Loss / CrossEntropyLoss with mean reduction and avg_factor.

The IoU of a box is only evaluated on the block of anchors its nearest-BEV rectangle can meet: everywhere else the clamped
extents, hence the IoU, are exactly 0, which is what the dense matrix of the reference holds there.
"""
import numpy as np
import torch
import torch.nn.functional as F_

import box_ops_ref as B
from head_ref_common import ulp_distance  # noqa: F401  (the tests reach it through this module)

F = np.float32
PI = np.pi

# ---- the golden scene: a 20 x 24 map (H != W) of 0.64 m cells, 3 sizes x 2 rotations ----
H, W, CELL = 20, 24, 0.64
X0, Y0 = -7.68, -6.4
RANGE_XY = [X0, Y0, X0 + W * CELL, Y0 + H * CELL]


def generator_cfg(zs=(-0.0345, -0.1188, 0.0), sizes=((2.08, 4.73, 1.77), (0.84, 1.81, 1.77), (0.84, 0.91, 1.74))):
    return dict(type='AlignedAnchor3DRangeGenerator',
                ranges=[[RANGE_XY[0], RANGE_XY[1], z, RANGE_XY[2], RANGE_XY[3], z] for z in zs],
                sizes=[list(s) for s in sizes], rotations=[0, 1.57], reshape_out=False)


def _assigner(pos, neg, low):
    return dict(type='MaxIoUAssigner', iou_calculator=dict(type='BboxOverlapsNearest3D'), pos_iou_thr=pos, neg_iou_thr=neg,
                min_pos_iou=low, ignore_iof_thr=-1)


ASSIGN_3 = [_assigner(0.55, 0.4, 0.4), _assigner(0.5, 0.3, 0.3), _assigner(0.5, 0.3, 0.3)]
TEST_CFG = dict(use_rotate_nms=True, nms_across_levels=False, nms_pre=4096, nms_thr=0.25, score_thr=0.1, min_bbox_size=0,
                max_num=500)


def _head(**kw):
    cfg = dict(num_classes=3, use_direction_classifier=True, anchor_generator=generator_cfg(), assign_per_class=False,
               diff_rad_by_sin=True, dir_offset=0.7854, dir_limit_offset=0,
               loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
               loss_bbox=dict(type='L1Loss', loss_weight=0.5),
               loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.2),
               train_cfg=dict(assigner=ASSIGN_3, allowed_border=0, code_weight=[1.0] * 7, pos_weight=-1, debug=False),
               test_cfg=dict(TEST_CFG))
    cfg.update(kw)
    return cfg


# case -> the head's settings (constructor keys of Anchor3DHead without the channels)
CASES = {
    'shipped': _head(),                                                      # configs/_base_/models/sst_base.py
    'per_class': _head(assign_per_class=True,
                       train_cfg=dict(assigner=ASSIGN_3, code_weight=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5], pos_weight=2.0)),
    'smooth': _head(diff_rad_by_sin=False, loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0),
                    loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=0.4, loss_weight=0.7),
                    test_cfg=dict(TEST_CFG, nms_pre=600, max_num=40)),
    'ped_cyc': _head(num_classes=2,                                          # configs/sst/sst_waymoD5_1x_ped_cyc_8heads_3f.py
                     anchor_generator=generator_cfg(zs=(-0.1188, 0.0), sizes=((0.84, 1.81, 1.77), (0.84, 0.91, 1.74))),
                     train_cfg=dict(assigner=ASSIGN_3[1:], code_weight=[1.0] * 7, pos_weight=-1)),
}


def case_labels(case, labels):
    """the scene's labels (0 car, 1 cyclist, 2 pedestrian) as the case's classes; the 2-class case keeps cyclists and
    pedestrians -> (keep mask, labels)"""
    labels = np.asarray(labels, np.int64)
    if CASES[case]['num_classes'] == 2:
        return labels > 0, labels - 1
    return np.ones(len(labels), bool), labels


# ------------------------------------------------------------------------------------------------------------------
# anchors
# ------------------------------------------------------------------------------------------------------------------

class Grid(object):
    """xs [n_sizes, W], ys [n_sizes, H], zs [n_sizes], sizes [n_sizes, 3], rots [n_rots] as float32 numpy arrays"""

    def __init__(self, xs, ys, zs, sizes, rots):
        self.xs, self.ys, self.zs = np.asarray(xs, F), np.asarray(ys, F), np.asarray(zs, F)
        self.sizes, self.rots = np.asarray(sizes, F).reshape(-1, 3), np.asarray(rots, F)
        self.ns, self.nr, self.H, self.W = len(self.sizes), len(self.rots), self.ys.shape[1], self.xs.shape[1]

    def anchors(self):
        """[H, W, n_sizes, n_rots, 7]"""
        shape = (self.H, self.W, self.ns, self.nr)
        out = np.zeros(shape + (7,), F)
        out[..., 0] = self.xs.T[None, :, :, None]
        out[..., 1] = self.ys.T[:, None, :, None]
        out[..., 2] = self.zs[None, None, :, None]
        out[..., 3:6] = self.sizes[None, None, :, None, :]
        out[..., 6] = self.rots
        return out


def make_grid(gen_cfg, height, width):
    """the generator's tables with the reference's arithmetic (torch.linspace over size + 1 points, the half-cell shift, the
    first `size` entries) on the host"""
    aligned = gen_cfg['type'] == 'AlignedAnchor3DRangeGenerator'
    corner = gen_cfg.get('align_corner', False)

    def axis(lo, hi, n):
        if not aligned:
            return torch.linspace(lo, hi, n)
        c = torch.linspace(lo, hi, n + 1)
        if not corner:
            c += (c[1] - c[0]) / 2
        return c[:n]

    ranges, sizes = gen_cfg['ranges'], gen_cfg['sizes']
    if len(ranges) != len(sizes):
        ranges = ranges * len(sizes)
    xs, ys, zs = [], [], []
    for rng in ranges:
        r = torch.tensor(rng, dtype=torch.float32)
        xs.append(axis(r[0].item(), r[3].item(), width).numpy())
        ys.append(axis(r[1].item(), r[4].item(), height).numpy())
        zs.append(axis(r[2].item(), r[5].item(), 1).numpy()[0])
    return Grid(np.stack(xs), np.stack(ys), np.array(zs), torch.tensor(sizes, dtype=torch.float32).numpy(),
                torch.tensor(gen_cfg.get('rotations', [0, 1.5707963]), dtype=torch.float32).numpy())


# ------------------------------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------------------------------

def limit_period(val, offset, period):
    val = np.asarray(val, F)
    return (val - np.floor(val / F(period) + F(offset)) * F(period)).astype(F)


def nearest_dims(rz, w, l):
    """extents along x and y of nearest_bev: (w, l), swapped where |limit_period(rz, 0.5, pi)| > pi / 4"""
    swap = np.abs(limit_period(rz, 0.5, PI)) > F(PI / 4)
    return np.where(swap, l, w).astype(F), np.where(swap, w, l).astype(F)


def nearest_bev(boxes):
    b = np.asarray(boxes, F)
    b = b.reshape(-1, b.shape[-1] if b.ndim == 2 else 7)
    dx, dy = nearest_dims(b[:, 6], b[:, 3], b[:, 4])
    return np.stack([b[:, 0] - dx / F(2), b[:, 1] - dy / F(2), b[:, 0] + dx / F(2), b[:, 1] + dy / F(2)], 1).astype(F)


def assign(grid, boxes, labels, assigners, per_class):
    """one sample -> (assigned int32 [H, W, ns, nr]: box index, -1 background, -2 ignored; max_iou fp32 of the same shape;
    gt_max fp32 [ns, G])"""
    boxes = np.asarray(boxes, F)
    boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.ndim == 2 else 7)
    labels = np.asarray(labels, np.int64).reshape(-1)
    n = len(boxes)
    if isinstance(assigners, dict):
        assigners = [assigners] * grid.ns
    shape = (grid.H, grid.W, grid.ns, grid.nr)
    assigned = np.full(shape, -1, np.int32)
    max_iou = np.zeros(shape, F)
    argmax = np.zeros(shape, np.int32)
    gt_max = np.zeros((grid.ns, n), F)
    gb = nearest_bev(boxes) if n else np.zeros((0, 4), F)
    garea = ((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])).astype(F)
    blocks = {}
    for s in range(grid.ns):
        for r in range(grid.nr):
            dx, dy = nearest_dims(grid.rots[r], grid.sizes[s, 0], grid.sizes[s, 1])
            ax1, ax2 = grid.xs[s] - dx / F(2), grid.xs[s] + dx / F(2)
            ay1, ay2 = grid.ys[s] - dy / F(2), grid.ys[s] + dy / F(2)
            aarea = ((ax2 - ax1)[None, :] * (ay2 - ay1)[:, None]).astype(F)
            for g in range(n):
                if per_class and labels[g] != s:
                    continue
                iw = np.maximum(np.minimum(gb[g, 2], ax2) - np.maximum(gb[g, 0], ax1), F(0))
                ih = np.maximum(np.minimum(gb[g, 3], ay2) - np.maximum(gb[g, 1], ay1), F(0))
                ws, hs = np.nonzero(iw > 0)[0], np.nonzero(ih > 0)[0]
                if len(ws) == 0 or len(hs) == 0:
                    continue
                w0, w1, h0, h1 = ws[0], ws[-1] + 1, hs[0], hs[-1] + 1
                overlap = (ih[h0:h1, None] * iw[None, w0:w1]).astype(F)
                union = np.maximum(garea[g] + aarea[h0:h1, w0:w1] - overlap, F(1e-6))
                iou = (overlap / union).astype(F)
                blocks[(s, r, g)] = (h0, h1, w0, w1, iou)
                sub_max, sub_arg = max_iou[h0:h1, w0:w1, s, r], argmax[h0:h1, w0:w1, s, r]
                better = iou > sub_max
                sub_arg[better] = g
                sub_max[better] = iou[better]
                gt_max[s, g] = max(gt_max[s, g], iou.max())
        a = assigners[s]
        m = max_iou[:, :, s, :]
        code = np.where(m >= F(a['pos_iou_thr']), argmax[:, :, s, :], np.where(m < F(a['neg_iou_thr']), -1, -2)).astype(np.int32)
        assigned[:, :, s, :] = code
        for g in range(n):
            if gt_max[s, g] >= F(a['min_pos_iou']) and gt_max[s, g] > 0:
                for r in range(grid.nr):
                    if (s, r, g) in blocks:
                        h0, h1, w0, w1, iou = blocks[(s, r, g)]
                        assigned[h0:h1, w0:w1, s, r][iou == gt_max[s, g]] = g
    return assigned, max_iou, gt_max


def encode(anchors, gts, dtype=F):
    """DeltaXYZWLHRBBoxCoder.encode, one operation at a time in ``dtype``; log is torch's (the library the golden used)"""
    a, g = np.asarray(anchors, dtype), np.asarray(gts, dtype)
    two = dtype(2)
    za, zg = a[..., 2] + a[..., 5] / two, g[..., 2] + g[..., 5] / two
    diagonal = np.sqrt((a[..., 4] * a[..., 4] + a[..., 3] * a[..., 3]).astype(dtype)).astype(dtype)

    def log(v):
        return torch.log(torch.from_numpy(np.ascontiguousarray(v, dtype))).numpy()

    return np.stack([(g[..., 0] - a[..., 0]) / diagonal, (g[..., 1] - a[..., 1]) / diagonal, (zg - za) / a[..., 5],
                     log(g[..., 3] / a[..., 3]), log(g[..., 4] / a[..., 4]), log(g[..., 5] / a[..., 5]),
                     g[..., 6] - a[..., 6]], -1).astype(dtype)


def direction_target(anchors, reg_targets, dir_offset):
    rot_gt = (np.asarray(reg_targets, F)[..., 6] + np.asarray(anchors, F)[..., 6]).astype(F)
    offset_rot = limit_period(rot_gt - F(dir_offset), 0, 2 * PI)
    return np.clip(np.floor(offset_rot / F(PI)).astype(np.int64), 0, 1), offset_rot


def dense_targets(grid, assigned, boxes, labels, num_classes, pos_weight, dir_offset, dtype=F):
    """one sample's flat (h, w, size, rot) targets as anchor_target_3d_single returns them -> dict"""
    assigned = assigned.reshape(-1)
    anchors = grid.anchors().reshape(-1, 7)
    pos = assigned >= 0
    n = len(assigned)
    out = dict(labels=np.full(n, num_classes, np.int64), label_weights=np.where(assigned == -2, 0, 1).astype(F),
               bbox_targets=np.zeros((n, 7), dtype), bbox_weights=np.zeros((n, 7), F), dir_targets=np.zeros(n, np.int64),
               dir_weights=pos.astype(F), num_pos=int(pos.sum()), num_neg=int((assigned == -1).sum()))
    if pos.any():
        gts = np.asarray(boxes, F)[assigned[pos], :7]
        out['labels'][pos] = np.asarray(labels, np.int64)[assigned[pos]]
        out['label_weights'][pos] = F(1.0 if pos_weight <= 0 else pos_weight)
        out['bbox_targets'][pos] = encode(anchors[pos], gts, dtype)
        out['bbox_weights'][pos] = 1
        out['dir_targets'][pos] = direction_target(anchors[pos], encode(anchors[pos], gts), dir_offset)[0]
    return out


def batch_targets(grid, boxes_list, labels_list, cfg, dtype=F):
    """-> (dict of batch-stacked dense targets, per-sample (assigned, max_iou, gt_max), num_total_pos, num_total_neg)"""
    per_sample, dense = [], []
    tc = cfg['train_cfg']
    for b, l in zip(boxes_list, labels_list):
        res = assign(grid, b, l, tc['assigner'], cfg['assign_per_class'])
        per_sample.append(res)
        dense.append(dense_targets(grid, res[0], b, l, cfg['num_classes'], tc.get('pos_weight', -1), cfg['dir_offset'], dtype))
    stacked = {k: np.stack([d[k] for d in dense]) for k in dense[0] if not k.startswith('num_')}
    return (stacked, per_sample, sum(max(d['num_pos'], 1) for d in dense), sum(max(d['num_neg'], 1) for d in dense))


# ------------------------------------------------------------------------------------------------------------------
# losses (torch, any dtype, differentiable)
# ------------------------------------------------------------------------------------------------------------------

def py_sigmoid_focal_loss(pred, target, weight, gamma, alpha, avg_factor):
    """mmdet 2.x py_sigmoid_focal_loss with reduction 'mean' and avg_factor"""
    pred_sigmoid = pred.sigmoid()
    target = target.type_as(pred)
    pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    loss = F_.binary_cross_entropy_with_logits(pred, target, reduction='none') * focal_weight
    return (loss * weight.reshape(-1, 1)).sum() / avg_factor


def box_loss(pred, target, weight, avg_factor, beta=None):
    diff = (pred - target).abs()
    if beta is not None:
        diff = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    return (diff * weight).sum() / avg_factor


def losses(cls_score, bbox_pred, dir_pred, tg, avg_factor, cfg):
    """Anchor3DHead.loss_single on the dense targets ``tg`` (numpy) -> (loss_cls, loss_bbox, loss_dir) in the maps' dtype"""
    dt, c = cls_score.dtype, cfg['num_classes']
    labels = torch.from_numpy(tg['labels']).reshape(-1)
    cls = cls_score.permute(0, 2, 3, 1).reshape(-1, c)
    lc = cfg['loss_cls']
    loss_cls = lc.get('loss_weight', 1.0) * py_sigmoid_focal_loss(
        cls, F_.one_hot(labels, c + 1)[:, :c], torch.from_numpy(tg['label_weights']).to(dt).reshape(-1), lc.get('gamma', 2.0),
        lc.get('alpha', 0.25), avg_factor)
    pos = (labels >= 0) & (labels < c)
    box = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 7)[pos]
    tgt = torch.from_numpy(tg['bbox_targets']).to(dt).reshape(-1, 7)[pos]
    wgt = torch.from_numpy(tg['bbox_weights']).to(dt).reshape(-1, 7)[pos]
    if pos.sum() == 0:
        return loss_cls, box.sum(), (None if dir_pred is None else dir_pred.permute(0, 2, 3, 1).reshape(-1, 2)[pos].sum())
    code_weight = cfg['train_cfg'].get('code_weight', None)
    if code_weight:
        wgt = wgt * wgt.new_tensor(code_weight)
    if cfg['diff_rad_by_sin']:
        p6 = torch.sin(box[..., 6:7]) * torch.cos(tgt[..., 6:7])
        t6 = torch.cos(box[..., 6:7]) * torch.sin(tgt[..., 6:7])
        box, tgt = torch.cat([box[..., :6], p6], -1), torch.cat([tgt[..., :6], t6], -1)
    lb = cfg['loss_bbox']
    loss_bbox = lb.get('loss_weight', 1.0) * box_loss(box, tgt, wgt, avg_factor, lb.get('beta', 1.0) if lb['type'] == 'SmoothL1Loss'
                                                      else None)
    loss_dir = None
    if dir_pred is not None:
        d = dir_pred.permute(0, 2, 3, 1).reshape(-1, 2)[pos]
        ce = F_.cross_entropy(d, torch.from_numpy(tg['dir_targets']).reshape(-1)[pos], reduction='none')
        loss_dir = cfg['loss_dir'].get('loss_weight', 1.0) * (ce * torch.from_numpy(tg['dir_weights']).to(dt).reshape(-1)[pos]).sum() \
            / avg_factor
    return loss_cls, loss_bbox, loss_dir


def loss_and_grads(cls_score, bbox_pred, dir_pred, tg, avg_factor, cfg, dtype=torch.float64):
    """float32 numpy maps -> dict of the three losses and of the gradients of their sum, computed in ``dtype``"""
    maps = [torch.from_numpy(np.ascontiguousarray(m)).to(dtype).requires_grad_(True) for m in (cls_score, bbox_pred, dir_pred)
            if m is not None]
    tg = dict(tg, bbox_targets=tg['bbox_targets'].astype(np.float64 if dtype == torch.float64 else F))
    out = losses(maps[0], maps[1], maps[2] if len(maps) > 2 else None, tg, avg_factor, cfg)
    total = sum(o for o in out if o is not None)
    total.backward()
    res = dict(loss_cls=out[0].item(), loss_bbox=out[1].item(), loss_dir=0.0 if out[2] is None else out[2].item())
    for k, m in zip(('d_cls', 'd_bbox', 'd_dir'), maps):
        res[k] = (torch.zeros_like(m) if m.grad is None else m.grad).numpy()
    return res


# ------------------------------------------------------------------------------------------------------------------
# decoding
# ------------------------------------------------------------------------------------------------------------------

def decode(anchors, deltas):
    """DeltaXYZWLHRBBoxCoder.decode in float32, one operation at a time; exp is torch's"""
    a, d = np.asarray(anchors, F), np.asarray(deltas, F)
    za = a[:, 2] + a[:, 5] / F(2)
    diagonal = np.sqrt((a[:, 4] * a[:, 4] + a[:, 3] * a[:, 3]).astype(F)).astype(F)
    ex = torch.exp(torch.from_numpy(np.ascontiguousarray(d[:, 3:6]))).numpy()
    xg, yg, zg = d[:, 0] * diagonal + a[:, 0], d[:, 1] * diagonal + a[:, 1], d[:, 2] * a[:, 5] + za
    wg, lg, hg = ex[:, 0] * a[:, 3], ex[:, 1] * a[:, 4], ex[:, 2] * a[:, 5]
    return np.stack([xg, yg, zg - hg / F(2), wg, lg, hg, d[:, 6] + a[:, 6]], 1).astype(F)


def candidates(grid, cls_score, bbox_pred, dir_pred, num_classes, nms_pre):
    """one sample's maps [C', H, W] -> (inds, boxes [n, 7], scores [n, C + 1], dir int64 [n], bev xyxyr [n, 5]) before the NMS"""
    cls = torch.from_numpy(np.ascontiguousarray(cls_score)).permute(1, 2, 0).reshape(-1, num_classes)
    scores = cls.sigmoid()
    box = np.ascontiguousarray(bbox_pred).transpose(1, 2, 0).reshape(-1, 7)
    dirs = np.ascontiguousarray(dir_pred).transpose(1, 2, 0).reshape(-1, 2)
    dir_score = torch.max(torch.from_numpy(dirs), dim=-1)[1].numpy()
    anchors = grid.anchors().reshape(-1, 7)
    inds = np.arange(len(anchors))
    if nms_pre > 0 and scores.shape[0] > nms_pre:
        inds = scores.max(dim=1)[0].topk(nms_pre)[1].numpy()
    boxes = decode(anchors[inds], box[inds])
    sc = np.concatenate([scores.numpy()[inds], np.zeros((len(inds), 1), F)], 1)
    hw, hl = boxes[:, 3] / F(2), boxes[:, 4] / F(2)
    bev = np.stack([boxes[:, 0] - hw, boxes[:, 1] - hl, boxes[:, 0] + hw, boxes[:, 1] + hl, boxes[:, 6]], 1).astype(F)
    return inds, boxes, sc, dir_score[inds], bev


def get_bboxes_single(grid, cls_score, bbox_pred, dir_pred, cfg):
    """get_bboxes_single -> (boxes [n, 7], scores [n], labels int64 [n]); the NMS is tests/box_ops_ref.nms_host"""
    tc = cfg['test_cfg']
    _, boxes, scores, dirs, bev = candidates(grid, cls_score, bbox_pred, dir_pred, cfg['num_classes'], tc.get('nms_pre', -1))
    res = B.multiclass_nms_host(boxes, bev, scores, tc.get('score_thr', 0), tc['max_num'], tc['nms_thr'], tc['use_rotate_nms'],
                                dir_scores=dirs)
    if res is None:
        return np.zeros((0, 7), F), np.zeros(0, F), np.zeros(0, np.int64)
    out = res['bboxes'].copy()
    dir_rot = limit_period(out[:, 6] - F(cfg['dir_offset']), cfg['dir_limit_offset'], PI)
    out[:, 6] = dir_rot + F(cfg['dir_offset']) + F(PI) * res['dir'].astype(F)
    return out, res['scores'], res['labels']
