"""Times the training and decoding side of Anchor3DHead (csrc/anchor_head.hip) at the shipped size - 468 x 468 map, 3 sizes x 2
rotations, 3 classes, 2 samples of about 100 boxes - with device events after warm-up (the median of --iters separately timed
calls, the middle one of three alternating rounds), next to the same data flow composed from torch ops on the same device, which
is the reference's algorithm (train_mixins.py:101-314, anchor3d_head.py:197-551): the [A, 7] anchor tensor, per sample and size
a dense [G, H * W * n_rot] nearest-BEV IoU matrix, the Python loop of gt_max_assign_all over the boxes, dense labels / weights /
box targets / direction targets, nonzero and len(pos_inds) in loss_single, permuted copies of the three maps; for decoding the
permuted maps, sigmoid, max, topk, the gathers and the coder.  Prints one JSON object.

    python tools/anchor_head_bench.py [--iters 20] [--out profiles/anchor_head/anchor_head_bench.json]

Per fused call: milliseconds (a call time by device events, not a kernel time: launch gaps are inside), the bytes the call has to
move computed from the shapes (maps read or written once, 4 B per anchor of targets) and those bytes over the time as a fraction
of the 8 TB/s HBM roof of the MI355X.  Host synchronisations are counted in the composed code (every bool() / int() / .item() /
nonzero of a device value); the fused training path has none.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_common import median_ms  # noqa: E402
import sst_amd  # noqa: E402
from sst_amd.anchor_head import limit_period  # noqa: E402

DEV = 'cuda:0'
HBM_BYTES_PER_S = 8.0e12
SYNCS = [0]
H = W = 468
GEN = dict(type='AlignedAnchor3DRangeGenerator',
           ranges=[[-74.88, -74.88, -0.0345, 74.88, 74.88, -0.0345], [-74.88, -74.88, -0.1188, 74.88, 74.88, -0.1188],
                   [-74.88, -74.88, 0, 74.88, 74.88, 0]],
           sizes=[[2.08, 4.73, 1.77], [0.84, 1.81, 1.77], [0.84, 0.91, 1.74]], rotations=[0, 1.57], reshape_out=False)
ASSIGN = [dict(type='MaxIoUAssigner', iou_calculator=dict(type='BboxOverlapsNearest3D'), pos_iou_thr=p, neg_iou_thr=n,
               min_pos_iou=n, ignore_iof_thr=-1) for p, n in ((0.55, 0.4), (0.5, 0.3), (0.5, 0.3))]
HEAD = dict(type='Anchor3DHead', num_classes=3, in_channels=384, feat_channels=384, use_direction_classifier=True,
            anchor_generator=GEN, diff_rad_by_sin=True, dir_offset=0.7854, dir_limit_offset=0,
            bbox_coder=dict(type='DeltaXYZWLHRBBoxCoder', code_size=7),
            loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
            loss_bbox=dict(type='L1Loss', loss_weight=0.5),
            loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.2),
            train_cfg=dict(assigner=ASSIGN, allowed_border=0, code_weight=[1.0] * 7, pos_weight=-1, debug=False),
            test_cfg=dict(use_rotate_nms=True, nms_across_levels=False, nms_pre=4096, nms_thr=0.25, score_thr=0.1, min_bbox_size=0,
                          max_num=500))
C, N_A = 3, 6


def host(x):
    """a device value the host branches on"""
    SYNCS[0] += 1
    return x.item()


def nearest_bev(boxes):
    bev = boxes[:, [0, 1, 3, 4, 6]]
    normed = torch.abs(limit_period(bev[:, -1], 0.5, np.pi))
    xywh = torch.where((normed > np.pi / 4)[..., None], bev[:, [0, 1, 3, 2]], bev[:, :4])
    return torch.cat([xywh[:, :2] - xywh[:, 2:] / 2, xywh[:, :2] + xywh[:, 2:] / 2], dim=-1)


def bbox_overlaps(b1, b2):
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = (torch.min(b1[:, None, 2:], b2[None, :, 2:]) - torch.max(b1[:, None, :2], b2[None, :, :2])).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    return overlap / torch.max(area1[:, None] + area2[None, :] - overlap, overlap.new_tensor([1e-6]))


def encode(a, g):
    za, zg = a[:, 2] + a[:, 5] / 2, g[:, 2] + g[:, 5] / 2
    diagonal = torch.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    return torch.stack([(g[:, 0] - a[:, 0]) / diagonal, (g[:, 1] - a[:, 1]) / diagonal, (zg - za) / a[:, 5],
                        torch.log(g[:, 3] / a[:, 3]), torch.log(g[:, 4] / a[:, 4]), torch.log(g[:, 5] / a[:, 5]),
                        g[:, 6] - a[:, 6]], -1)


def composed_targets(anchors, boxes_list, labels_list):
    """anchor_target_3d: per sample, per size one assigner over a dense IoU matrix -> the six dense tensors and num_total_pos"""
    feat = H * W
    outs, total_pos = [[] for _ in range(6)], 0
    for boxes, gt_labels in zip(boxes_list, labels_list):
        per = [[] for _ in range(6)]
        n_pos = 0
        for i, cfg in enumerate(ASSIGN):
            cur = anchors[..., i, :, :].reshape(-1, 7)
            n = cur.size(0)
            overlaps = bbox_overlaps(nearest_bev(boxes), nearest_bev(cur))
            assigned = overlaps.new_full((n,), -1, dtype=torch.long)
            max_overlaps, argmax = overlaps.max(dim=0)
            gt_max, _ = overlaps.max(dim=1)
            assigned[(max_overlaps >= 0) & (max_overlaps < cfg['neg_iou_thr'])] = 0
            pos = max_overlaps >= cfg['pos_iou_thr']
            assigned[pos] = argmax[pos] + 1
            for g in range(boxes.size(0)):
                if host(gt_max[g] >= cfg['min_pos_iou']):
                    assigned[overlaps[g, :] == gt_max[g]] = g + 1
            SYNCS[0] += 2
            pos_inds = torch.nonzero(assigned > 0, as_tuple=False).squeeze(-1).unique()
            neg_inds = torch.nonzero(assigned == 0, as_tuple=False).squeeze(-1).unique()
            labels = gt_labels.new_full((n,), C)
            label_weights = cur.new_zeros(n)
            bbox_targets, bbox_weights = torch.zeros_like(cur), torch.zeros_like(cur)
            dir_targets, dir_weights = gt_labels.new_zeros(n), cur.new_zeros(n)
            if len(pos_inds) > 0:
                gt_of = assigned[pos_inds] - 1
                t = encode(cur[pos_inds], boxes[gt_of])
                off = limit_period(t[:, 6] + cur[pos_inds, 6] - HEAD['dir_offset'], 0, 2 * np.pi)
                bbox_targets[pos_inds] = t
                bbox_weights[pos_inds] = 1.0
                dir_targets[pos_inds] = torch.clamp(torch.floor(off / np.pi).long(), min=0, max=1)
                dir_weights[pos_inds] = 1.0
                labels[pos_inds] = gt_labels[gt_of]
                label_weights[pos_inds] = 1.0
            label_weights[neg_inds] = 1.0
            n_pos += len(pos_inds)
            for lst, t, tail in zip(per, (labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights),
                                    ((), (), (7,), (7,), (), ())):
                lst.append(t.reshape(feat, 1, 2, *tail))
        for lst, parts, tail in zip(outs, per, ((), (), (7,), (7,), (), ())):
            lst.append(torch.cat(parts, dim=1).reshape(-1, *tail))
        total_pos += max(n_pos, 1)
    return [torch.stack(lst) for lst in outs], total_pos


def composed_loss(cls_score, bbox_pred, dir_pred, tg, num_total):
    labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights = tg
    labels = labels.reshape(-1)
    cls = cls_score.permute(0, 2, 3, 1).reshape(-1, C)
    host(labels.max())
    target = F.one_hot(labels, C + 1)[:, :C].type_as(cls)
    p = cls.sigmoid()
    pt = (1 - p) * target + p * (1 - target)
    focal = (0.25 * target + 0.75 * (1 - target)) * pt.pow(2.0)
    loss_cls = (F.binary_cross_entropy_with_logits(cls, target, reduction='none') * focal
                * label_weights.reshape(-1, 1)).sum() / num_total
    box = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 7)
    SYNCS[0] += 1
    pos_inds = ((labels >= 0) & (labels < C)).nonzero(as_tuple=False).reshape(-1)
    pb, pt_, pw = box[pos_inds], bbox_targets.reshape(-1, 7)[pos_inds], bbox_weights.reshape(-1, 7)[pos_inds]
    dirs = dir_pred.permute(0, 2, 3, 1).reshape(-1, 2)[pos_inds]
    sin_p = torch.sin(pb[:, 6:7]) * torch.cos(pt_[:, 6:7])
    sin_t = torch.cos(pb[:, 6:7]) * torch.sin(pt_[:, 6:7])
    pb, pt_ = torch.cat([pb[:, :6], sin_p], -1), torch.cat([pt_[:, :6], sin_t], -1)
    loss_bbox = 0.5 * ((pb - pt_).abs() * pw).sum() / num_total
    loss_dir = 0.2 * (F.cross_entropy(dirs, dir_targets.reshape(-1)[pos_inds], reduction='none')
                      * dir_weights.reshape(-1)[pos_inds]).sum() / num_total
    return loss_cls, loss_bbox, loss_dir


def composed_decode(anchors, cls_score, bbox_pred, dir_pred, nms_pre):
    """get_bboxes_single up to the NMS, one sample"""
    flat = anchors.reshape(-1, 7)
    dir_score = torch.max(dir_pred.permute(1, 2, 0).reshape(-1, 2), dim=-1)[1]
    scores = cls_score.permute(1, 2, 0).reshape(-1, C).sigmoid()
    box = bbox_pred.permute(1, 2, 0).reshape(-1, 7)
    _, top = scores.max(dim=1)[0].topk(nms_pre)
    a, d, scores, dir_score = flat[top], box[top], scores[top], dir_score[top]
    za = a[:, 2] + a[:, 5] / 2
    diagonal = torch.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    hg = torch.exp(d[:, 5]) * a[:, 5]
    boxes = torch.stack([d[:, 0] * diagonal + a[:, 0], d[:, 1] * diagonal + a[:, 1], d[:, 2] * a[:, 5] + za - hg / 2,
                         torch.exp(d[:, 3]) * a[:, 3], torch.exp(d[:, 4]) * a[:, 4], hg, d[:, 6] + a[:, 6]], -1)
    bev = sst_amd.box_ops.xywhr2xyxyr(boxes[:, [0, 1, 3, 4, 6]])
    return boxes, torch.cat([scores, scores.new_zeros(scores.shape[0], 1)], 1), dir_score, bev


def scene(n_boxes, seed):
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    for _ in range(2):
        kind = torch.randint(0, 3, (n_boxes,), generator=g)
        b = torch.zeros(n_boxes, 7)
        b[:, :2] = (torch.rand(n_boxes, 2, generator=g) - 0.5) * 146
        b[:, 3:6] = torch.tensor(GEN['sizes'])[kind] * (0.8 + 0.45 * torch.rand(n_boxes, 3, generator=g))
        b[:, 2] = -1.5 + torch.rand(n_boxes, generator=g)
        b[:, 6] = torch.tensor([0.0, 1.5708, 3.1416, -1.5708])[torch.randint(0, 4, (n_boxes,), generator=g)] \
            + 0.3 * torch.randn(n_boxes, generator=g)
        boxes.append(b.to(DEV))
        labels.append(kind.to(DEV))
    return boxes, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--boxes', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    head = sst_amd.build_head(HEAD).to(DEV)
    g = torch.Generator().manual_seed(1)
    maps = [(torch.randn(2, N_A * c, H, W, generator=g) * s + m).to(DEV).requires_grad_(True)
            for c, s, m in ((C, 1.5, -3.0), (7, 0.3, 0.0), (2, 1.0, 0.0))]
    boxes, labels = scene(args.boxes, seed=args.boxes)
    anchors = head.anchor_generator.grid_anchors([(H, W)], device=DEV)[0]
    grid = head.anchor_generator.grid((H, W), DEV)

    def backward(losses):
        for t in maps:
            t.grad = None
        (losses[0] + losses[1] + losses[2]).backward()

    def fused_targets():
        return head.targets(boxes, labels, (H, W))

    def fused_loss_fwd(t):
        return sst_amd.anchor_loss(maps[0], maps[1], maps[2], t, C, loss_weight_bbox=0.5, loss_weight_dir=0.2,
                                   code_weight=[1.0] * 7, dir_offset=0.7854)

    def fused():
        out = fused_loss_fwd(fused_targets())
        backward(out)
        return out

    def composed():
        tg, n = composed_targets(anchors, boxes, labels)
        out = composed_loss(*maps, tg, n)
        backward(out)
        return out

    inds = maps[0][0].detach().sigmoid().view(N_A, C, -1).amax(1).t().reshape(-1).topk(4096)[1].contiguous()
    det = [m[0].detach().contiguous() for m in maps]

    def fused_decode():
        return sst_amd.anchor_decode(det[0], det[1], det[2], grid, C, inds)

    def fused_select_decode():
        top = det[0].sigmoid().view(N_A, C, -1).amax(1).t().reshape(-1).topk(4096)[1].contiguous()
        return sst_amd.anchor_decode(det[0], det[1], det[2], grid, C, top)

    a, b = fused(), composed()
    gap = {k: abs(float(x) - float(y)) / abs(float(y)) for k, x, y in zip(('loss_cls', 'loss_bbox', 'loss_dir'), a, b)}
    t_f = fused_targets()
    tg_c, n_c = composed_targets(anchors, boxes, labels)
    same = bool(torch.equal(torch.where(t_f.assigned >= 0, 1, 0).long(), (tg_c[0] < C).long()))
    dec_gap = float((fused_select_decode()[0] - composed_decode(anchors, *det, 4096)[0]).abs().max())
    out_f = fused_loss_fwd(t_f)
    rounds = {k: [] for k in ('fused', 'composed', 'fused_targets', 'composed_targets', 'fused_loss_fwd', 'fused_loss_bwd',
                              'composed_loss', 'fused_decode', 'fused_select_decode', 'composed_decode')}
    for _ in range(3):                       # alternate the paths: other work shares the machine
        rounds['fused'].append(median_ms(fused, args.iters))
        rounds['composed'].append(median_ms(composed, max(args.iters // 4, 3), warmup=1))
        rounds['fused_targets'].append(median_ms(fused_targets, args.iters))
        rounds['composed_targets'].append(median_ms(lambda: composed_targets(anchors, boxes, labels), max(args.iters // 4, 3), warmup=1))
        rounds['fused_loss_fwd'].append(median_ms(lambda: fused_loss_fwd(t_f), args.iters))
        rounds['fused_loss_bwd'].append(median_ms(
            lambda: torch.autograd.grad(out_f[0] + out_f[1] + out_f[2], maps, retain_graph=True), args.iters))
        rounds['composed_loss'].append(median_ms(lambda: backward(composed_loss(*maps, tg_c, n_c)), args.iters))
        rounds['fused_decode'].append(median_ms(fused_decode, args.iters))
        rounds['fused_select_decode'].append(median_ms(fused_select_decode, args.iters))
        rounds['composed_decode'].append(median_ms(lambda: composed_decode(anchors, *det, 4096), args.iters))
    SYNCS[0] = 0
    composed()
    syncs = SYNCS[0]
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, samples=2, boxes_per_sample=args.boxes, map=[H, W],
               anchors_per_sample=H * W * N_A, classes=C,
               statistic='median of device-event call times, the middle one of three alternating rounds',
               positives=int((t_f.assigned >= 0).sum()), positive_sets_equal=same, relative_gap_fused_vs_composed=gap,
               decode_max_abs_gap=dec_gap, composed_host_syncs=syncs, fused_host_syncs=0)
    for k, v in rounds.items():
        res[k + '_ms'] = round(sorted(m for m, _ in v)[1], 4)
        res[k + '_min_ms'] = round(min(m for _, m in v), 4)
    res['composed_over_fused'] = round(res['composed_ms'] / res['fused_ms'], 2)
    res['composed_over_fused_decode'] = round(res['composed_decode_ms'] / res['fused_select_decode_ms'], 2)
    # what each fused call has to move: maps read or written once, 4 B per anchor of targets, the boxes
    cells, n_anchor = 2 * H * W, 2 * H * W * N_A
    per_map = dict(cls=cells * N_A * C * 4, box=cells * N_A * 7 * 4, dir=cells * N_A * 2 * 4)
    nbytes = dict(fused_targets=3 * n_anchor * 4,                                    # written, then read and rewritten
                  fused_loss_fwd=per_map['cls'] + n_anchor * 4,                      # box / dir maps only at the positives
                  fused_loss_bwd=per_map['cls'] + n_anchor * 4 + sum(per_map.values()),
                  fused_decode=4096 * (C + 7 + 2) * 64 + 4096 * (7 + C + 1 + 2 + 5) * 4)     # a 64 B sector per gathered value
    res['maps_bytes_per_sample'] = sum(per_map.values()) // 2
    res['algorithmic_bytes'] = nbytes
    res['fraction_of_hbm_roof'] = {k: round(v / (res[k + '_ms'] * 1e-3) / HBM_BYTES_PER_S, 4) for k, v in nbytes.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
