"""Times the RoI head's step around its network (csrc/roi_head.hip) - assignment, sampling, targets, loss forward, loss backward -
with device events after warm-up (the median of --iters separately timed steps, three alternating rounds), against the same step
composed from torch ops on the same device in the reference's data flow (roi_heads/fsd_roi_head.py:213-296,
bbox_heads/fsd_bbox_head.py:207-579, samplers/iou_neg_piecewise_sampler.py, mmdet's MaxIoUAssigner): per sample and class two
boolean-mask compactions, an IoU matrix launch, the assigner's Python loop over the boxes, ``nonzero`` / ``randperm`` / ``unique``
in the sampler; per sample the canonical transform and the encode; in the loss ``.item()`` reads, the per-sample re-compaction and
the corner loss as small torch ops that autograd replays.  The composed path's IoU is this library's
``box_ops.boxes3d_overlaps_lidar``.  Prints one JSON object.

    python tools/roi_head_bench.py [--iters 30] [--out profiles/roi_head/roi_head_bench.json] [--no-profiler]

Sizes: 2 samples x 300 and x 1 500 proposals, 60 boxes each, num = 256, three classes with the shipped thresholds.  Per path:
milliseconds of the whole step and of its assignment and loss parts, kernel launches (counted by torch.profiler in a separate,
untimed step; null when the profiler is not available) and host reads (counted in the composed code: every bool() / int() /
.item() of a device value, every boolean-mask index, nonzero and unique; the fused path has the one read of ``counts``).
"""
import argparse
import functools
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _bench_common  # noqa: E402
from _bench_common import median_ms  # noqa: E402
import sst_amd  # noqa: E402
from sst_amd import box_ops  # noqa: E402

DEV = 'cuda:0'
SYNCS = [0]
CFG = dict(num_classes=3, class_mask=True, pos_iou_thr=[0.45, 0.35, 0.35], neg_iou_thr=[0.45, 0.35, 0.35],
           min_pos_iou=[0.45, 0.35, 0.35], num=256, pos_fraction=0.55, neg_piece_fractions=[0.8, 0.2],
           neg_iou_piece_thrs=[0.55, 0.1], cls_pos_thr=(0.8, 0.65, 0.65), cls_neg_thr=(0.2, 0.15, 0.15))
WEIGHTS = (1.0, 2.0, 1.0)
TWO_PI = 2 * math.pi

count_launches = functools.partial(_bench_common.count_launches, ours='roi_')  # kernels of csrc/roi_head.hip


def read(n=1):
    SYNCS[0] += n


def masked(t, mask):
    read()
    return t[mask]


def nonzero(mask):
    read()
    return torch.nonzero(mask, as_tuple=False).view(-1)


def assign_class(boxes, gts, labels, c):
    """MaxIoUAssigner.assign of one class -> (gt_inds, max_overlaps, labels)"""
    n, m = boxes.size(0), gts.size(0)
    gt_inds = boxes.new_full((n,), -1, dtype=torch.long)
    if n == 0 or m == 0:
        if m == 0:
            gt_inds[:] = 0
        return gt_inds, boxes.new_zeros(n), gt_inds.new_full((n,), -1)
    overlaps = box_ops.boxes3d_overlaps_lidar(gts, boxes)
    max_overlaps, argmax = overlaps.max(dim=0)
    gt_max, _ = overlaps.max(dim=1)
    gt_inds[(max_overlaps >= 0) & (max_overlaps < CFG['neg_iou_thr'][c])] = 0
    pos = max_overlaps >= CFG['pos_iou_thr'][c]
    gt_inds[pos] = argmax[pos] + 1
    for i in range(m):                                           # the assigner's loop over ground-truth boxes
        read()
        if gt_max[i] >= CFG['min_pos_iou'][c]:
            gt_inds[overlaps[i, :] == gt_max[i]] = i + 1
    out_labels = gt_inds.new_full((n,), -1)
    pos_inds = nonzero(gt_inds > 0)
    if pos_inds.numel() > 0:
        out_labels[pos_inds] = labels[gt_inds[pos_inds] - 1]
    return gt_inds, max_overlaps, out_labels


def random_choice(gallery, num):
    return gallery[torch.randperm(gallery.numel(), device=gallery.device)[:num]]


def sample(gt_inds, max_overlaps):
    num = CFG['num']
    pos_inds = nonzero(gt_inds > 0)
    expected_pos = int(num * CFG['pos_fraction'])
    if pos_inds.numel() > expected_pos:
        pos_inds = random_choice(pos_inds, expected_pos)
    pos_inds = pos_inds.unique()
    read()
    expected = num - pos_inds.numel()
    neg_inds = nonzero(gt_inds == 0)
    if len(neg_inds) > expected:
        chosen, extend = neg_inds.new_zeros([0]), 0
        ov = max_overlaps[neg_inds]
        pieces = CFG['neg_iou_piece_thrs']
        for q in range(len(pieces)):
            last = q == len(pieces) - 1
            want = expected - len(chosen) if last else int(expected * CFG['neg_piece_fractions'][q]) + extend
            lo = 0 if last else pieces[q + 1]
            piece = nonzero((ov >= lo) & (ov < pieces[q]))
            if len(piece) < want:
                chosen = torch.cat([chosen, neg_inds[piece]], dim=0)
                extend += want - len(piece)
            else:
                chosen = torch.cat([chosen, neg_inds[random_choice(piece, want)]], dim=0)
                extend = 0
        neg_inds = chosen
    neg_inds = neg_inds.unique()
    read()
    return pos_inds, neg_inds


def rotate_z(xyz, angle):
    c, s = torch.cos(angle), torch.sin(angle)
    return torch.stack([xyz[:, 0] * c + xyz[:, 1] * s, -xyz[:, 0] * s + xyz[:, 1] * c, xyz[:, 2]], 1)


def encode(anchor, box):
    diag = torch.sqrt(anchor[:, 4] ** 2 + anchor[:, 3] ** 2)
    return torch.stack([(box[:, 0] - anchor[:, 0]) / diag, (box[:, 1] - anchor[:, 1]) / diag,
                        ((box[:, 2] + box[:, 5] / 2) - (anchor[:, 2] + anchor[:, 5] / 2)) / anchor[:, 5],
                        torch.log(box[:, 3] / anchor[:, 3]), torch.log(box[:, 4] / anchor[:, 4]), torch.log(box[:, 5] / anchor[:, 5]),
                        box[:, 6] - anchor[:, 6]], 1)


def decode(anchor, d):
    diag = torch.sqrt(anchor[:, 4] ** 2 + anchor[:, 3] ** 2)
    hg = torch.exp(d[:, 5]) * anchor[:, 5]
    return torch.stack([d[:, 0] * diag + anchor[:, 0], d[:, 1] * diag + anchor[:, 1],
                        d[:, 2] * anchor[:, 5] + anchor[:, 2] + anchor[:, 5] / 2 - hg / 2, torch.exp(d[:, 3]) * anchor[:, 3],
                        torch.exp(d[:, 4]) * anchor[:, 4], hg, d[:, 6] + anchor[:, 6]], 1)


def target_single(pos_bboxes, pos_gt, ious, pos_labels):
    """_get_target_single -> (soft label, targets of the positives, reg_mask)"""
    n = ious.size(0)
    all_labels = torch.cat([pos_labels, pos_labels.new_full((n - pos_labels.size(0),), -1)])
    label = ious.new_zeros(n)
    for c in range(3):
        m = all_labels == c
        this = masked(ious, m)
        pos, neg = this > CFG['cls_pos_thr'][c], this < CFG['cls_neg_thr'][c]
        soft = pos.float()
        mid = ~pos & ~neg
        soft[mid] = (this[mid] - CFG['cls_neg_thr'][c]) / (CFG['cls_pos_thr'][c] - CFG['cls_neg_thr'][c])
        read()
        label[m] = soft
    read()
    assert bool((label >= 0).all())
    reg_mask = ious.new_zeros(n, dtype=torch.long)
    reg_mask[:pos_gt.size(0)] = 1
    read()
    if not bool(reg_mask.bool().any()):
        return label, pos_gt.new_empty((0, 7)), reg_mask
    ct = pos_gt.clone()
    roi_ry = pos_bboxes[:, 6] % TWO_PI
    ct[:, 0:3] -= pos_bboxes[:, 0:3]
    ct[:, 6] -= roi_ry
    ct[:, 0:3] = rotate_z(ct[:, 0:3], -(roi_ry + math.pi / 2))
    ry = ct[:, 6] % TWO_PI
    opposite = (ry > math.pi * 0.5) & (ry < math.pi * 1.5)
    ry[opposite] = (ry[opposite] + math.pi) % TWO_PI
    read()
    flag = ry > math.pi
    ry[flag] = ry[flag] - TWO_PI
    read()
    ct[:, 6] = torch.clamp(ry, min=-math.pi / 2, max=math.pi / 2)
    anchor = pos_bboxes.clone()
    anchor[:, 0:3] = 0
    anchor[:, 6] = 0
    return label, encode(anchor, ct), reg_mask


def corners(boxes):
    norm = torch.tensor([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]],
                        dtype=boxes.dtype).to(boxes.device) - boxes.new_tensor([0.5, 0.5, 0])
    local = boxes[:, None, 3:6] * norm[None]
    c, s = torch.cos(boxes[:, 6])[:, None], torch.sin(boxes[:, 6])[:, None]
    return torch.stack([local[..., 0] * c + local[..., 1] * s, -local[..., 0] * s + local[..., 1] * c, local[..., 2]], -1) \
        + boxes[:, None, 0:3]


def composed_assign(props, plabels, gts, glabels):
    """_assign_and_sample + get_targets -> per sample (rois, soft label, targets, reg_mask, positive boxes, positive labels)"""
    out = []
    for s in range(len(props)):
        boxes, pl, g, gl = props[s], plabels[s], gts[s], glabels[s]
        n = boxes.size(0)
        gt_inds, max_ov, lab = pl.new_zeros(n), boxes.new_zeros(n), pl.new_full((n,), -1)
        for c in range(3):
            gm, pm = gl == c, pl == c
            inds, ov, labels = assign_class(masked(boxes[:, :7], pm), masked(g[:, :7], gm), masked(gl, gm), c)
            pad = torch.nn.functional.pad(nonzero(gm) + 1, (2, 0))
            pad[0] = -1
            read(3)
            gt_inds[pm], max_ov[pm], lab[pm] = pad[inds + 1], ov, labels
        pos_inds, neg_inds = sample(gt_inds, max_ov)
        pos_gt = g[gt_inds[pos_inds] - 1] if g.numel() else g.view(-1, g.size(-1))
        ious = max_ov[torch.cat([pos_inds, neg_inds])]
        label, targets, reg_mask = target_single(boxes[pos_inds], pos_gt[:, :7], ious, lab[pos_inds])
        rois = torch.cat([boxes[pos_inds], boxes[neg_inds]])
        out.append((torch.nn.functional.pad(rois, (1, 0), value=float(s)), label, targets, reg_mask, pos_gt[:, :7], lab[pos_inds]))
    return out


def composed_loss(parts, cls_all, bbox_all, nonempty_all):
    rois = torch.cat([p[0] for p in parts])
    n = rois.size(0)
    cls_score, bbox_pred, nonempty = cls_all[:n], bbox_all[:n], nonempty_all[:n]
    labels, targets = torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])
    reg_mask = torch.cat([p[3] for p in parts]).clone()
    pos_gt, pos_labels = torch.cat([p[4] for p in parts]), torch.cat([p[5] for p in parts])
    pos_batch = torch.cat([torch.full((len(p[2]),), i, dtype=torch.int) for i, p in enumerate(parts)]).to(rois.device)
    weights = nonempty.float()
    reg_mask[~nonempty] = 0
    bce = torch.nn.functional.binary_cross_entropy_with_logits(cls_score.view(-1), labels, reduction='none')
    losses = [WEIGHTS[0] * (bce * weights).sum() / n]
    pos_inds = reg_mask > 0
    read()
    num_pos = pos_inds.sum().item()
    read()
    if not bool(pos_inds.any()):
        return losses + [bbox_pred.sum() * 0, bbox_pred.sum() * 0]
    pos_pred = masked(bbox_pred, pos_inds)

    def refilter(data):                                          # filter_pos_assigned_but_empty_rois
        read()
        bsz = int(rois[:, 0].max().item()) + 1
        kept = []
        for b in range(bsz):
            kept.append(masked(data, pos_batch == b)[nonzero(masked(pos_inds, rois[:, 0].int() == b))])
        return torch.cat(kept, 0)

    targets = refilter(targets)
    read()
    assert not bool((pos_pred == -1).all(1).any())
    losses.append(WEIGHTS[1] * (pos_pred - targets).abs().sum() / num_pos)
    pos_rois = masked(rois[:, 1:8], pos_inds)
    anchors = pos_rois.clone().detach()
    anchors[:, 0:3] = 0
    pred = decode(anchors, pos_pred)
    pred = torch.cat([rotate_z(pred[:, 0:3], pos_rois[:, 6] + math.pi / 2) + pos_rois[:, 0:3], pred[:, 3:]], 1)
    gt, gt_labels = refilter(pos_gt), refilter(pos_labels)
    car = gt_labels == 0
    gt, pred = masked(gt, car), masked(pred, car)
    if len(gt) > 0:
        flip = gt.clone()
        flip[:, 6] += math.pi
        pc = corners(pred)
        dist = torch.min(torch.norm(pc - corners(gt), dim=2), torch.norm(pc - corners(flip), dim=2))
        quad = torch.clamp(dist, max=1)
        losses.append(WEIGHTS[2] * (0.5 * quad ** 2 + (dist - quad)).mean())
    else:
        losses.append(bbox_pred.sum() * 0)
    return losses


def scene(n_props, n_boxes, seed):
    g = torch.Generator().manual_seed(seed)
    props, plabels, gts, glabels = [], [], [], []
    for _ in range(2):
        b = torch.zeros(n_boxes, 7)
        b[:, :2] = (torch.rand(n_boxes, 2, generator=g) - 0.5) * 140
        b[:, 2] = -1.5 + torch.rand(n_boxes, generator=g) * 0.5
        b[:, 3:6] = torch.tensor([2.0, 4.6, 1.6]) * (0.8 + 0.45 * torch.rand(n_boxes, 3, generator=g))
        b[:, 6] = (torch.rand(n_boxes, generator=g) - 0.5) * 6.28
        gl = torch.randint(0, 3, (n_boxes,), generator=g)
        of = torch.randint(0, n_boxes, (n_props,), generator=g)
        scale = torch.tensor([0.05, 0.15, 0.4, 0.8])[torch.randint(0, 4, (n_props,), generator=g)][:, None]
        p = b[of] + torch.randn(n_props, 7, generator=g) * torch.tensor([0.8, 0.8, 0.3, 0.3, 0.5, 0.2, 0.3]) * scale
        p[:, 3:6] = p[:, 3:6].clamp(min=0.3)
        far = torch.rand(n_props, generator=g) < 0.3
        p[far, :2] = (torch.rand(int(far.sum()), 2, generator=g) - 0.5) * 140
        props.append(p.to(DEV).contiguous()), plabels.append(gl[of].to(DEV)), gts.append(b.to(DEV)), glabels.append(gl.to(DEV))
    rows = 2 * CFG['num']
    cls_score = (torch.randn(rows, 1, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    bbox_pred = (torch.randn(rows, 7, generator=g) * 0.3).to(DEV).requires_grad_(True)
    nonempty = (torch.rand(rows, generator=g) < 0.85).to(DEV)
    return props, plabels, gts, glabels, cls_score, bbox_pred, nonempty


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'statistic': 'median (min) of device-event times, '
           'the middle one of three alternating rounds', 'cases': []}
    for n_props in (300, 1500):
        props, plabels, gts, glabels, cls_score, bbox_pred, nonempty = scene(n_props, 60, seed=n_props)
        leaves = [cls_score, bbox_pred]
        all_gts = torch.cat(gts)

        def backward(losses):
            for t in leaves:
                t.grad = None
            sum(losses).backward()

        def fused_assign():
            return sst_amd.roi_compact(sst_amd.roi_assign_sample(props, plabels, gts, glabels, **CFG))

        def fused_loss_fwd(rows):
            n = rows['rois'].size(0)
            out = sst_amd.roi_loss(cls_score[:n], bbox_pred[:n], nonempty[:n], rows['rois'], rows['soft_label'], rows['reg_mask'],
                                   rows['targets'], rows['gt_index'], rows['labels'], all_gts, loss_weights=WEIGHTS,
                                   with_corner_loss=True, car_index=0)
            return list(out[:3])

        def fused():
            out = fused_loss_fwd(fused_assign())
            backward(out)
            return out

        def composed_assign_fn():
            return composed_assign(props, plabels, gts, glabels)

        def composed():
            out = composed_loss(composed_assign_fn(), cls_score, bbox_pred, nonempty)
            backward(out)
            return out

        rows_f, parts_c = fused_assign(), composed_assign_fn()
        fused(), composed()
        rounds = {k: [] for k in ('fused', 'composed', 'fused_assign', 'composed_assign', 'fused_loss', 'composed_loss')}
        for _ in range(3):                       # alternate the paths: other work shares the machine
            rounds['fused'].append(median_ms(fused, args.iters))
            rounds['composed'].append(median_ms(composed, args.iters))
            rounds['fused_assign'].append(median_ms(fused_assign, args.iters))
            rounds['composed_assign'].append(median_ms(composed_assign_fn, args.iters))
            rounds['fused_loss'].append(median_ms(lambda: backward(fused_loss_fwd(rows_f)), args.iters))
            rounds['composed_loss'].append(median_ms(lambda: backward(composed_loss(parts_c, cls_score, bbox_pred, nonempty)),
                                                     args.iters))
        SYNCS[0] = 0
        composed()
        syncs = SYNCS[0]
        # the two paths draw different random numbers; what does not depend on the draw must agree: the pool of positives is
        # below its cap at these sizes, so every positive is taken by both
        pos_f = [int(c[0]) for c in rows_f['counts']]
        pos_c = [int(p[3].sum()) for p in parts_c]
        case = dict(proposals_per_sample=n_props, samples=2, boxes_per_sample=60, num=CFG['num'], rois_fused=int(rows_f['rois'].size(0)),
                    rois_composed=int(sum(p[0].size(0) for p in parts_c)), positives_fused=pos_f, positives_composed=pos_c,
                    composed_host_reads=syncs, fused_host_reads=1)
        for k, v in rounds.items():
            case[k + '_ms'] = round(sorted(m for m, _ in v)[1], 4)
            case[k + '_min_ms'] = round(min(m for _, m in v), 4)
            case[k + '_rounds_ms'] = [round(m, 4) for m, _ in v]
        case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
        if not args.no_profiler:
            total = sum(fused_loss_fwd(rows_f))
            case['fused_launches'] = dict(
                assign=count_launches(fused_assign, True), loss_fwd=count_launches(lambda: fused_loss_fwd(rows_f), True),
                loss_bwd=count_launches(lambda: torch.autograd.grad(total, leaves, retain_graph=True), True),
                step=count_launches(fused))
            case['composed_launches'] = dict(step=count_launches(composed))
        res['cases'].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
