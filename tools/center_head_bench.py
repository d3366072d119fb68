"""Times the training side of CenterHead (csrc/center_head.hip) - targets + loss forward + loss backward of one task - with
device events after warm-up (the median of --iters separately timed steps, three alternating rounds), against the same step
composed from torch ops on the same device in the reference's data flow (dense_heads/centerpoint_head.py:385-610: a Python loop
over every box of every sample with scalar-tensor arithmetic, a numpy Gaussian, a host-to-device copy and a torch.max on a slice
each; then clip_sigmoid, the Gaussian focal loss element-wise, num_pos read back, the concatenated and permuted regression map,
gather, L1, autograd's backward).  Prints one JSON object.

    python tools/center_head_bench.py [--iters 30] [--out profiles/center_head/center_head_bench.json] [--no-profiler]

Sizes: the shipped head - 2 samples on the 468 x 468 map, 3 classes, max_objs 500 - with 150 and with 400 boxes per sample.
Per path: milliseconds of the whole step and of its targets and loss parts, kernel launches and memsets (counted by
torch.profiler in a separate, untimed step; null when the profiler is not available) and host synchronisations (counted in the
composed code: every bool() / int() / .item() of a device value and every nonzero; the fused path has none).
"""
import argparse
import functools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _bench_common  # noqa: E402
from _bench_common import median_ms  # noqa: E402
import sst_amd  # noqa: E402

DEV = 'cuda:0'
SYNCS = [0]
TASKS = [dict(num_class=3, class_names=['car', 'pedestrian', 'cyclist'])]
CFG = dict(grid_size=[468, 468, 1], voxel_size=(0.32, 0.32, 6), out_size_factor=1, dense_reg=1, gaussian_overlap=0.1,
           max_objs=500, min_radius=2, point_cloud_range=[-74.88, -74.88, -2, 74.88, 74.88, 4],
           code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0])
W_CLS, W_BBOX = 1.0, 2.0

# kernels of csrc/center_head.hip against torch's glue (concatenating the lists of boxes and labels, adding the two losses)
count_launches = functools.partial(_bench_common.count_launches, ours='center_')


def host(x):
    """a device value the host branches on"""
    SYNCS[0] += 1
    return x.item()


def radius_of(height, width, overlap):
    b1 = height + width
    r1 = (b1 + torch.sqrt(b1 ** 2 - 4 * (width * height * (1 - overlap) / (1 + overlap)))) / 2
    b2 = 2 * (height + width)
    r2 = (b2 + torch.sqrt(b2 ** 2 - 16 * ((1 - overlap) * width * height))) / 2
    b3 = -2 * overlap * (height + width)
    r3 = (b3 + torch.sqrt(b3 ** 2 - 16 * overlap * ((overlap - 1) * width * height))) / 2
    return torch.minimum(torch.minimum(r1, r2), r3)


def composed_targets(boxes_list, labels_list):
    """one task of three classes; per sample and per box what get_targets_single does"""
    osf, max_objs = CFG['out_size_factor'], CFG['max_objs']
    w, h = CFG['grid_size'][0] // osf, CFG['grid_size'][1] // osf
    pc, vs = torch.tensor(CFG['point_cloud_range']), torch.tensor(CFG['voxel_size'])
    outs = [[], [], [], []]
    for boxes, labels in zip(boxes_list, labels_list):
        full = torch.cat([boxes[:, :2], (boxes[:, 2] + boxes[:, 5] * 0.5)[:, None], boxes[:, 3:]], 1)
        picks = []
        for c in range(3):
            SYNCS[0] += 1
            picks.append(torch.where(labels == c)[0])
        order = torch.cat(picks)
        task_boxes, task_cls = full[order], labels[order]
        heatmap = full.new_zeros((3, h, w))
        anno = full.new_zeros((max_objs, 10))
        ind = labels.new_zeros(max_objs)
        mask = full.new_zeros(max_objs, dtype=torch.uint8)
        for k in range(min(task_boxes.size(0), max_objs)):
            box = task_boxes[k]
            width, length = box[3] / vs[0] / osf, box[4] / vs[1] / osf
            if host(width > 0) and host(length > 0):
                SYNCS[0] += 1
                radius = max(CFG['min_radius'], int(radius_of(length, width, CFG['gaussian_overlap'])))
                centre = torch.stack([(box[0] - pc[0]) / vs[0] / osf, (box[1] - pc[1]) / vs[1] / osf])
                cell = centre.to(torch.int32)
                x, y = int(host(cell[0])), int(host(cell[1]))
                if not (0 <= x < w and 0 <= y < h):
                    continue
                sigma = (2 * radius + 1) / 6
                yy, xx = np.ogrid[-radius:radius + 1, -radius:radius + 1]
                g = np.exp(-(xx * xx + yy * yy) / (2 * sigma * sigma))
                left, right, top, bottom = min(x, radius), min(w - x, radius + 1), min(y, radius), min(h - y, radius + 1)
                SYNCS[0] += 1          # an index taken from a device value
                patch = heatmap[task_cls[k]][y - top:y + bottom, x - left:x + right]
                piece = torch.from_numpy(g[radius - top:radius + bottom, radius - left:radius + right]).to(DEV, torch.float32)
                torch.max(patch, piece, out=patch)
                ind[k] = y * w + x
                mask[k] = 1
                anno[k] = torch.cat([centre - cell, box[2:3], box[3:6].log(), torch.sin(box[6:7]), torch.cos(box[6:7]),
                                     box[7:9]])
        for lst, t in zip(outs, (heatmap, anno, ind, mask)):
            lst.append(t)
    return [torch.stack(lst) for lst in outs]


def composed_loss(logits, heads, heatmap, anno, ind, mask):
    p = torch.clamp(logits.sigmoid(), min=1e-4, max=1 - 1e-4)
    num_pos = host(heatmap.eq(1).float().sum())
    pos = -(p + 1e-12).log() * (1 - p).pow(2) * heatmap.eq(1).float()
    neg = -(1 - p + 1e-12).log() * p.pow(2) * (1 - heatmap).pow(4)
    loss_heatmap = (pos + neg).sum() / max(num_pos, 1) * W_CLS
    pred = torch.cat(heads, 1).permute(0, 2, 3, 1).contiguous()
    pred = pred.view(pred.size(0), -1, pred.size(3))
    pred = pred.gather(1, ind.unsqueeze(2).expand(-1, -1, pred.size(2)))
    m = mask.unsqueeze(2).expand_as(anno).float() * (~torch.isnan(anno)).float()
    weights = m * m.new_tensor(CFG['code_weights'])
    loss_bbox = ((pred - anno).abs() * weights).sum() / (mask.float().sum() + 1e-4) * W_BBOX
    return loss_heatmap, loss_bbox


def scene(n_boxes, seed):
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    for _ in range(2):
        b = torch.zeros(n_boxes, 9)
        b[:, :2] = (torch.rand(n_boxes, 2, generator=g) - 0.5) * 148
        b[:, 2] = -1.5 + torch.rand(n_boxes, generator=g) * 0.5
        kind = torch.randint(0, 3, (n_boxes,), generator=g)
        b[:, 3:6] = torch.tensor([[2.0, 4.6, 1.6], [0.8, 0.9, 1.7], [0.8, 1.8, 1.7]])[kind] * (0.8 + 0.45 * torch.rand(n_boxes, 3, generator=g))
        b[:, 6] = (torch.rand(n_boxes, generator=g) - 0.5) * 6.28
        b[:, 7:9] = torch.randn(n_boxes, 2, generator=g)
        boxes.append(b.to(DEV))
        labels.append(kind.to(DEV))
    return boxes, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'statistic': 'median (min) of device-event times, '
           'the middle one of three alternating rounds', 'cases': []}
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(2, 3, 468, 468, generator=g) * 2 - 2).to(DEV).requires_grad_(True)
    heads = [torch.randn(2, c, 468, 468, generator=g).to(DEV).requires_grad_(True) for c in (2, 1, 3, 2, 2)]
    leaves = [logits] + heads

    def backward(losses):
        for t in leaves:
            t.grad = None
        (losses[0] + losses[1]).backward()

    for n_boxes in (150, 400):
        boxes, labels = scene(n_boxes, seed=n_boxes)

        def fused_targets():
            return [x[0] for x in sst_amd.center_targets(boxes, labels, TASKS, CFG, True)]

        def fused_loss_fwd(tgt):
            return sst_amd.center_loss(logits, *heads, *tgt, CFG['code_weights'], W_CLS, W_BBOX)

        def fused():
            out = fused_loss_fwd(fused_targets())
            backward(out)
            return out

        def composed():
            out = composed_loss(logits, heads, *composed_targets(boxes, labels))
            backward(out)
            return out

        a, b = fused(), composed()
        gap = dict(loss_heatmap=abs(float(a[0]) - float(b[0])) / abs(float(b[0])),
                   loss_bbox=abs(float(a[1]) - float(b[1])) / abs(float(b[1])))
        tgt_f, tgt_c = fused_targets(), composed_targets(boxes, labels)
        same_targets = bool(torch.equal(tgt_f[2], tgt_c[2]) and torch.equal(tgt_f[3], tgt_c[3]))
        rounds = {k: [] for k in ('fused', 'composed', 'fused_targets', 'composed_targets', 'fused_loss', 'composed_loss')}
        for _ in range(3):                       # alternate the paths: other work shares the machine
            rounds['fused'].append(median_ms(fused, args.iters))
            rounds['composed'].append(median_ms(composed, args.iters))
            rounds['fused_targets'].append(median_ms(fused_targets, args.iters))
            rounds['composed_targets'].append(median_ms(lambda: composed_targets(boxes, labels), args.iters))
            rounds['fused_loss'].append(median_ms(lambda: backward(fused_loss_fwd(tgt_f)), args.iters))
            rounds['composed_loss'].append(median_ms(lambda: backward(composed_loss(logits, heads, *tgt_c)), args.iters))
        SYNCS[0] = 0
        composed()
        syncs = SYNCS[0]
        case = dict(samples=2, boxes_per_sample=n_boxes, map=[468, 468], classes=3, max_objs=500,
                    composed_host_syncs=syncs, fused_host_syncs=0, relative_gap_fused_vs_composed=gap,
                    ind_and_mask_equal=same_targets)
        for k, v in rounds.items():
            case[k + '_ms'] = round(sorted(m for m, _ in v)[1], 4)
            case[k + '_min_ms'] = round(min(m for _, m in v), 4)
            case[k + '_rounds_ms'] = [round(m, 4) for m, _ in v]
        case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
        if not args.no_profiler:
            out = fused_loss_fwd(tgt_f)
            case['fused_launches'] = dict(
                targets=count_launches(fused_targets, True), loss_fwd=count_launches(lambda: fused_loss_fwd(tgt_f), True),
                loss_bwd=count_launches(lambda: torch.autograd.grad(out[0] + out[1], leaves, retain_graph=True), True),
                step=count_launches(fused))
            case['composed_launches'] = dict(step=count_launches(composed))
        # what the algorithm has to move: inputs read once, outputs written once
        cells, slots = 2 * 3 * 468 * 468, 2 * 500
        case['algorithmic_bytes'] = dict(
            targets=2 * n_boxes * (36 + 8) + cells * 4 + slots * (40 + 8 + 1), loss_fwd=cells * 8 + slots * (40 + 8 + 1 + 40),
            loss_bwd=cells * 12 + 2 * 10 * 468 * 468 * 4 + slots * (40 + 8 + 1 + 80))
        res['cases'].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
