"""Times the training side of VoteSegHead (csrc/seg_loss.hip) - point targets + loss forward + loss backward - with device
events after warm-up (the median of --iters separately timed steps), against the same function composed from torch ops on the
same device in the reference's data flow (decode_heads/segmentation_head.py:106-275: a Python loop over the samples with a
points-in-boxes launch and boolean-index compactions each, element-wise losses, the asserts with their read-backs, autograd's
backward).  Prints one JSON object.

    python tools/seg_loss_bench.py [--iters 30] [--out profiles/seg_loss/seg_loss_bench.json] [--no-profiler]

Sizes: N = 160 000 points, C = 3 sigmoid focal (the Waymo configs), and N = 300 000, C = 11 softmax cross entropy (nuScenes);
2 samples x 40 boxes each.  Per step and path: milliseconds, kernel launches (counted by torch.profiler in a separate, untimed
step; null when the profiler is not available) and host synchronisations (counted in the composed code: every .item(), bool()
of a device value and boolean-index compaction; the fused path has none).  The algorithmic bytes of the three fused entry
points are computed from the shapes.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_common import count_launches, median_ms  # noqa: E402
import sst_amd  # noqa: E402
from sst_amd import seg_loss  # noqa: E402

DEV = 'cuda:0'
SYNCS = [0]


def read(x):
    SYNCS[0] += 1
    return x.item()


def compact(t, mask):
    SYNCS[0] += 1          # a boolean index reads the number of selected rows back
    return t[mask]


def composed_targets(points_list, boxes_list, labels_list, bg_label):
    """get_targets / get_point_labels / get_vote_target / encode_vote_targets as the reference writes them"""
    label_list, target_list, mask_list = [], [], []
    for points, bboxes, bbox_labels in zip(points_list, boxes_list, labels_list):
        points = points[:, :3]
        valid = bbox_labels >= 0
        bboxes, bbox_labels = compact(bboxes, valid), compact(bbox_labels, valid)
        inbox = sst_amd.points_in_boxes_gpu(points[None].contiguous(), bboxes[None].contiguous())[0].long()
        bg = inbox < 0
        labels = bbox_labels[inbox]
        labels[bg] = bg_label
        centre = torch.zeros_like(bboxes[:, :3])
        centre[:, :2] = bboxes[:, :2]
        centre[:, 2] = bboxes[:, 2] + bboxes[:, 5] * 0.5
        delta = centre[inbox] - points
        delta[bg] = 0
        label_list.append(labels)
        target_list.append(torch.sign(delta) * (delta.abs() ** 0.5))
        mask_list.append(~bg)
    return torch.cat(label_list), torch.cat(target_list), torch.cat(mask_list)


def composed_losses(logits, vote_preds, labels, vote_targets, vote_mask, spec):
    """losses() as the reference writes it, with py_sigmoid_focal_loss / F.cross_entropy / L1 underneath"""
    c = logits.size(1)
    z = logits * spec['logit_scale']
    if spec['mode'] == seg_loss.SIGMOID_FOCAL:
        target = F.one_hot(labels, c + 1)[:, :c].type_as(z)
        p = z.sigmoid()
        one_minus_pt = (1 - p) * target + p * (1 - target)
        weight = (spec['alpha'] * target + (1 - spec['alpha']) * (1 - target)) * one_minus_pt.pow(spec['gamma'])
        loss_sem = (F.binary_cross_entropy_with_logits(z, target, reduction='none') * weight).mean()
        assert read(labels.max()) == c
    else:
        loss_sem = F.cross_entropy(z, labels, weight=spec['class_weight_t'], reduction='none').mean()
        assert read(labels.max()) == c - 1
    votes = compact(vote_preds.reshape(-1, c, 3), vote_mask).reshape(-1, 3)
    num_valid = vote_mask.sum()
    valid_label = compact(labels, vote_mask)
    SYNCS[0] += 1
    if num_valid > 0:
        assert read(valid_label.max()) < c and read(valid_label.min()) >= 0
        idx = torch.arange(num_valid, device=labels.device) * c + valid_label
        loss_vote = (votes[idx] - compact(vote_targets, vote_mask)).abs().mean()
    else:
        loss_vote = vote_preds.sum() * 0
    out = {'loss_sem_seg': loss_sem * spec['w_decode'], 'loss_vote': loss_vote}
    thr = spec['score_thresh']
    if spec['mode'] == seg_loss.SIGMOID_FOCAL:
        scores = z.sigmoid()
        for i in range(c):
            real = labels == i
            out[f'recall_{i}'] = ((scores[:, i] > thr[i]) & real).sum().float() / (real.sum().float() + 1e-5)
    else:
        score = z.softmax(1)[:, :-1]
        num_fg = score.new_zeros(1)
        for gi, members in enumerate(spec['groups']):
            pred = score[:, members].sum(1) > thr[gi]
            num_fg += pred.sum().float()
            for k in members:
                real = labels == k
                out[f'recall_{k}'] = (pred & real).sum().float() / (real.sum().float() + 1e-5)
        out['num_fg'] = num_fg
    return out


def scene(n, n_boxes, seed):
    """two samples of n / 2 points around n_boxes boxes each; a few boxes labelled -1"""
    g = torch.Generator().manual_seed(seed)
    points, boxes = [], []
    for s in range(2):
        m = n // 2 + (n % 2) * s
        b = torch.zeros(n_boxes, 7)
        b[:, :2] = (torch.rand(n_boxes, 2, generator=g) - 0.5) * 120
        b[:, 2] = -1.5 + torch.rand(n_boxes, generator=g) * 0.5
        b[:, 3:6] = torch.tensor([2.0, 4.5, 1.7]) * (0.6 + 0.8 * torch.rand(n_boxes, 3, generator=g))
        b[:, 6] = (torch.rand(n_boxes, generator=g) - 0.5) * 6.28
        which = torch.randint(0, n_boxes, (m,), generator=g)
        near = b[which, :3] + torch.tensor([0, 0, 0.8]) + torch.randn(m, 3, generator=g) * torch.tensor([1.5, 1.5, 0.5])
        far = (torch.rand(m, 3, generator=g) - 0.5) * torch.tensor([150.0, 150.0, 0.3]) + torch.tensor([0, 0, -1.7])
        xyz = torch.where(torch.rand(m, 1, generator=g) < 0.25, near, far)
        points.append(torch.cat([xyz, torch.rand(m, 2, generator=g)], 1).to(DEV))
        boxes.append(b.to(DEV))
    return points, boxes


def count_kernels(fn):
    n = count_launches(fn, ours='seg_')
    return n['ours'] + n['torch'] if n else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'statistic': 'median (min) of device-event times',
           'cases': []}
    nusc_groups = [[0], [1, 4], [3, 2], [9], [6, 5], [7, 8]]
    specs = [
        dict(name='waymo_sigmoid_focal', n=160000, c=3, mode=seg_loss.SIGMOID_FOCAL, n_fg=3, logit_scale=1.0, gamma=3.0,
             alpha=0.8, w_decode=1.0, score_thresh=[0.3, 0.25, 0.25], class_weight=None, groups=None),
        dict(name='nusc_softmax_ce', n=300000, c=11, mode=seg_loss.SOFTMAX_CE, n_fg=10, logit_scale=1.0, gamma=2.0, alpha=0.25,
             w_decode=10.0, score_thresh=[0.2, 0.2, 0.2, 0.1, 0.1, 0.1], class_weight=[1.0] * 10 + [0.1], groups=nusc_groups),
    ]
    for spec in specs:
        n, c = spec['n'], spec['c']
        points, boxes = scene(n, 40, seed=c)
        g = torch.Generator().manual_seed(1)
        labels = [torch.randint(0, spec['n_fg'], (40,), generator=g).to(DEV) for _ in range(2)]
        for l in labels:
            l[::13] = -1
        logits = (torch.randn(n, c, generator=g) * 2).to(DEV).requires_grad_(True)
        votes = torch.randn(n, 3 * c, generator=g).to(DEV).requires_grad_(True)
        spec['class_weight_t'] = None if spec['class_weight'] is None else torch.tensor(spec['class_weight'], device=DEV)
        group_of = None
        if spec['groups'] is not None:
            group_of = [-1] * (c - 1)
            for gi, members in enumerate(spec['groups']):
                for k in members:
                    group_of[k] = gi
        thr_t = torch.tensor(spec['score_thresh'], device=DEV)
        grp_t = None if group_of is None else torch.tensor(group_of, dtype=torch.int32, device=DEV)
        bg = spec['n_fg']

        def fused():
            logits.grad = votes.grad = None
            lab, tgt, mask, _ = seg_loss.seg_point_targets(points, boxes, labels, bg)
            out = seg_loss.seg_vote_loss(logits, votes, lab, tgt, mask, mode=spec['mode'], logit_scale=spec['logit_scale'],
                                         gamma=spec['gamma'], alpha=spec['alpha'], class_weight=spec['class_weight_t'],
                                         loss_weight_decode=spec['w_decode'], score_thresh=thr_t, class_group=grp_t)
            (out[0] + out[1]).backward()
            return out

        def composed():
            logits.grad = votes.grad = None
            lab, tgt, mask = composed_targets(points, boxes, labels, bg)
            out = composed_losses(logits, votes, lab, tgt, mask, spec)
            (out['loss_sem_seg'] + out['loss_vote']).backward()
            return out

        a, b = fused(), composed()
        gap = dict(loss_sem=abs(float(a[0]) - float(b['loss_sem_seg'])) / abs(float(b['loss_sem_seg'])),
                   loss_vote=abs(float(a[1]) - float(b['loss_vote'])) / abs(float(b['loss_vote'])))
        fused_ms, composed_ms = [], []
        for _ in range(3):                       # alternate the two paths: other work shares the machine
            fused_ms.append(median_ms(fused, args.iters, warmup=5))
            composed_ms.append(median_ms(composed, args.iters, warmup=5))
        SYNCS[0] = 0
        composed()
        syncs = SYNCS[0]
        # what the algorithm has to move: inputs read once, outputs written once (fp32 / int64 labels / uint8 mask)
        targets_bytes = n * (12 + 4 + 8 + 12 + 1) + 80 * (28 + 8)
        fwd_bytes = n * (4 * c + 8 + 1) + int(mask_rows(fused)) * 24
        bwd_bytes = n * (4 * c + 8 + 1 + 12) + n * 4 * c + n * 12 * c
        f_med = sorted(m for m, _ in fused_ms)[1]
        c_med = sorted(m for m, _ in composed_ms)[1]
        res['cases'].append(dict(
            name=spec['name'], N=n, C=c, samples=2, boxes_per_sample=40,
            fused_ms=round(f_med, 4), fused_min_ms=round(min(m for _, m in fused_ms), 4),
            fused_rounds_ms=[round(m, 4) for m, _ in fused_ms],
            composed_ms=round(c_med, 4), composed_min_ms=round(min(m for _, m in composed_ms), 4),
            composed_rounds_ms=[round(m, 4) for m, _ in composed_ms],
            composed_over_fused=round(c_med / f_med, 2),
            fused_launches=None if args.no_profiler else count_kernels(fused),
            composed_launches=None if args.no_profiler else count_kernels(composed),
            fused_host_syncs=0, composed_host_syncs=syncs,
            algorithmic_bytes=dict(targets=targets_bytes, loss_fwd=fwd_bytes, loss_bwd=bwd_bytes),
            relative_gap_fused_vs_composed=gap))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


def mask_rows(fused):
    """masked points of the scene (they add a 12-byte vote gather and a 12-byte target read each to the forward)"""
    return int(fused()[4][0].item())


if __name__ == '__main__':
    main()
