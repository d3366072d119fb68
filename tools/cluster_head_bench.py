"""Times the training side of the FSD cluster heads (csrc/cluster_head.hip) - targets + loss forward + loss backward of all
tasks - with device events after warm-up (the median of --iters separately timed steps, three alternating rounds), against the
same step composed from torch ops on the same device in the reference's data flow (dense_heads/sparse_cluster_head_v2.py:160-405,
sparse_cluster_head.py:250-483: per task the regrouping of the ground truth by class, per task and sample two boolean-mask
compactions, a points-in-boxes launch, an ``.any()`` read-back, index assignments, an ``encode`` and the masked scatter back; per
task a focal loss, ``nonzero()``, the gathered L1 losses and ``assert (label_weights == 1).all()``; autograd's backward).  The
composed path's points-in-boxes is this library's kernel (``sst_amd.points_in_boxes_gpu``).  Prints one JSON object.

    python tools/cluster_head_bench.py [--iters 30] [--out profiles/cluster_head/cluster_head_bench.json] [--no-profiler]

Sizes: N = 3 000 rows, 3 single-class tasks, 2 samples of 80 boxes (FSD on Waymo); N = 60 000 rows, 2 tasks of 5 classes, code
size 10, 2 samples of 80 boxes (FSDv2 on nuScenes).  Per path: milliseconds of the whole step and of its targets and loss parts,
kernel launches (counted by torch.profiler in a separate, untimed step; null when the profiler is not available) and host reads
(counted in the composed code: every bool() / int() / .item() of a device value, every boolean-mask index and every nonzero; the
fused path has none).
"""
import argparse
import functools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _bench_common  # noqa: E402
from _bench_common import median_ms  # noqa: E402
import sst_amd  # noqa: E402

DEV = 'cuda:0'
SYNCS = [0]
GAMMA, ALPHA = 2.0, 0.25
WEIGHTS = [2.0, 0.5, 0.5, 0.2, 0.2]


def masked(t, mask):
    """a boolean-mask compaction: its size comes back to the host"""
    SYNCS[0] += 1
    return t[mask]


def encode(boxes, base, code):
    parts = [boxes[:, :3] - base, (boxes[:, 3:6] + 1e-6).log(), boxes[:, 6:7].sin(), boxes[:, 6:7].cos()]
    if code == 10:
        parts.append(boxes[:, 7:9])
    return torch.cat(parts, 1)


def composed_targets_task(task, names, xyz, bidx, boxes_list, labels_list, code):
    """get_targets of one task -> (labels, label_weights, bbox_targets, bbox_weights)"""
    c = len(task['class_names'])
    n = xyz.size(0)
    batch = len(boxes_list)
    outs = [xyz.new_zeros(n, dtype=torch.long), xyz.new_zeros(n), xyz.new_zeros((n, code)), xyz.new_zeros((n, code))]
    for s in range(batch):
        # modify_gt_for_single_task_single_sample: the sample's boxes regrouped by the task's classes
        gb, gl = boxes_list[s], labels_list[s]
        SYNCS[0] += 1                                        # assert (gt_labels_3d >= 0).all()
        bool((gl >= 0).all())
        picked_b, picked_l = [], []
        for i, name in enumerate(task['class_names']):
            m = gl == names.index(name)
            picked_b.append(masked(gb, m))
            picked_l.append(gl.new_ones(picked_b[-1].size(0)) * i)
        gb, gl = torch.cat(picked_b), torch.cat(picked_l)
        # split_by_batch, get_targets_single, combine_by_batch
        mask = bidx == s
        pts = masked(xyz, mask)
        labels = gl.new_full((pts.size(0),), c)
        tg, wt = pts.new_zeros((pts.size(0), code)), pts.new_zeros((pts.size(0), code))
        valid = gl >= 0
        gb, gl = masked(gb, valid), masked(gl, valid)
        if gb.size(0) and pts.size(0):
            inbox = sst_amd.points_in_boxes_gpu(pts.unsqueeze(0), gb[:, :7].unsqueeze(0).contiguous()).squeeze(0).long()
            pos = inbox > -1
            SYNCS[0] += 1
            if bool(pos.any()):
                pos_inds = torch.nonzero(pos, as_tuple=False).squeeze(-1)
                SYNCS[0] += 1
                assigned = inbox[pos_inds]
                labels[pos_inds] = gl[assigned]
                wt[pos_inds] = 1.0
                pb = gb[assigned]
                tg[pos_inds] = encode(pb, pts[pos_inds], code)
                if pb.size(1) == 10:
                    SYNCS[0] += 2                            # the two asserts on the copy-paste flag
                    pb[:, 9].max().item(), pb[:, 9].min().item()
                    wt[pos_inds, -2:] = pb[:, [9]]
        for full, part in zip(outs, (labels, pts.new_ones(pts.size(0)), tg, wt)):
            SYNCS[0] += 1                                    # full_data[sample_mask] = data
            full[mask] = part
    return outs


def composed_loss_task(logits, reg, labels, label_weights, tg, wt, code):
    c = logits.size(1)
    SYNCS[0] += 1
    assert bool((label_weights == 1).all())
    target = torch.nn.functional.one_hot(labels, c + 1)[:, :c].float()
    p = logits.sigmoid()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(logits, target, reduction='none')
    focal = bce * (ALPHA * target + (1 - ALPHA) * (1 - target)) * (target - p).abs().pow(GAMMA)
    losses = [WEIGHTS[0] * (focal * label_weights[:, None]).sum() / logits.size(0)]
    pos_inds = ((labels >= 0) & (labels < c)).nonzero(as_tuple=False).reshape(-1)
    SYNCS[0] += 1
    num_pos = len(pos_inds)
    pr, pt, pw = reg[pos_inds], tg[pos_inds], wt[pos_inds]
    for k, (lo, hi) in enumerate(((0, 3), (3, 6), (6, 8), (8, 10))):
        if lo >= code:
            continue
        if num_pos == 0:
            losses.append(pr.sum() * 0)
        else:
            e = ((pr[:, lo:hi] - pt[:, lo:hi]).abs() * pw[:, lo:hi])
            losses.append(WEIGHTS[k + 1] * (e.mean() if k == 3 else e.sum() / num_pos))
    return losses


def scene(n, tasks, names, cols, seed):
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    for _ in range(2):
        b = torch.zeros(80, cols)
        b[:, :2] = (torch.rand(80, 2, generator=g) - 0.5) * 140
        b[:, 2] = -1.5 + torch.rand(80, generator=g) * 0.5
        b[:, 3:6] = torch.tensor([2.0, 4.6, 1.6]) * (0.8 + 0.45 * torch.rand(80, 3, generator=g))
        b[:, 6] = (torch.rand(80, generator=g) - 0.5) * 6.28
        if cols > 7:
            b[:, 7:9] = torch.randn(80, 2, generator=g)
        if cols == 10:
            b[:, 9] = (torch.rand(80, generator=g) < 0.7).float()
        boxes.append(b.to(DEV))
        labels.append(torch.randint(0, len(names), (80,), generator=g).to(DEV))
    bidx = torch.randint(0, 2, (n,), generator=g)
    which = torch.randint(0, 80, (n,), generator=g)
    centre = torch.stack([b.cpu() for b in boxes])[bidx, which, :3]
    near = centre + torch.tensor([0.0, 0.0, 0.8]) + torch.randn(n, 3, generator=g) * torch.tensor([1.2, 1.2, 0.5])
    far = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([150.0, 150.0, 4.0])
    xyz = torch.where(torch.rand(n, 1, generator=g) < 0.6, near, far).to(DEV).contiguous()
    cls = torch.sort(torch.randint(0, len(names), (n,), generator=g))[0]
    inds = torch.stack([cls, bidx, torch.arange(n)], 1).to(DEV)
    code = 8 if cols == 7 else 10
    logits = [(torch.randn(n, len(t['class_names']), generator=g) * 2 - 2).to(DEV).requires_grad_(True) for t in tasks]
    reg = [torch.randn(n, code, generator=g).to(DEV).requires_grad_(True) for _ in tasks]
    return boxes, labels, xyz, inds, logits, reg, code


READBACK_NAMES = set()


def learn_readback_names():
    """the names under which this profiler shows the copy of a host read (a deliberate ``float(tensor)``)"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            float(torch.zeros(2, device=DEV).sum())
            torch.cuda.synchronize()
        READBACK_NAMES.update(e.name for e in prof.events() if e.device_type == DeviceType.CUDA and 'memcpy' in e.name.lower())
    except Exception:
        pass


# kernels of csrc/cluster_head.hip, and those copies that look like a host read
count_launches = functools.partial(_bench_common.count_launches, ours='cluster_', readback_names=READBACK_NAMES)


WAYMO = (['Car', 'Pedestrian', 'Cyclist'], [dict(class_names=['Car']), dict(class_names=['Pedestrian']),
                                            dict(class_names=['Cyclist'])])
NUSC_NAMES = ['car', 'truck', 'trailer', 'bus', 'construction_vehicle', 'bicycle', 'motorcycle', 'pedestrian', 'traffic_cone',
              'barrier']
NUSC = (NUSC_NAMES, [dict(class_names=NUSC_NAMES[:5]), dict(class_names=NUSC_NAMES[5:])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'statistic': 'median (min) of device-event times, '
           'the middle one of three alternating rounds', 'cases': []}
    for n, (names, tasks), cols in ((3000, WAYMO, 7), (60000, NUSC, 10)):
        boxes, labels, xyz, inds, logits, reg, code = scene(n, tasks, names, cols, seed=n)
        leaves = logits + reg
        bidx = inds[:, 1].contiguous()

        def backward(losses):
            for t in leaves:
                t.grad = None
            sum(losses).backward()

        def fused_targets():
            return sst_amd.cluster_targets(xyz, inds, boxes, labels, tasks, names, code)

        def fused_loss_fwd(tg):
            losses, _ = sst_amd.cluster_loss(logits, reg, [t[0] for t in tg], [t[2] for t in tg], [t[3] for t in tg], gamma=GAMMA,
                                             alpha=ALPHA, loss_weights=WEIGHTS)
            return [l for task in losses for l in task[:code // 2]]

        def fused():
            out = fused_loss_fwd(fused_targets())
            backward(out)
            return out

        def composed_targets():
            return [composed_targets_task(t, names, xyz, bidx, boxes, labels, code) for t in tasks]

        def composed_loss_fwd(tg):
            return [l for t in range(len(tasks)) for l in composed_loss_task(logits[t], reg[t], *tg[t], code)]

        def composed():
            out = composed_loss_fwd(composed_targets())
            backward(out)
            return out

        a, b = fused(), composed()
        gap = max(abs(float(x) - float(y)) / max(abs(float(y)), 1e-12) for x, y in zip(a, b))
        tg_f, tg_c = fused_targets(), composed_targets()
        same = all(bool(torch.equal(f[0], c[0]) and torch.equal(f[3], c[3])) for f, c in zip(tg_f, tg_c))
        rounds = {k: [] for k in ('fused', 'composed', 'fused_targets', 'composed_targets', 'fused_loss', 'composed_loss')}
        for _ in range(3):                       # alternate the paths: other work shares the machine
            rounds['fused'].append(median_ms(fused, args.iters))
            rounds['composed'].append(median_ms(composed, args.iters))
            rounds['fused_targets'].append(median_ms(fused_targets, args.iters))
            rounds['composed_targets'].append(median_ms(composed_targets, args.iters))
            rounds['fused_loss'].append(median_ms(lambda: backward(fused_loss_fwd(tg_f)), args.iters))
            rounds['composed_loss'].append(median_ms(lambda: backward(composed_loss_fwd(tg_c)), args.iters))
        SYNCS[0] = 0
        composed()
        syncs = SYNCS[0]
        case = dict(rows=n, tasks=len(tasks), classes=len(names), code_size=code, samples=2, boxes_per_sample=80,
                    positive_rows=[int((t[1] >= 0).sum()) for t in tg_f], composed_host_reads=syncs, fused_host_reads=0,
                    largest_relative_gap_fused_vs_composed=gap, labels_and_weights_equal=same)
        for k, v in rounds.items():
            case[k + '_ms'] = round(sorted(m for m, _ in v)[1], 4)
            case[k + '_min_ms'] = round(min(m for _, m in v), 4)
            case[k + '_rounds_ms'] = [round(m, 4) for m, _ in v]
        case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
        if not args.no_profiler:
            total = sum(fused_loss_fwd(tg_f))
            learn_readback_names()
            case['fused_launches'] = dict(
                targets=count_launches(fused_targets, True), loss_fwd=count_launches(lambda: fused_loss_fwd(tg_f), True),
                loss_bwd=count_launches(lambda: torch.autograd.grad(total, leaves, retain_graph=True), True),
                step=count_launches(fused))
            case['composed_launches'] = dict(step=count_launches(composed))
        # what the algorithm has to move: inputs read once, outputs written once
        c_all = sum(len(t['class_names']) for t in tasks)
        case['algorithmic_bytes'] = dict(
            targets=n * (12 + 8) + 160 * (cols * 4 + 8) + len(tasks) * n * (8 + 4 + 8 * code),
            loss_fwd=n * (4 * c_all + len(tasks) * 8) + sum(case['positive_rows']) * 12 * code,
            loss_bwd=n * (8 * c_all + len(tasks) * (8 + 4 * code)) + sum(case['positive_rows']) * 12 * code)
        res['cases'].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
