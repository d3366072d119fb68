"""Times the rotated-box ops (csrc/box_ops.hip) with device events after warm-up and prints one JSON object.

    python tools/box_ops_bench.py [--iters 20] [--out profiles/box_ops/box_ops_bench.json]

- points in boxes at 160 000 points x T in {64, 256}, B in {1, 2}, both modes; batch mode also as the fraction of 8 TB/s
  from the bytes it writes; against a torch-composed broadcast [N, T] test of the same arithmetic;
- the IoU matrix at 500 x 200 and 4096 x 4096;
- NMS over sorted boxes at N in {500, 4096, 16384}, one and three groups;
- box3d_multiclass_nms at 3 classes x 4096 candidates against the reference's data flow (a per-class Python loop over
  this library's nms_gpu), with the host read-backs of each call counted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sst_amd import box_ops as B  # noqa: E402

DEV = 'cuda:0'


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def lidar_scene(b, n_pts, t, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(b, n_pts, 3, generator=g) * torch.tensor([150.0, 150.0, 6.0]) - torch.tensor([75.0, 75.0, 2.0]))
    c = torch.rand(b, t, 3, generator=g) * torch.tensor([150.0, 150.0, 1.0]) - torch.tensor([75.0, 75.0, 2.0])
    s = torch.rand(b, t, 3, generator=g) * torch.tensor([3.0, 8.0, 2.0]) + torch.tensor([0.8, 0.8, 1.0])
    r = (torch.rand(b, t, 1, generator=g) * 2 - 1) * np.pi
    return pts.to(DEV), torch.cat([c, s, r], -1).to(DEV)


def torch_membership(pts, boxes):
    """the broadcast [N, T] test of points_in_boxes_cuda.cu:24-50 composed from torch ops"""
    cz = boxes[..., 2] + boxes[..., 5] * 0.5
    rot = boxes[..., 6] + np.pi / 2
    cosa, sina = torch.cos(rot), torch.sin(rot)
    sx = pts[..., 0:1] - boxes[:, None, :, 0]
    sy = pts[..., 1:2] - boxes[:, None, :, 1]
    lx = sx * cosa[:, None] - sy * sina[:, None]
    ly = sx * sina[:, None] + sy * cosa[:, None]
    lz = pts[..., 2:3] - cz[:, None]
    hl, hw, hh = boxes[:, None, :, 4] * 0.5, boxes[:, None, :, 3] * 0.5, boxes[:, None, :, 5] * 0.5
    return ((lz.abs() <= hh) & (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw)).int()


def bev_boxes(n, extent, seed):
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(n, 2, generator=g) * 2 - 1) * extent
    s = torch.rand(n, 2, generator=g) * 4 + 0.8
    r = (torch.rand(n, 1, generator=g) * 2 - 1) * np.pi
    return torch.cat([c - s / 2, c + s / 2, r], 1).to(DEV).contiguous()


class ReadbackCounter(object):
    """counts the .item() reads of device tensors inside the block (sst_amd.box_ops reads its kept count that way); the
    nonzero that sizes the candidate list is the only other stall of box3d_multiclass_nms, added by the caller"""

    def __init__(self):
        self.n = 0
        self._orig = torch.Tensor.item

    def __enter__(self):
        counter = self

        def item(t):
            if t.is_cuda:
                counter.n += 1
            return counter._orig(t)
        torch.Tensor.item = item
        return self

    def __exit__(self, *a):
        torch.Tensor.item = self._orig


def reference_multiclass_flow(bboxes, bboxes_for_nms, scores, score_thr, nms_thr):
    """box3d_nms.py:52-100.  Host stalls per class, counted as the code makes them: `.any()`, the boolean selections
    `mlvl_scores[cls_inds, i]`, `mlvl_bboxes_for_nms[cls_inds, :]` and `mlvl_bboxes[cls_inds, :]` (each sizes its output
    on the host), and the kept count inside nms_gpu"""
    out = []
    syncs = 0
    for i in range(scores.shape[1] - 1):
        cls_inds = scores[:, i] > score_thr
        syncs += 1
        if not cls_inds.any():
            continue
        _scores = scores[cls_inds, i]
        sel = B.nms_gpu(bboxes_for_nms[cls_inds, :], _scores, nms_thr)
        out.append(bboxes[cls_inds, :][sel])
        syncs += 4
    res = torch.cat(out)
    return res, syncs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='one size per family (for a profiler run)')
    args = ap.parse_args()
    it = args.iters
    res = {'device': torch.cuda.get_device_name(0), 'iters': it, 'points_in_boxes': [], 'iou_matrix': [], 'nms': []}

    for b in ((1,) if args.quick else (1, 2)):
        for t in ((64,) if args.quick else (64, 256)):
            pts, boxes = lidar_scene(b, 160000, t)
            first = timed(lambda: B.points_in_boxes_gpu(pts, boxes), it)
            batch = timed(lambda: B.points_in_boxes_batch(pts, boxes), it)
            comp = timed(lambda: torch_membership(pts, boxes), it)
            same = bool(torch.equal(B.points_in_boxes_batch(pts, boxes), torch_membership(pts, boxes)))
            written = 4.0 * b * 160000 * t
            res['points_in_boxes'].append(dict(
                B=b, N=160000, T=t, first_box_ms=round(first, 4), batch_ms=round(batch, 4),
                batch_fraction_of_8TBps=round(written / (batch * 1e-3) / 8e12, 4),
                torch_composed_batch_ms=round(comp, 4), torch_composed_equal=same))

    for na, nb in (((500, 200),) if args.quick else ((500, 200), (4096, 4096))):
        a, bb = bev_boxes(na, 40.0, 1), bev_boxes(nb, 40.0, 2)
        res['iou_matrix'].append(dict(n_a=na, n_b=nb, iou_ms=round(timed(lambda: B.boxes_iou_bev(a, bb), it), 4),
                                      overlap_ms=round(timed(lambda: B.boxes_overlap_bev(a, bb), it), 4)))

    for n in ((4096,) if args.quick else (500, 4096, 16384)):
        boxes = bev_boxes(n, float(np.sqrt(n)) * 1.2, 3)
        grp = (torch.arange(n, device=DEV) % 3).int()
        one = timed(lambda: B.nms_sorted(boxes, 0.25), it)
        three = timed(lambda: B.nms_sorted(boxes, 0.0, groups=grp, group_thresh=[0.25, 0.5, 0.7]), it)
        kept = B.nms_sorted(boxes, 0.25)[1]
        res['nms'].append(dict(N=n, one_group_ms=round(one, 4), three_groups_ms=round(three, 4), kept_one_group=kept))

    # multi-class NMS: 3 classes x 4096 candidates
    n = 4096
    g = torch.Generator().manual_seed(4)
    bev = bev_boxes(n, 60.0, 4)
    bboxes = torch.cat([bev, torch.randn(n, 4, generator=g).to(DEV)], 1)
    scores = torch.cat([torch.rand(n, 3, generator=g) * 0.9 + 0.1, torch.zeros(n, 1)], 1).to(DEV)
    cfg = dict(nms_thr=0.25, use_rotate_nms=True)
    ours = timed(lambda: B.box3d_multiclass_nms(bboxes, bev, scores, 0.05, 500, cfg), it)
    ref = timed(lambda: reference_multiclass_flow(bboxes, bev, scores, 0.05, 0.25), it)
    with ReadbackCounter() as rc:
        B.box3d_multiclass_nms(bboxes, bev, scores, 0.05, 500, cfg)
    res['multiclass_nms'] = dict(classes=3, candidates_per_class=n, grouped_ms=round(ours, 4),
                                 per_class_loop_ms=round(ref, 4),
                                 grouped_host_stalls_per_call=rc.n + 1,  # + the nonzero that sizes the candidate list
                                 per_class_loop_host_stalls_per_call=reference_multiclass_flow(bboxes, bev, scores, 0.05,
                                                                                               0.25)[1])
    # FSD's proposal config: nms_thr None for every class (no NMS launch)
    cfg_none = dict(nms_thr=None, use_rotate_nms=True)
    res['multiclass_nms']['all_classes_nms_none_ms'] = round(
        timed(lambda: B.box3d_multiclass_nms(bboxes, bev, scores, 0.05, 500, cfg_none), it), 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
