"""Times the device-side training augmentation (sst_amd.augment.TrainAugment, csrc/augment.hip) at the shape of a Waymo training
batch - 1 and 2 samples of 180 000 points, C = 5, 35 pasted boxes with 6 000 pasted points, 50 ground-truth boxes, shuffle on -
with device events after warm-up (the median of --iters separately timed calls, three alternating rounds).  Prints one JSON object.

    python tools/augment_bench.py [--iters 20] [--out profiles/augment/augment_bench.json]

Per batch size:
  kernels_host_in   the whole call from host tensors: packing, the one host-to-device copy, the launches, the one host read
  kernels_dev_in    the same from device tensors (the points are packed by device copies)
  kernels_noshuffle device tensors, PointShuffle off (the same sort runs: its key is the row index)
  torch_device      baseline (b): the same steps as plain torch device ops - the plane test as a matrix product, boolean indexing,
                    `@`, randperm - from device tensors
  torch_host        baseline (a): the same torch code on the CPU with 16 threads: what the reference's pipeline costs per frame
                    (its numba plane test is replaced by the matrix product, which is faster)
and, for the kernel paths, the host time of a call (a host clock around the call, which ends in the read of the counts), the
device time of each kernel (torch.profiler, a run of its own) and the algorithmic bytes - 4C read per input row and 4C written
per survivor - over the call's device time as a fraction of 8 TB/s; the key traffic is stated separately."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from _bench_common import median_ms  # noqa: E402
from sst_amd.augment import TrainAugment, box_planes  # noqa: E402

DEV = 'cuda:0'
POINTS, COLS, PASTED_BOXES, PASTED_POINTS, GT = 180000, 5, 35, 6000, 50
RANGE = [-74.88, -74.88, -2, 74.88, 74.88, 4]
HBM_BYTES_PER_S = 8e12
PIPELINE = [dict(type='ObjectSample', db_sampler=dict()),
            dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
            dict(type='GlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
                 translation_std=[0, 0, 0.2]),
            dict(type='PointsRangeFilter', point_cloud_range=RANGE), dict(type='ObjectRangeFilter', point_cloud_range=RANGE),
            dict(type='PointShuffle')]


def scene(g):
    """a sweep-like cloud (a disc, denser near the sensor), boxes on it, the pasted points inside their boxes"""
    r = 85.0 * np.sqrt(g.uniform(0, 1, POINTS)) ** 1.5
    phi = g.uniform(0, 2 * np.pi, POINTS)
    pts = np.stack([r * np.cos(phi), r * np.sin(phi), g.uniform(-2.2, 3.0, POINTS), g.uniform(0, 1, POINTS), g.uniform(0, 1, POINTS)], 1)

    def boxes(n):
        b = np.zeros((n, 7), np.float32)
        rr, pp = 70.0 * np.sqrt(g.uniform(0, 1, n)), g.uniform(0, 2 * np.pi, n)
        b[:, 0], b[:, 1], b[:, 2] = rr * np.cos(pp), rr * np.sin(pp), g.uniform(-1.5, 0, n)
        b[:, 3:6], b[:, 6] = g.uniform([1.5, 1.5, 1.2], [6, 3, 2.5], (n, 3)), g.uniform(-np.pi, np.pi, n)
        return b
    pasted, per = boxes(PASTED_BOXES), PASTED_POINTS // PASTED_BOXES
    own = []
    for b in pasted:
        k = per + (PASTED_POINTS - per * PASTED_BOXES if len(own) == 0 else 0)
        local = g.uniform(-0.45, 0.45, (k, 3)) * b[3:6]
        c, s = np.cos(b[6]), np.sin(b[6])
        own.append(np.stack([local[:, 0] * c + local[:, 1] * s + b[0], -local[:, 0] * s + local[:, 1] * c + b[1],
                             local[:, 2] + 0.5 * b[5] + b[2], g.uniform(0, 1, k), g.uniform(0, 1, k)], 1))
    return dict(points=pts.astype(np.float32), gt=boxes(GT), labels=g.randint(0, 3, GT).astype(np.int64),
                sampled=dict(gt_bboxes_3d=pasted, gt_labels_3d=g.randint(0, 3, PASTED_BOXES).astype(np.int64),
                             points=np.concatenate(own).astype(np.float32)))


def torch_pipeline(s, rec, dev, shuffle=True):
    """the chain with plain torch ops on ``dev`` (inputs already there): removal, cat, flips, rotation, scale, translation, both
    range filters, limit_yaw, randperm"""
    pts, planes = s['points_' + dev.type], s['planes_' + dev.type]
    sgn = pts[:, :3] @ planes[:, :3].T + planes[:, 3]
    inside = (sgn.view(-1, PASTED_BOXES, 6) < 0).all(-1).any(-1)
    pts = torch.cat([s['pasted_' + dev.type], pts[~inside]])
    boxes = s['boxes_' + dev.type].clone()
    labels = s['labels_' + dev.type]
    if rec['flip_h']:
        pts[:, 1] = -pts[:, 1]
        boxes[:, 1], boxes[:, 6] = -boxes[:, 1], -boxes[:, 6] + np.pi
    if rec['flip_v']:
        pts[:, 0] = -pts[:, 0]
        boxes[:, 0], boxes[:, 6] = -boxes[:, 0], -boxes[:, 6]
    c, sn = float(rec['cos']), float(rec['sin'])
    rot = torch.tensor([[c, -sn, 0], [sn, c, 0], [0, 0, 1]], dtype=torch.float32, device=dev)
    pts[:, :3] = pts[:, :3] @ rot
    boxes[:, :3] = boxes[:, :3] @ rot
    boxes[:, 6] += float(rec['angle'])
    pts[:, :3] *= float(rec['scale'])
    boxes[:, :6] *= float(rec['scale'])
    trans = torch.tensor(rec['trans'], device=dev)
    pts[:, :3] += trans
    boxes[:, :3] += trans
    r = RANGE
    keep = ((pts[:, 0] > r[0]) & (pts[:, 1] > r[1]) & (pts[:, 2] > r[2]) & (pts[:, 0] < r[3]) & (pts[:, 1] < r[4]) & (pts[:, 2] < r[5]))
    pts = pts[keep]
    bk = (boxes[:, 0] > r[0]) & (boxes[:, 1] > r[1]) & (boxes[:, 0] < r[3]) & (boxes[:, 1] < r[4])
    boxes, labels = boxes[bk], labels[bk]
    boxes[:, 6] = boxes[:, 6] - torch.floor(boxes[:, 6] / (2 * np.pi) + 0.5) * (2 * np.pi)
    if shuffle:
        pts = pts[torch.randperm(pts.size(0), device=dev)]
    return pts, boxes, labels


def host_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 4)


def kernel_times(fn):
    """device time per kernel name of one call (torch.profiler), or None"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if e.device_type == DeviceType.CUDA:
                name = e.name.replace('(anonymous namespace)::', '').split('(')[0][:48]
                out[name] = round(out.get(name, 0.0) + e.device_time / 1e3, 4)
        return out or None
    except Exception as err:                                           # the profiler is optional here, the timings are not
        return dict(error=repr(err)[:200])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench needs a GPU')
    dev = torch.device(DEV)
    torch.set_num_threads(16)
    g = np.random.RandomState(0)
    scenes = [scene(g), scene(g)]
    for s in scenes:
        planes = torch.from_numpy(box_planes(s['sampled']['gt_bboxes_3d']).reshape(-1, 4))
        for d in (dev, torch.device('cpu')):
            s['points_' + d.type] = torch.from_numpy(s['points']).to(d)
            s['pasted_' + d.type] = torch.from_numpy(s['sampled']['points']).to(d)
            s['planes_' + d.type] = planes.to(d)
            s['boxes_' + d.type] = torch.from_numpy(np.concatenate([s['gt'], s['sampled']['gt_bboxes_3d']])).to(d)
            s['labels_' + d.type] = torch.from_numpy(np.concatenate([s['labels'], s['sampled']['gt_labels_3d']])).to(d)
    result = dict(shape=dict(points=POINTS, cols=COLS, pasted_boxes=PASTED_BOXES, pasted_points=PASTED_POINTS, gt_boxes=GT),
                  device=torch.cuda.get_device_name(0), iters=args.iters, threads=torch.get_num_threads())
    for batch in (1, 2):
        use = scenes[:batch]
        aug, plain = TrainAugment.from_pipeline(PIPELINE), TrainAugment.from_pipeline(PIPELINE[:-1])
        np.random.seed(batch)
        params = aug.draw_params(batch)
        boxes, labels, sampled = [s['gt'] for s in use], [s['labels'] for s in use], [s['sampled'] for s in use]
        host_pts = [torch.from_numpy(s['points']) for s in use]
        dev_pts = [s['points_cuda'] for s in use]
        rec = aug.records(params, aug.assemble(boxes, labels, sampled, batch))
        paths = dict(kernels_host_in=lambda: aug(host_pts, boxes, labels, sampled, None, params),
                     kernels_dev_in=lambda: aug(dev_pts, boxes, labels, sampled, None, params),
                     kernels_noshuffle=lambda: plain(dev_pts, boxes, labels, sampled, None, params),
                     torch_device=lambda: [torch_pipeline(s, rec[i], dev) for i, s in enumerate(use)])
        seen = {k: [] for k in paths}
        for _ in range(3):                                             # alternating rounds: other work shares the machine
            for k, fn in paths.items():
                seen[k].append(median_ms(fn, args.iters))
        entry = {k: dict(ms=round(sorted(x for x, _ in v)[1], 4), min_ms=round(min(x for _, x in v), 4),
                         rounds_ms=[round(x, 4) for x, _ in v]) for k, v in seen.items()}
        cpu = torch.device('cpu')
        t = []
        for _ in range(args.host_iters + 1):
            t0 = time.perf_counter()
            for i, s in enumerate(use):
                torch_pipeline(s, rec[i], cpu)
            t.append((time.perf_counter() - t0) * 1e3)
        entry['torch_host'] = dict(ms=round(float(np.median(t[1:])), 3), min_ms=round(min(t[1:]), 3))
        for k in ('kernels_host_in', 'kernels_dev_in'):
            entry[k]['host_ms_per_call'] = host_ms(paths[k], args.iters)
        res = aug(dev_pts, boxes, labels, sampled, None, params)
        rows_in = sum(POINTS + PASTED_POINTS for _ in use)
        rows_out = int(res['offsets'][-1])
        algo = 4 * COLS * (rows_in + rows_out)
        passes = (33 + max(1, int(np.ceil(np.log2(max(batch, 2))))) + 7) // 8
        entry['rows_in'], entry['rows_out'], entry['algorithmic_bytes'] = rows_in, rows_out, algo
        entry['key_bytes'] = dict(classify_write=8 * rows_in, sort_passes=passes, sort_read_write=passes * 2 * 12 * rows_in,
                                  gather_key_perm_read=12 * rows_in, gather_row_reread=4 * COLS * rows_out)
        for k in ('kernels_host_in', 'kernels_dev_in', 'kernels_noshuffle'):
            entry[k]['fraction_of_8TBps_algorithmic'] = round(algo / HBM_BYTES_PER_S / (entry[k]['ms'] * 1e-3), 5)
        entry['kernel_device_ms'] = kernel_times(paths['kernels_dev_in'])
        entry['speedup_vs_torch_device'] = round(entry['torch_device']['ms'] / entry['kernels_dev_in']['ms'], 3)
        entry['speedup_vs_torch_host'] = round(entry['torch_host']['ms'] / entry['kernels_host_in']['ms'], 3)
        result[f'batch{batch}'] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
