"""Times the CTRL tracklet stage at its natural batch - 16 tracklets x 150 frames x 3 candidates, about 1 000 points per frame, the
pairs capped by max_all_point - with device events after warm-up (the median of --iters separately timed calls, three alternating
rounds), each new path against its torch counterpart on the same device and in the same process.  Prints one JSON object.

    python tools/tracklet_bench.py [--iters 10] [--out profiles/tracklet/tracklet_bench.json] [--no-profiler]

1. targets: sst_amd.tracklet_targets (packing, the one host-to-device copy and the one launch) against tests/tracklet_ref.targets on
   the device - the reference's algorithm, candidate by candidate and tracklet by tracklet, with the library's aligned IoU (the
   parent commit has no such path).  Kernel launches (torch.profiler) and host synchronisations (one call under
   torch.cuda.set_sync_debug_mode('warn'), warnings counted) on each side.
2. rows: sst_amd.tracklet_rows forward + backward against torch indexing + cat + autograd (tests/tracklet_ref.rows), with the
   stage's algorithmic bytes over the measured time as a fraction of 8 TB/s.
3. pool: the existing dynamic_point_pool_mixed at this shape - 2 400 RoIs, combined mode, caps 300 000 (training) and 600 000
   (testing) pairs."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import _bench_common  # noqa: E402
from _bench_common import median_ms  # noqa: E402
from fg_sample_bench import count_syncs  # noqa: E402
import tracklet_ref as T  # noqa: E402
import sst_amd  # noqa: E402

DEV = 'cuda:0'
TRACKLETS, FRAMES, CANDS, PTS_PER_FRAME, F = 16, 150, 3, 1000, 67
HBM_BYTES_PER_S = 8e12
CFG = dict(candidate_thresh=0.5, object_centric=False, iou_thr=0.5, cls_pos_thr=(0.8, 0.65, 0.7), cls_neg_thr=(0.2, 0.15, 0.25),
           num_classes=3)


def lidar(trk, name, device=None):
    t = sst_amd.LiDARTracklet('seg', name, int(trk.type), True, trk.boxes.clone(), list(trk.ts_list), list(trk.score_list))
    t.freeze()
    t.set_type(int(trk.type), 'mmdet3d')
    return t.to(device) if device is not None else t


def rounds(paths, iters):
    """three alternating rounds (other work shares the machine) -> per path (middle median, minimum, the three medians)"""
    seen = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():
            seen[k].append(median_ms(fn, iters))
    return {k: dict(ms=round(sorted(x for x, _ in v)[1], 4), min_ms=round(min(x for _, x in v), 4),
                    rounds_ms=[round(x, 4) for x, _ in v]) for k, v in seen.items()}


def scene_points(trks, rng):
    """about PTS_PER_FRAME points per frame inside the (slightly enlarged) predicted box of that frame -> xyz, sample, frame"""
    xyz, sample, frame = [], [], []
    for t, trk in enumerate(trks):
        b = trk.boxes.numpy()
        n = len(b)
        local = (rng.random((n, PTS_PER_FRAME, 3)) - 0.5) * (b[:, None, 3:6] * 1.1)
        c, s = np.cos(b[:, None, 6]), np.sin(b[:, None, 6])
        x = b[:, None, 0] + local[..., 0] * c + local[..., 1] * s
        y = b[:, None, 1] - local[..., 0] * s + local[..., 1] * c
        z = b[:, None, 2] + b[:, None, 5] / 2 + local[..., 2]
        xyz.append(np.stack([x, y, z], -1).reshape(-1, 3))
        sample.append(np.full(n * PTS_PER_FRAME, t))
        frame.append(np.repeat(np.arange(n), PTS_PER_FRAME))
    return (torch.as_tensor(np.concatenate(xyz), dtype=torch.float32).to(DEV), torch.as_tensor(np.concatenate(sample)).to(DEV),
            torch.as_tensor(np.concatenate(frame)).to(DEV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tracklet_bench needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), tracklets=TRACKLETS, frames=FRAMES, candidates=CANDS, points_per_frame=PTS_PER_FRAME,
               feat_cols=F, iters=args.iters)
    trks, cand_lists = T.make_tracklets(5, [FRAMES] * TRACKLETS, [CANDS] * TRACKLETS)
    count_syncs(lambda: None)       # the debug mode's own one-time notice speaks of synchronizing: let it pass before anything is counted

    # 1. the targets
    lt = [lidar(t, str(i)) for i, t in enumerate(trks)]
    lc = [[lidar(c, 'c') for c in cs] for cs in cand_lists]
    dt = [T.Trk(t.boxes.to(DEV), t.ts_list, t.score_list, t.type) for t in trks]
    dc = [[T.Trk(c.boxes.to(DEV), c.ts_list, c.score_list, c.type) for c in cs] for cs in cand_lists]
    train_cfg = dict(CFG, assigner=dict(object_centric=False, iou_thr=0.5))
    fused = lambda: sst_amd.tracklet_targets(lt, lc, train_cfg, device=DEV)                          # noqa: E731
    composed = lambda: T.targets(dt, dc, CFG, torch.float32, iou_fn=sst_amd.aligned_iou_3d)           # noqa: E731
    a, b = fused(), composed()
    same = all(torch.equal(a[k].cpu(), b[k].to(a[k].dtype)) for k in b)
    stats = {}
    T.targets(dt, dc, CFG, torch.float32, iou_fn=sst_amd.aligned_iou_3d, stats=stats)
    case = dict(rows=int(a['rois'].size(0)), candidate_rows=int(a['gts'].size(0)), outputs_equal=bool(same),
                positives=int(a['counts'][:, 0].sum()), fused_host_syncs=count_syncs(fused), composed_host_syncs=count_syncs(composed),
                composed_iou_calls=stats['iou_launches'], composed_reads_in_the_reference=stats['host_reads'])
    for k, v in rounds(dict(fused=fused, composed=composed), args.iters).items():
        case.update({f'{k}_{name}': x for name, x in v.items()})
    case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
    if not args.no_profiler:
        case['fused_launches'] = _bench_common.count_launches(fused, ours='tracklet_')
        case['composed_launches'] = _bench_common.count_launches(composed)
    res['targets'] = case

    # 3. the pool at this shape (its pairs feed the rows below)
    rng = np.random.default_rng(1)
    xyz, sample, frame = scene_points(trks, rng)
    rois, roi_frame = a['rois'].contiguous(), a['frame_inds']
    pool = {}
    for mode, cap in (('train', 300000), ('test', 600000)):
        ext = sst_amd.TrackletPointRoIExtractor(extra_wlh=[0.5, 0.5, 0.5], max_inbox_point=512, max_all_point=cap, debug=False, combined=True)
        run = lambda: ext(xyz, sample, frame, rois, roi_frame)           # noqa: E731
        inds, roi_inds, _ = run()
        ms, low = median_ms(run, args.iters)
        pool[mode] = dict(cap=cap, rois=int(rois.size(0)), points=int(xyz.size(0)), pairs=int(inds.numel()), ms=round(ms, 4),
                          min_ms=round(low, 4), host_syncs=count_syncs(run))
    res['pool'] = pool

    # 2. the rows of the box head, on the pairs of the training cap
    ext = sst_amd.TrackletPointRoIExtractor(extra_wlh=[0.5, 0.5, 0.5], max_inbox_point=512, max_all_point=300000, debug=False, combined=True)
    inds, roi_inds, _ = ext(xyz, sample, frame, rois, roi_frame)
    n, m = int(xyz.size(0)), int(inds.numel())
    feats = torch.randn(n, F, device=DEV).requires_grad_(True)
    scores = a['scores']
    weight = torch.randn(m, F + 2, device=DEV)

    def rows_fused():
        feats.grad = None
        out, _ = sst_amd.tracklet_rows(feats, xyz, frame, inds, roi_inds, roi_frame, scores, combined=True, with_roi_scores=True)
        out.backward(weight)
        return out

    def rows_torch():
        feats.grad = None
        out, _ = T.rows(feats, xyz, frame, inds, roi_inds, roi_frame, scores, True, True)
        out.backward(weight)
        return out

    x = rows_fused()
    g1 = feats.grad.clone()
    y = rows_torch()
    g2 = feats.grad.clone()
    fwd_bytes = m * (4 * F + 16 + 16 + 4 + 12) + m * (4 * (F + 2) + 12)
    bwd_bytes = m * 4 * F + 8 * m + n * 4 * F
    case = dict(rows=m, points=n, forward_equal=bool(torch.equal(x, y)), backward_max_abs_diff=float((g1 - g2).abs().max()),
                repeats_max=int(torch.bincount(inds.clamp(min=0)).max()), algorithmic_bytes=int(fwd_bytes + bwd_bytes),
                fused_host_syncs=count_syncs(rows_fused), torch_host_syncs=count_syncs(rows_torch))
    for k, v in rounds(dict(fused=rows_fused, torch=rows_torch), args.iters).items():
        case.update({f'{k}_{name}': x for name, x in v.items()})
    case['torch_over_fused'] = round(case['torch_ms'] / case['fused_ms'], 2)
    case['fused_gbytes_per_s'] = round(case['algorithmic_bytes'] / (case['fused_ms'] * 1e-3) / 1e9, 1)
    case['fused_fraction_of_hbm'] = round(case['algorithmic_bytes'] / (case['fused_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
    if not args.no_profiler:
        case['fused_launches'] = _bench_common.count_launches(rows_fused, ours='tracklet_')
        case['torch_launches'] = _bench_common.count_launches(rows_torch)
    res['rows'] = case
    res['requirements'] = dict(fused_targets_read_nothing_back=res['targets']['fused_host_syncs'] == 0,
                               targets_not_slower=res['targets']['fused_ms'] <= res['targets']['composed_ms'],
                               rows_not_slower=res['rows']['fused_ms'] <= res['rows']['torch_ms'])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
