"""Times the CTRL test-time augmentation (sst_amd.tracklet_tta, csrc/tracklet_tta.hip) at the shape of an inference batch of the
shipped configs: samples_per_gpu = 8 tracklets whose lengths are spread over 20 .. 200 frames, the loader's cap of 1 024 points
per frame (a uniform 1 .. 1 024), C = 5, D = 5, the four views of the shipped ``tta_pipeline`` (double flip), merge 'weighted', the
model of configs/ctrl/ctrl_veh_24e.py.  Prints one JSON object.

    python tools/tracklet_tta_bench.py [--iters 5] [--out profiles/tracklet_tta/tracklet_tta_bench.json]

  parent   what a user can do without this module: per view one call of the device test_pipeline (TrackletAugment), the flips and
           the rotation of points and boxes as torch device ops, the modules of simple_test, the inverse as torch device ops and
           LiDARTracklet.update_from_prediction per tracklet; then the host numpy merge (tests/tracklet_tta_ref.merge); view k
           shuffles with the seed the fused path gives it, so both paths feed the network the same rows in the same order
  fused    the new path: TrackletTTA.__call__ (front), tta_network (once per view: the default), tta_finish and the one host read
  fused_single_pass   the same with tta_single_pass (one network pass over the K * B samples; not bit-equal, see the module)
Each part (front, network, finish) is timed on a host clock around work that ends in a device synchronise, the median of --iters
calls in three alternating rounds; ``host_ms`` is the same part's time until its last launch returns (no synchronise), ``launches``
the device-side kernels, memsets and copies of one call (torch.profiler, a run of its own)."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _bench_common import count_launches  # noqa: E402
import sst_amd  # noqa: E402
from sst_amd.tracklet_augment import TrackletAugment, TrackletParams  # noqa: E402
from sst_amd.tracklet_detector import get_bboxes_from_tracklet  # noqa: E402
from sst_amd.tracklet_tta import VIEW_SEED, attach_tracklet_tta, tta_finish  # noqa: E402

DEV = 'cuda:0'
BATCH, MAX_POINTS, COLS = 8, 1024, 5
LENGTHS = [20, 46, 72, 98, 124, 150, 176, 200]
FIXTURES = os.path.join(ROOT, 'tests', 'golden', 'configs')


def sample(g, t, n):
    """one tracklet of a car 20 to 60 m from the ego vehicle, its poses and the points of every frame"""
    yaw = g.uniform(-np.pi, np.pi) + np.cumsum(g.normal(0, 0.01, n))
    xy = g.uniform(-60, 60, 2) + np.cumsum(np.stack([np.sin(yaw), np.cos(yaw)], 1) * 0.3, 0)
    boxes = np.concatenate([xy, np.full((n, 1), -0.5), np.tile([2.0, 4.6, 1.7], (n, 1)), yaw[:, None]], 1).astype(np.float32)
    poses = []
    for k in range(n):
        a = 0.7 + 0.003 * k
        m = np.eye(4, dtype=np.float32)
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = [1.0e4 + 100 * t + 0.9 * k, -2.0e4 + 0.5 * k, 30.0]
        poses.append(m)
    lens = g.randint(1, MAX_POINTS + 1, n)
    pts = np.zeros((int(lens.sum()), COLS), np.float32)
    of = np.repeat(np.arange(n), lens)
    pts[:, :3] = boxes[of, :3] + g.uniform(-1, 1, (len(of), 3)) * [3.0, 3.0, 1.0]
    pts[:, 3:] = g.uniform(0, 1, (len(of), COLS - 3))
    return dict(boxes=boxes, ts=[1_550_000_000_000_000 + 100_000 * k for k in range(n)], poses=poses,
                scores=g.uniform(0.1, 0.9, n).astype(np.float32).tolist(), lens=lens, points=pts)


def tracklets_of(samples):
    trks = []
    for t, s in enumerate(samples):
        trk = sst_amd.LiDARTracklet('seg', f'p{t}', 0, True, torch.as_tensor(s['boxes']), s['ts'], list(s['scores']))
        trk.freeze()
        trk.set_type(0, 'mmdet3d')
        trk.pose_list = [torch.as_tensor(p) for p in s['poses']]
        trks.append(trk)
    return trks


def flip_rotate(x, view, inverse=False):
    """the view's transform (or its inverse) of points [N, >= 3] or boxes [n, 7] on the device, as torch ops"""
    h, v, angle = view
    is_box = x.size(1) == 7

    def rot(a):
        c, s = float(np.cos(np.float32(a))), float(np.sin(np.float32(a)))
        x[:, :2] = x[:, :2] @ x.new_tensor([[c, -s], [s, c]])
        if is_box:
            x[:, 6] += a

    def flips():
        if h:
            x[:, 1] = -x[:, 1]
            if is_box:
                x[:, 6] = -x[:, 6] + np.pi
        if v:
            x[:, 0] = -x[:, 0]
            if is_box:
                x[:, 6] = -x[:, 6]

    if inverse:
        flips()
        rot(-angle)
    else:
        rot(angle)
        flips()
    return x


class Clock(object):
    """per part: the time until its last launch returned and the time until the device finished"""

    def __init__(self):
        self.parts = {}

    def part(self, name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        p = self.parts.setdefault(name, dict(host=0.0, total=0.0))
        p['host'] += (t1 - t0) * 1e3
        p['total'] += (t2 - t0) * 1e3
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tracklet_tta_bench needs a GPU')
    import tracklet_tta_ref as R
    torch.set_num_threads(16)
    g = np.random.RandomState(0)
    samples = [sample(g, t, n) for t, n in enumerate(LENGTHS)]
    host_in = [(s['points'], s['lens']) for s in samples]
    pipes = eval(open(os.path.join(FIXTURES, 'pipeline', 'ctrl', 'ctrl_veh_24e.pipeline.py')).read())
    tta_pipeline = eval(open(os.path.join(FIXTURES, 'pipeline', 'ctrl', 'ctrl_veh_24e.tta_pipeline.py')).read())['tta_pipeline']
    model = eval(open(os.path.join(FIXTURES, 'ctrl', 'ctrl_veh_24e.model.py')).read())
    torch.manual_seed(0)
    plain = sst_amd.build_detector(model).to(DEV).eval()
    det = attach_tracklet_tta(copy.deepcopy(plain), dict(merge='weighted'), tta_pipeline)
    aug = TrackletAugment.from_pipeline(pipes['test_pipeline'])
    views = det.tta.views
    K = len(views)
    trks0 = tracklets_of(samples)
    seeds = list(range(1, BATCH + 1))
    n_rows = sum(LENGTHS)

    def parent(clock):
        per_view_boxes, per_view_scores = [], []
        head = plain.roi_head
        for k, view in enumerate(views):
            trks = copy.deepcopy(trks0)

            def front():
                p = TrackletParams(BATCH)
                with np.errstate(over='ignore'):                       # the seeds the fused path gives view k: the same rows, the same order
                    p.seed[:] = np.asarray(seeds, np.uint64) + np.uint64(VIEW_SEED) * np.uint64(k)
                res = aug(host_in, trks, None, p)
                flip_rotate(res['points_packed'], view)
                for t in trks:
                    flip_rotate(t.boxes, view)
                return res
            res = clock.part('front', front)

            def network():
                with torch.no_grad():
                    pts = plain.fake_points_for_empty_input(res['points'])
                    inds = plain.fake_points_for_empty_input([f.long() for f in res['pts_frame_inds']])
                    plain.tracklet_to_device(trks, None, pts[0].device)
                    seg = plain.segmentor.forward_train(points=pts, pts_frame_inds=inds, img_metas=None)
                    rois, roi_frame_inds, cls_preds, labels_3d = head.tracklets2rois(trks)
                    out = head._bbox_forward(seg['seg_points'][:, :3], seg['seg_feats'], seg['batch_idx'], seg['pts_frame_inds'], rois,
                                             cls_preds, roi_frame_inds)
                    return get_bboxes_from_tracklet(rois, out['cls_score'], out['bbox_pred'], out['valid_roi_mask'], labels_3d, cls_preds,
                                                    None, cfg=head.test_cfg, batch_size=BATCH)
            decoded = clock.part('network', network)

            def finish():
                for trk, (boxes, scores, labels, valid) in zip(trks, decoded):
                    flip_rotate(trk.boxes, view, inverse=True)
                    trk.update_from_prediction(flip_rotate(boxes.clone(), view, inverse=True), scores, labels, valid)
                per_view_boxes.append(np.concatenate([t.boxes.numpy() for t in trks]))
                per_view_scores.append(np.array([s for t in trks for s in t.score_list], np.float64))
            clock.part('finish', finish)
        return clock.part('finish', lambda: R.merge(np.stack(per_view_boxes), np.stack(per_view_scores), 'weighted'))

    def fused(clock):
        trks = copy.deepcopy(trks0)
        v = clock.part('front', lambda: det.tta(host_in, trks, seeds=seeds))
        boxes, scores, valid = clock.part('network', lambda: det.tta_network(v))

        def finish():
            out = tta_finish(boxes, scores, valid, v['old_boxes'], v['old_scores'], v['ego_mats'], views, 'weighted', return_views=False)
            merged = out['merged'].cpu()
            return merged[:7 * n_rows].view(n_rows, 7).numpy(), merged[7 * n_rows:].numpy()
        return clock.part('finish', finish)

    def fused_single(clock):
        det.tta_single_pass = True
        try:
            return fused(clock)
        finally:
            det.tta_single_pass = False

    paths = dict(parent=parent, fused=fused, fused_single_pass=fused_single)
    results = {}
    for name, fn in paths.items():                                     # warm-up: every shape, every kernel class
        results[name] = fn(Clock())
    rounds = {k: [] for k in paths}
    for _ in range(3):                                                 # alternating rounds: other work shares the machine
        for name, fn in paths.items():
            clock = Clock()
            for _ in range(args.iters):
                fn(clock)
            rounds[name].append({p: {k: v / args.iters for k, v in t.items()} for p, t in clock.parts.items()})
    entry = {}
    for name, rs in rounds.items():
        e = {}
        for part in ('front', 'network', 'finish'):
            totals = sorted(r[part]['total'] for r in rs)
            hosts = sorted(r[part]['host'] for r in rs)
            e[part] = dict(ms=round(totals[1], 3), rounds_ms=[round(r[part]['total'], 3) for r in rs], host_ms=round(hosts[1], 3))
        e['total_ms'] = round(sum(e[p]['ms'] for p in ('front', 'network', 'finish')), 3)
        entry[name] = e
    # launches, in a run of its own
    for name, fn in paths.items():
        entry[name]['launches'] = count_launches(lambda: fn(Clock()))
    trks = copy.deepcopy(trks0)
    v = det.tta(host_in, trks, seeds=seeds)
    entry['fused']['launches_front'] = count_launches(lambda: det.tta(host_in, copy.deepcopy(trks0), seeds=seeds), ours='tta_')
    b, s, m = det.tta_network(v)
    entry['fused']['launches_finish'] = count_launches(
        lambda: tta_finish(b, s, m, v['old_boxes'], v['old_scores'], v['ego_mats'], views, 'weighted', return_views=False)['merged'].cpu(),
        ours='tta_')
    # the two orders of rounding against each other, and against the parent path
    pb, ps, _ = results['parent']
    fb, fs = results['fused']
    sb, ss = results['fused_single_pass']
    entry['agreement'] = dict(fused_vs_parent_boxes=float(np.abs(fb - pb).max()), fused_vs_parent_scores=float(np.abs(fs - ps).max()),
                              single_pass_vs_fused_boxes=float(np.abs(sb - fb).max()), single_pass_vs_fused_scores=float(np.abs(ss - fs).max()))
    rows_in = int(sum(s['lens'].sum() for s in samples))
    result = dict(shape=dict(batch=BATCH, lengths=LENGTHS, max_points=MAX_POINTS, cols=COLS, deco=5, views=K, rows_in=rows_in,
                             rows_out=int(v['offsets'][-1]), tracklet_rows=n_rows),
                  device=torch.cuda.get_device_name(0), iters=args.iters, threads=torch.get_num_threads(), batch8=entry)
    for part in ('front', 'network', 'finish'):
        entry[f'speedup_{part}_fused_over_parent'] = round(entry['parent'][part]['ms'] / entry['fused'][part]['ms'], 3)
    entry['speedup_total_fused_over_parent'] = round(entry['parent']['total_ms'] / entry['fused']['total_ms'], 3)
    entry['speedup_total_single_pass_over_parent'] = round(entry['parent']['total_ms'] / entry['fused_single_pass']['total_ms'], 3)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
