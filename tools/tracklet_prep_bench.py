"""Times CTRL's offline stage (sst_amd.tracklet_prep, csrc/tracklet_prep.hip) at the shape of one Waymo segment.  Prints one JSON object.

    python tools/tracklet_prep_bench.py [--iters 5] [--out profiles/tracklet_prep/tracklet_prep_bench.json]

  affinity   300 predicted x 150 ground-truth tracklets of one segment, 100 frames each out of 200 (45 000 pairs):
             fused    sst_amd.tracklet_affinity - one packed copy, one launch, one read
             by_hand  the reference's loop (generate_candidates.py:61-62) on the parent's ops: per pair the Python set intersection, two
                      index copies, sst_amd.aligned_iou_3d and .max().item() (LiDARTracklet.intersection_ious).  Timed on the first
                      --hand-fraction of the predicted tracklets (default 0.1) and scaled to all of them; says so in the result.
  crops      20 frames of 180 000 points (6 columns) x 200 boxes:
             fused    sst_amd.box_point_crops (count, scan, one read of the total, fill) and box_point_counts (the count alone)
             by_hand  the reference's loop (generate_track_input.py:93-101) on the parent's ops: per box points_in_boxes_gpu on the
                      whole cloud, a mask, an index and a copy to the host - all 4 000 boxes
Every time is a host clock around work that ends in a host read or a device synchronise: the median of --iters calls after a warm-up."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sst_amd  # noqa: E402

DEV = 'cuda:0'
TS0 = 1_550_000_000_000_000
N_PD, N_GT, LEN, SPAN = 300, 150, 100, 200
FRAMES, POINTS, BOXES, COLS = 20, 180_000, 200, 6


def median_ms(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times]


def segment(rng):
    """150 objects on gently turning paths over 200 frames; a ground-truth tracklet per object and two predicted ones"""
    yaw = rng.uniform(-np.pi, np.pi, (N_GT, 1)) + np.cumsum(rng.normal(0, 0.01, (N_GT, SPAN)), 1)
    step = rng.uniform(0.0, 0.6, (N_GT, 1))
    xy = rng.uniform(-70, 70, (N_GT, 1, 2)) + np.cumsum(np.stack([np.sin(yaw), np.cos(yaw)], 2) * step[..., None], 1)
    size = np.tile(np.array([2.0, 4.6, 1.7]), (N_GT, SPAN, 1)) * (1 + rng.normal(0, 0.02, (N_GT, 1, 3)))
    paths = np.concatenate([xy, np.full((N_GT, SPAN, 1), -1.0), size, yaw[..., None]], 2).astype(np.float32)

    def trk(k, name, noise):
        s = int(rng.integers(0, SPAN - LEN + 1))
        b = paths[k, s:s + LEN] + (rng.normal(0, 1, (LEN, 7)) * np.array([0.2, 0.2, 0.05, 0.05, 0.1, 0.05, 0.05]) * noise).astype(np.float32)
        t = sst_amd.LiDARTracklet('seg', name, 1, True, torch.as_tensor(b), [TS0 + 100_000 * (s + i) for i in range(LEN)], [0.5] * LEN)
        t.freeze()
        return t

    gts = [trk(k, f'g{k}', 0.0) for k in range(N_GT)]
    pds = [trk(k % N_GT, f'p{k}', 1.0) for k in range(N_PD)]
    return pds, gts


def frames_of(rng):
    points_list, boxes_list = [], []
    for _ in range(FRAMES):
        yaw = rng.uniform(-np.pi, np.pi, BOXES)
        boxes = np.stack([rng.uniform(-70, 70, BOXES), rng.uniform(-70, 70, BOXES), np.full(BOXES, -1.0), np.full(BOXES, 2.0),
                          np.full(BOXES, 4.6), np.full(BOXES, 1.7), yaw], 1).astype(np.float32)
        pts = rng.uniform(-1, 1, (POINTS, COLS)).astype(np.float32) * np.array([75, 75, 2, 1, 1, 1], np.float32)
        k = rng.integers(0, BOXES, POINTS // 4)                     # a quarter of the cloud lies on the objects
        pts[: len(k), :3] = boxes[k, :3] + rng.uniform(-1, 1, (len(k), 3)).astype(np.float32) * np.array([2.5, 2.5, 1.0], np.float32) \
            + np.array([0, 0, 0.85], np.float32)
        points_list.append(torch.as_tensor(pts).to(DEV))
        boxes_list.append(torch.as_tensor(boxes).to(DEV))
    return points_list, boxes_list


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--hand-fraction', type=float, default=0.1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tracklet_prep_bench needs a GPU')
    torch.set_num_threads(16)
    rng = np.random.default_rng(0)
    result = dict(device=torch.cuda.get_device_name(0), iters=args.iters)

    # ---- affinity
    pds, gts = segment(rng)
    fused = {}

    def run_fused():
        fused['out'] = sst_amd.tracklet_affinity(pds, gts, device=DEV)
    ms, all_ms = median_ms(run_fused, args.iters)
    n_hand = max(1, int(round(N_PD * args.hand_fraction)))
    for t in pds[:n_hand] + gts:
        t.to(DEV)
    hand = {}

    def run_hand():
        hand['out'] = [[(lambda v: float(v.max().item()) if v.numel() else 0.0)(p.intersection_ious(g)) for g in gts] for p in pds[:n_hand]]
    run_hand()                                                          # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_hand()
    hand_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(np.asarray(h, np.float32), f[1]) for h, f in zip(hand['out'], fused['out']))
    aff = np.stack([a for _, a in fused['out']])
    result['affinity'] = dict(
        shape=dict(predicted=N_PD, ground_truth=N_GT, frames=LEN, pairs=N_PD * N_GT, pairs_with_shared_frames=int(sum(
            bool(set(p.ts_list) & set(g.ts_list)) for p in pds for g in gts)), pairs_above_0p5=int((aff > 0.5).sum())),
        fused_ms=round(ms, 3), fused_all_ms=all_ms,
        by_hand_fraction=n_hand / N_PD, by_hand_measured_ms=round(hand_ms, 1), by_hand_scaled_ms=round(hand_ms * N_PD / n_hand, 1),
        by_hand_per_pair_ms=round(hand_ms / (n_hand * N_GT), 4), speedup_scaled=round(hand_ms * N_PD / n_hand / ms, 1), bit_equal=bool(same))

    # ---- crops
    points_list, boxes_list = frames_of(rng)
    got = {}

    def run_crops():
        got['out'] = sst_amd.box_point_crops(points_list, boxes_list)

    def run_counts():
        got['counts'] = sst_amd.box_point_counts(points_list, boxes_list).cpu()
    crops_ms, crops_all = median_ms(run_crops, args.iters)
    counts_ms, counts_all = median_ms(run_counts, args.iters)

    def run_by_hand():
        out = []
        for pc, boxes in zip(points_list, boxes_list):
            xyz = pc[:, :3].contiguous()
            for b in range(boxes.size(0)):
                inds = sst_amd.points_in_boxes_gpu(xyz[None], boxes[b:b + 1][None])[0]
                out.append(pc[inds == 0].cpu().numpy())
        return out
    run_by_hand()                                                       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hand_crops = run_by_hand()
    hand_crops_ms = (time.perf_counter() - t0) * 1e3
    rows, src, counts, offsets = got['out']
    same = np.array_equal(np.concatenate(hand_crops), rows.cpu().numpy()) and [len(p) for p in hand_crops] == counts.cpu().tolist()
    n_rows = int(rows.size(0))
    # algorithmic bytes: xyz of every point read by the count and the fill, the boxes, the cell matrix written, scanned and read, the rows
    cells = FRAMES * BOXES * -(-POINTS // sst_amd._lib.load().sst_box_crops_tile())
    algo = 2 * FRAMES * POINTS * 12 + 2 * FRAMES * BOXES * 28 + 4 * cells * 4 + n_rows * (2 * COLS * 4 + 8)
    result['crops'] = dict(
        shape=dict(frames=FRAMES, points=POINTS, boxes=BOXES, cols=COLS, rows_out=n_rows, cells=cells, algorithmic_bytes=algo),
        fused_ms=round(crops_ms, 3), fused_all_ms=crops_all, count_only_ms=round(counts_ms, 3), count_only_all_ms=counts_all,
        by_hand_ms=round(hand_crops_ms, 1), by_hand_per_box_ms=round(hand_crops_ms / (FRAMES * BOXES), 4),
        speedup=round(hand_crops_ms / crops_ms, 1), equal=bool(same), algorithmic_gb_s=round(algo / crops_ms / 1e6, 1))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
