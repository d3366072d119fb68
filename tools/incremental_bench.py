"""Times the FSD++ incremental point stage at the shipped shape - 2 samples x 7 frames x about 160 000 points, about 100 seed
boxes per previous frame, incremental_cfg of configs/fsdpp/fsdpp_waymoD1_1x_7f_6base.py - with device events after warm-up (the
median of --iters separately timed calls, three alternating rounds), the fused stage against its restatement with torch ops
(tests/incremental_ref.py: the reference's loop over samples and frames) on the same device and in the same process.  Prints one
JSON object.

    python tools/incremental_bench.py [--iters 10] [--out profiles/incremental/incremental_bench.json] [--no-profiler]

1. training: sst_amd.generate_points (packing, the one host-to-device copy, the launches, the one host read) against
   incremental_ref.generate_points with the same keys; outputs compared bit for bit; kernel launches, copies (torch.profiler) and
   host synchronisations (torch.cuda.set_sync_debug_mode('warn'), warnings counted) on each side; the bytes the stage must move
   (20 B read per point and pass, 24 B written per kept row; the bitmaps stay in L2) over the measured time as a fraction of 8 TB/s.
2. sequential: one frame of the test path - six previous clouds and six previous crops moved into the current frame, the delta
   points of the current frame and of frame -1 (the list form v3), the crop of the current frame by 100 boxes - the library's
   calls against the restatement's."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import _bench_common  # noqa: E402
from _bench_common import median_ms  # noqa: E402
from fg_sample_bench import count_syncs  # noqa: E402
import incremental_ref as R  # noqa: E402
from sst_amd import incremental as I  # noqa: E402

DEV = 'cuda:0'
SAMPLES, FRAMES, POINTS, BOXES = 2, 7, 160000, 100
HBM_BYTES_PER_S = 8e12
CFG = dict(voxel_size=(0.25, 0.25, 0.4), point_cloud_range=[-80, -80, -2, 80, 80, 4], center_noise=0.0, dim_noise=0.0, yaw_noise=0.0,
           extra_width=1.0, num_previous_frames=6, crop_frames=6, max_crop_points=128, crop_shuffle=True, max_age=1, num_base_frame=5)


def rounds(paths, iters):
    """three alternating rounds (other work shares the machine) -> per path (middle median, minimum, the three medians)"""
    seen = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():
            seen[k].append(median_ms(fn, iters))
    return {k: dict(ms=round(sorted(x for x, _ in v)[1], 4), min_ms=round(min(x for _, x in v), 4),
                    rounds_ms=[round(x, 4) for x, _ in v]) for k, v in seen.items()}


def frame(g, shift):
    """a sweep-like cloud: a ground disc, denser near the sensor, and clumps where the boxes are; moved by ``shift`` along x"""
    r = 75.0 * np.sqrt(g.uniform(0, 1, POINTS)) ** 1.5
    phi = g.uniform(0, 2 * np.pi, POINTS)
    xyz = np.stack([r * np.cos(phi) + shift, r * np.sin(phi), g.normal(-1.6, 0.05, POINTS)], 1)
    tall = g.uniform(0, 1, POINTS) < 0.3
    xyz[tall, 2] = g.uniform(-1.6, 2.5, int(tall.sum()))
    return np.concatenate([xyz, g.uniform(0, 1, (POINTS, 2))], 1).astype(np.float32)


def seeds_for(cloud, g):
    c = cloud[g.integers(0, len(cloud), BOXES), :3]
    b = np.concatenate([c[:, :2], np.full((BOXES, 1), -1.8), g.uniform(1.5, 5.0, (BOXES, 2)), g.uniform(1.5, 2.0, (BOXES, 1)),
                        g.uniform(-3, 3, (BOXES, 1))], 1)
    return dict(gt_bboxes_3d=b.astype(np.float32), gt_labels_3d=g.integers(0, 3, BOXES), scores=g.uniform(0, 1, BOXES).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'incremental_bench needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), samples=SAMPLES, frames=FRAMES, points_per_frame=POINTS, boxes_per_frame=BOXES,
               iters=args.iters, incremental_cfg={k: v for k, v in CFG.items()})
    g = np.random.default_rng(0)
    count_syncs(lambda: None)
    pts, finds, seeds, per_frame = [], [], [], []
    for s in range(SAMPLES):
        clouds = [frame(g, 0.5 * k) for k in range(FRAMES)]
        per_frame.append(clouds)
        pts.append(torch.from_numpy(np.concatenate(clouds, 0)).to(DEV))
        finds.append(torch.arange(FRAMES).repeat_interleave(POINTS).neg().long().to(DEV))
        seeds.append([seeds_for(clouds[k + 1], g) for k in range(6)])
    total = sum(len(p) for p in pts)
    keys = torch.randint(0, 2 ** 32, (total,), dtype=torch.int64, device=DEV)
    per_sample = [keys[:len(pts[0])], keys[len(pts[0]):]]

    # 1. the training batch
    fused = lambda: I.generate_points(pts, finds, seeds, CFG, True, keys=keys)                # noqa: E731
    composed = lambda: R.generate_points(pts, finds, seeds, CFG, keys=per_sample)              # noqa: E731
    a, b = fused(), composed()
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[0], b[0])) and a[1] == b[1]
    rows = sum(len(x) for x in a[0])
    again = fused()
    must_move = total * 20 * 3 + rows * 24          # the points are read by the mark, count and rows launches
    case = dict(points=total, rows=rows, num_delta_points=a[1], outputs_equal=bool(same),
                two_runs_equal=all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[0], again[0])),
                bitmap_bytes_per_sample_and_query=int(np.prod(I.spatial_size(CFG['voxel_size'], CFG['point_cloud_range'])) + 31) // 32 * 4,
                bytes_the_stage_must_move=int(must_move), fused_host_syncs=count_syncs(fused), composed_host_syncs=count_syncs(composed))
    for k, v in rounds(dict(fused=fused, composed=composed), args.iters).items():
        case.update({f'{k}_{name}': x for name, x in v.items()})
    case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
    case['fused_gbytes_per_s'] = round(must_move / (case['fused_ms'] * 1e-3) / 1e9, 1)
    case['fused_fraction_of_hbm'] = round(must_move / (case['fused_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
    if not args.no_profiler:
        case['fused_launches'] = _bench_common.count_launches(fused, ours='incr_')
        case['composed_launches'] = _bench_common.count_launches(composed)
    res['training'] = case

    # 2. one frame of the sequential path
    clouds = [torch.from_numpy(c).to(DEV) for c in per_frame[0]]
    cur, pre = clouds[0], clouds[1:]
    crops = [c[:4000].contiguous() for c in pre]
    mats = []
    for k in range(6):
        yaw = 0.01 * (k + 1)
        m = np.eye(4, dtype=np.float32)
        m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        m[:3, 3] = [0.5 * (k + 1), 0.02 * k, 0.0]
        mats.append(m)
    boxes = R.enlarged(torch.from_numpy(seeds[0][0]['gt_bboxes_3d']).to(DEV), 1.0)
    vs, rng = CFG['voxel_size'], CFG['point_cloud_range']

    def seq_fused():
        moved = I.transform_clouds(pre + crops, mats + mats)
        base = list(moved[:6])[-5:]
        d0 = F.pad(I.find_delta_points_by_voxelization_list_v3(base, cur, vs, rng), (0, 1), 'constant', 0)
        d1 = F.pad(I.find_delta_points_by_voxelization_list_v3(base[:-1], base[-1], vs, rng), (0, 1), 'constant', -0.1)
        crop = I.seed_crop(cur, boxes, 128, keys[:len(cur)])
        return d0, d1, crop, moved

    def seq_composed():
        moved = [R.frame_transform(c, m) for c, m in zip(pre + crops, mats + mats)]
        base = moved[:6][-5:]
        d0 = F.pad(R.find_delta_points_by_voxelization_list_v3(base, cur, vs, rng), (0, 1), 'constant', 0)
        d1 = F.pad(R.find_delta_points_by_voxelization_list_v3(base[:-1], base[-1], vs, rng), (0, 1), 'constant', -0.1)
        crop = cur[R.crop_indices(cur, boxes, 128, keys[:len(cur)])]
        return d0, d1, crop, moved

    x, y = seq_fused(), seq_composed()
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x[:3], y[:3])) \
        and all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x[3], y[3]))
    case = dict(points_per_cloud=POINTS, delta_rows=int(len(x[0]) + len(x[1])), crop_rows=int(len(x[2])), outputs_equal=bool(same),
                fused_host_syncs=count_syncs(seq_fused), composed_host_syncs=count_syncs(seq_composed))
    for k, v in rounds(dict(fused=seq_fused, composed=seq_composed), args.iters).items():
        case.update({f'{k}_{name}': x for name, x in v.items()})
    case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
    if not args.no_profiler:
        case['fused_launches'] = _bench_common.count_launches(seq_fused, ours='_k')
        case['composed_launches'] = _bench_common.count_launches(seq_composed)
    res['sequential'] = case
    res['requirements'] = dict(training_not_slower=res['training']['fused_ms'] <= res['training']['composed_ms'],
                               sequential_not_slower=res['sequential']['fused_ms'] <= res['sequential']['composed_ms'],
                               training_one_host_read=res['training']['fused_host_syncs'] <= 1,
                               outputs_equal=res['training']['outputs_equal'] and res['sequential']['outputs_equal'])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
