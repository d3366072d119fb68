"""Times the device-side CTRL tracklet pipeline (sst_amd.tracklet_augment.TrackletAugment, csrc/tracklet_augment.hip) at the shape
of a training batch of the shipped configs - samples_per_gpu = 16 tracklets of 100 frames with up to 1 024 points each (a uniform
1 .. 1 024 per frame), C = 5, D = 5, two candidates per tracklet, shuffle on - with device events after warm-up (the median of
--iters separately timed calls, three alternating rounds).  Prints one JSON object.

    python tools/tracklet_augment_bench.py [--iters 20] [--out profiles/tracklet_augment/tracklet_augment_bench.json]

  kernels_host_in   the whole call from host arrays: the per-box host work, packing, the one host-to-device copy, the launches,
                    the one host read
  kernels_dev_in    the same from device tensors (one concatenated tensor per sample, packed by device copies)
  torch_device      the same steps as plain torch device ops, frame by frame as the reference writes them (pad, matrix product,
                    cat per frame; flip, rotation, scale, translation, range, randperm per sample), inputs on the device
  restatement_host  tests/tracklet_augment_ref.py (numpy) over the samples on 16 host threads
and, for the kernel paths, the host time of a call split into its parts (a host clock; the call ends in the read of the counts),
the device time of each kernel (torch.profiler, a run of its own) and the algorithmic bytes - 4C read per input row, 4(C + D) + 4
written per survivor - over the call's time and over the sum of its launches' device time, as fractions of 8 TB/s."""
import argparse
import copy
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _bench_common import median_ms  # noqa: E402
import sst_amd  # noqa: E402
from sst_amd.tracklet_augment import TrackletAugment  # noqa: E402

DEV = 'cuda:0'
BATCH, FRAMES, MAX_POINTS, COLS, DECO, CANDS = 16, 100, 1024, 5, 5, 2
RANGE = [-204.7, -204.7, -3.99, 204.7, 204.7, 7.99]
HBM_BYTES_PER_S = 8e12
PIPELINE = [dict(type='LoadTrackletPoints', load_dim=6, use_dim=5, max_points=1024), dict(type='LoadTrackletAnnotations'),
            dict(type='TrackletCutting', ratio=0.0, max_length=150), dict(type='TrackletPoseTransform', concat=False),
            dict(type='TrackletNoise', center_noise_cfg=dict(max_noise=[0.2, 0.2, 0.1], consistent=False),
                 size_noise_cfg=dict(max_noise=[0.2, 0.2, 0.1], consistent=False), yaw_noise_cfg=dict(max_noise=0.2, consistent=False)),
            dict(type='PointDecoration', properties=['yaw', 'size', 'score'], concat=True),
            dict(type='TrackletRandomFlip', flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
            dict(type='TrackletGlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
                 translation_std=[0, 0, 0.2]),
            dict(type='PointsRangeFilter', point_cloud_range=RANGE), dict(type='PointShuffle')]


def sample(g, t):
    """one tracklet of a car 20 to 60 m from the ego vehicle, its poses, two candidates and the points of every frame"""
    n = FRAMES
    yaw = g.uniform(-np.pi, np.pi) + np.cumsum(g.normal(0, 0.01, n))
    xy = g.uniform(-60, 60, 2) + np.cumsum(np.stack([np.sin(yaw), np.cos(yaw)], 1) * 0.3, 0)
    boxes = np.concatenate([xy, np.full((n, 1), -0.5), np.tile([2.0, 4.6, 1.7], (n, 1)), yaw[:, None]], 1).astype(np.float32)
    ts = [1_550_000_000_000_000 + 100_000 * k for k in range(n)]
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
    return dict(boxes=boxes, ts=ts, poses=poses, scores=g.uniform(0.1, 0.9, n).astype(np.float32).tolist(), lens=lens, points=pts)


def tracklets_of(samples):
    trks, cands = [], []
    for t, s in enumerate(samples):
        trk = sst_amd.LiDARTracklet('seg', f'p{t}', 0, True, torch.as_tensor(s['boxes']), s['ts'], s['scores'])
        trk.freeze()
        trk.pose_list = [torch.as_tensor(p) for p in s['poses']]
        cl = []
        for c in range(CANDS):
            keep = list(range(c, FRAMES, 1 + c))
            g = sst_amd.LiDARTracklet('seg', f'g{t}_{c}', 0, True, torch.as_tensor(s['boxes'][keep] + 0.05 * c), [s['ts'][i] for i in keep],
                                      [1.0] * len(keep))
            g.freeze()
            g.pose_list = [trk.pose_list[i] for i in keep]
            cl.append(g)
        trks.append(trk)
        cands.append(cl)
    return trks, cands


def torch_pipeline(s, mm, deco, rec, dev):
    """the reference's steps with plain torch ops on ``dev``: per frame pad, ``@ mm.T``, the appended columns, cat; per sample
    flips, rotation, scale, translation, the range, randperm.  ``mm`` [n, 4, 4], ``deco`` [n, D] on ``dev``"""
    frames = torch.split(s['points_' + dev.type], s['lens'].tolist())
    out, inds = [], []
    for k, p in enumerate(frames):
        xyz = (torch.nn.functional.pad(p[:, :3], (0, 1), 'constant', 1) @ mm[k].T)[:, :3]
        out.append(torch.cat([xyz, p[:, 3:], deco[k][None].expand(len(p), -1)], 1))
        inds.append(torch.full((len(p),), k, dtype=torch.int32, device=dev))
    pts, inds = torch.cat(out, 0), torch.cat(inds, 0)
    if rec['flip_h']:
        pts[:, 1] = -pts[:, 1]
    if rec['flip_v']:
        pts[:, 0] = -pts[:, 0]
    c, sn = float(rec['cos']), float(rec['sin'])
    pts[:, :3] = pts[:, :3] @ torch.tensor([[c, -sn, 0], [sn, c, 0], [0, 0, 1]], dtype=torch.float32, device=dev)
    pts[:, :3] *= float(rec['scale'])
    pts[:, :3] += torch.tensor(rec['trans'], device=dev)
    r = RANGE
    keep = ((pts[:, 0] > r[0]) & (pts[:, 1] > r[1]) & (pts[:, 2] > r[2]) & (pts[:, 0] < r[3]) & (pts[:, 1] < r[4]) & (pts[:, 2] < r[5]))
    pts, inds = pts[keep], inds[keep]
    order = torch.randperm(pts.size(0), device=dev)
    return pts[order], inds[order]


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
        raise SystemExit('tracklet_augment_bench needs a GPU')
    import tracklet_augment_ref as R
    dev = torch.device(DEV)
    torch.set_num_threads(16)
    g = np.random.RandomState(0)
    samples = [sample(g, t) for t in range(BATCH)]
    for s in samples:
        s['points_cuda'] = torch.from_numpy(s['points']).to(dev)
    aug = TrackletAugment.from_pipeline(PIPELINE)
    trks0, cands0 = tracklets_of(samples)
    params = aug.draw_params(trks0, np.random.RandomState(1), torch.Generator().manual_seed(1))
    rec = aug.records(params)
    per_sample, _, _ = aug.prepare_boxes(copy.deepcopy(trks0), copy.deepcopy(cands0), params)     # copies: the call's own tracklets stay as loaded
    mats_dev = [ps[0].to(dev) for ps in per_sample]
    deco_dev = [ps[1].to(dev) for ps in per_sample]
    host_in = [(s['points'], s['lens']) for s in samples]
    dev_in = [(s['points_cuda'], s['lens']) for s in samples]

    members = [m for t, cl in zip(trks0, cands0) for m in [t] + cl]
    saved = [m.boxes for m in members]

    def fresh():
        """a call moves the boxes of its tracklets to the shared pose and to the device: put the loader's state back (no copy)"""
        for m, b in zip(members, saved):
            m.boxes, m.shared_pose = b, None
            m.freeze()
        return trks0, cands0

    def call(inputs):
        trks, cands = fresh()
        return aug(inputs, trks, cands, params)

    paths = dict(kernels_host_in=lambda: call(host_in), kernels_dev_in=lambda: call(dev_in),
                 torch_device=lambda: [torch_pipeline(s, mats_dev[i], deco_dev[i], rec[i], dev) for i, s in enumerate(samples)])
    result = dict(shape=dict(batch=BATCH, frames=FRAMES, max_points=MAX_POINTS, cols=COLS, deco=DECO, candidates=CANDS),
                  device=torch.cuda.get_device_name(0), iters=args.iters, threads=torch.get_num_threads())
    seen = {k: [] for k in paths}
    for _ in range(3):                                                 # alternating rounds: other work shares the machine
        for k, fn in paths.items():
            seen[k].append(median_ms(fn, args.iters))
    entry = {k: dict(ms=round(sorted(x for x, _ in v)[1], 4), min_ms=round(min(x for _, x in v), 4),
                     rounds_ms=[round(x, 4) for x, _ in v]) for k, v in seen.items()}

    def restate(i):
        s = samples[i]
        frames = np.split(s['points'], np.cumsum(s['lens'])[:-1])
        return R.augment_sample(frames, per_sample[i][0].numpy(), per_sample[i][1].numpy(), per_sample[i][2], rec[i], i)

    t = []
    with ThreadPoolExecutor(16) as pool:
        for _ in range(args.host_iters + 1):
            t0 = time.perf_counter()
            list(pool.map(restate, range(BATCH)))
            t.append((time.perf_counter() - t0) * 1e3)
    entry['restatement_host'] = dict(ms=round(float(np.median(t[1:])), 3), min_ms=round(min(t[1:]), 3), threads=16)
    for k in ('kernels_host_in', 'kernels_dev_in'):
        entry[k]['host_ms_per_call'] = host_ms(paths[k], args.iters)
    # the host parts of a call, each on a host clock
    parts = {}
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        fresh()
    parts['reset_of_the_tracklets_bench_only'] = (time.perf_counter() - t0) / args.host_iters * 1e3
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        aug.prepare_boxes(*fresh(), params)
    parts['prepare_boxes'] = (time.perf_counter() - t0) / args.host_iters * 1e3
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        aug.draw_params(trks0, np.random.RandomState(1), torch.Generator().manual_seed(1))
    parts['draw_params'] = (time.perf_counter() - t0) / args.host_iters * 1e3
    rows_in = int(sum(s['lens'].sum() for s in samples))
    pinned = torch.empty(rows_in * COLS * 4, dtype=torch.uint8, pin_memory=True)
    flat = np.concatenate([s['points'] for s in samples]).reshape(-1).view(np.uint8)
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        pinned.numpy()[:] = flat
    parts['pack_points_into_pinned'] = (time.perf_counter() - t0) / args.host_iters * 1e3
    stage = torch.empty_like(pinned, device=dev)
    parts['copy_points_h2d_device_ms'] = median_ms(lambda: stage.copy_(pinned, non_blocking=True), args.iters)[0]
    entry['host_parts_ms'] = {k: round(v, 4) for k, v in parts.items()}
    res = call(dev_in)
    rows_out = int(res['offsets'][-1])
    algo = 4 * COLS * rows_in + (4 * (COLS + DECO) + 4) * rows_out
    passes = (33 + 4 + 7) // 8
    entry['rows_in'], entry['rows_out'], entry['algorithmic_bytes'] = rows_in, rows_out, algo
    entry['key_bytes'] = dict(classify_write=12 * rows_in, sort_passes=passes, sort_read_write=passes * 2 * 12 * rows_in,
                              gather_key_perm_frame_read=16 * rows_in, gather_row_reread=4 * COLS * rows_out)
    for k in ('kernels_host_in', 'kernels_dev_in'):
        entry[k]['fraction_of_8TBps_algorithmic'] = round(algo / HBM_BYTES_PER_S / (entry[k]['ms'] * 1e-3), 5)
    entry['kernel_device_ms'] = kernel_times(paths['kernels_dev_in'])
    if entry['kernel_device_ms'] and 'error' not in entry['kernel_device_ms']:
        launches = sum(v for k, v in entry['kernel_device_ms'].items() if not k.startswith('Mem'))
        entry['kernel_device_ms_sum_of_launches'] = round(launches, 4)
        entry['fraction_of_8TBps_algorithmic_over_launch_time'] = round(algo / HBM_BYTES_PER_S / (launches * 1e-3), 5)
    entry['speedup_vs_torch_device'] = round(entry['torch_device']['ms'] / entry['kernels_dev_in']['ms'], 3)
    entry['speedup_vs_restatement_host'] = round(entry['restatement_host']['ms'] / entry['kernels_host_in']['ms'], 3)
    result['batch16'] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
