"""Times ClusterAssigner.forward with ``class_batched`` (csrc/cluster_classes.hip: all classes in one pass, one host read)
against the per-class loop (sst_amd/cluster.py as it was: per class a sorted-unique with its range read, a segmented mean, the
connected components and the size read), in ONE process, in alternating rounds, and prints one JSON object.

    python tools/cluster_classes_bench.py [--rounds 7] [--iters 20] [--mode train|eval] [--out profiles/argo2/cluster_classes_bench.json]

Per round and path: ``--iters`` calls, each ending in a device synchronise (the call's own last host read is not the end of
its device work: the caller's next step needs the outputs).  Reported per path: the median over rounds of the round's mean
host time per call (host clock, to the last synchronise) and of its mean device time per call (events around the call), the
spread over rounds ((max - min) / median), the device-to-host copies of one call as the profiler counts them (``dtoh_copies``), launches, and for the batched pass
the 256 x 256 tile pairs of the edge test that were staged and that left early.

Two seeded synthetic cases:
  fsd    the three classes of `bench.py --workload fsd` at its vote counts: its cloud generator and its foreground stand-in
         (bench_workloads.lidar_like_cloud(160000), fsd_foreground_stand_in with zero votes), its cell sizes and distances.
  argo2  six groups over +-204.8 m with the cell sizes and distances of configs/argo2/argo_onestage_12e.py.  The vote counts
         per group are a GUESS (no Argoverse 2 sweep has been run through the segmentor here): vehicles dominate, riders and
         small objects are few.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sst_amd  # noqa: E402
from sst_amd import cluster  # noqa: E402
from _bench_common import count_launches  # noqa: E402

DEV = 'cuda:0'
ARGO2_RANGE = [-204.8, -204.8, -3.2, 204.8, 204.8, 3.2]
ARGO2_CELLS = [(0.3, 0.3, 6.4), (0.05, 0.05, 6.4), (0.08, 0.08, 6.4), (0.5, 0.5, 6.4), (0.1, 0.1, 6.4), (0.08, 0.08, 6.4)]
ARGO2_DISTS = [0.6, 0.1, 0.15, 1.0, 0.2, 0.15]
# (votes, objects, scatter of the votes around an object's centre in metres) per group and sample: a guess
ARGO2_GROUPS = [(30000, 120, 0.25), (4000, 60, 0.04), (3000, 80, 0.06), (12000, 25, 0.4), (1500, 30, 0.08), (300, 6, 0.06)]


def fsd_case():
    import bench_workloads as W
    cloud = W.lidar_like_cloud(160000, 1000, DEV)[0]
    votes = torch.zeros(cloud.size(0), 3, 3, device=DEV)
    sel, pts = W.fsd_foreground_stand_in(cloud, votes)
    cfg = W.FSD_CFG
    a = sst_amd.ClusterAssigner(point_cloud_range=cfg['pc_range'], class_names=cfg['classes'], **cfg['cluster'])
    return a, [p.contiguous() for p in pts], [torch.zeros(p.size(0), dtype=torch.int32, device=DEV) for p in pts]


def argo2_case(samples=2, seed=0):
    rng = np.random.default_rng(seed)
    pts, bat = [], []
    for votes, objects, sigma in ARGO2_GROUPS:
        centres = rng.uniform(-200, 200, (samples, objects, 2))
        b = np.sort(rng.integers(0, samples, votes * samples))
        xy = centres[b, rng.integers(0, objects, len(b))] + rng.normal(0, sigma, (len(b), 2))
        p = np.concatenate([xy, rng.uniform(-1, 1, (len(b), 1))], 1).astype(np.float32)
        pts.append(torch.from_numpy(p).to(DEV))
        bat.append(torch.from_numpy(b.astype(np.int32)).to(DEV))
    names = [f'group{i + 1}' for i in range(6)]
    a = sst_amd.ClusterAssigner([list(c) for c in ARGO2_CELLS], 2, ARGO2_RANGE, list(ARGO2_DISTS), class_names=names)
    return a, pts, bat


def timed_round(fn, iters):
    """-> (host ms per call, device ms per call), every call ended by a synchronise"""
    torch.cuda.synchronize()
    dev_ms = 0.0
    t0 = time.perf_counter()
    for _ in range(iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        dev_ms += start.elapsed_time(stop)
    return 1e3 * (time.perf_counter() - t0) / iters, dev_ms / iters


def summary(rounds):
    host, devt = np.array([r[0] for r in rounds]), np.array([r[1] for r in rounds])
    return dict(host_ms=round(float(np.median(host)), 4), device_ms=round(float(np.median(devt)), 4),
                host_spread=round(float((host.max() - host.min()) / np.median(host)), 3),
                device_spread=round(float((devt.max() - devt.min()) / np.median(devt)), 3),
                host_ms_rounds=[round(float(v), 4) for v in host])


def crc(result):
    inds, masks = result
    h = 0
    for t in list(inds) + list(masks):
        h = zlib.crc32(t.cpu().numpy().tobytes(), h)
    return h


def run_case(name, a, pts, bat, training, rounds, iters):
    a.train(training)
    a.class_batched = False
    loop = lambda: a(pts, bat)                                                          # noqa: E731
    want = loop()
    cluster.enable_class_batched(a)
    fused = lambda: a(pts, bat)                                                         # noqa: E731
    got = fused()
    same = all(torch.equal(x, y) for x, y in zip(want[0] + want[1], got[0] + got[1]))
    g = len(pts)
    cells = [a._per_class(a.cluster_voxel_size, c) for c in a.class_names[:g]]
    dists = [a._per_class(a.connected_dist, c) for c in a.class_names[:g]]
    stats = cluster._assign_classes(pts, bat, cells, dists, a.min_points, a.point_cloud_range[:3], training, count_tiles=True)[2]
    res = dict(case=name, mode='train' if training else 'eval', classes=g, votes=[int(p.size(0)) for p in pts],
               kept_votes=[int(i.size(0)) for i in want[0]], centroids=stats['centroids'], outputs_equal=bool(same),
               crc_loop=crc(want), crc_batched=crc(got), tiles_staged=stats['tiles_run'], tiles_left_early=stats['tiles_skipped'])
    per = dict(loop=[], batched=[])
    for fn in (loop, fused):                                                            # warm both before any timed round
        a.class_batched = fn is fused
        for _ in range(3):
            fn()
    for _ in range(rounds):                                                             # alternating rounds
        a.class_batched = False
        per['loop'].append(timed_round(loop, iters))
        a.class_batched = True
        per['batched'].append(timed_round(fused, iters))
    res['loop'], res['batched'] = summary(per['loop']), summary(per['batched'])
    for key, fn, flag in (('loop', loop, False), ('batched', fused, True)):
        a.class_batched = flag
        n = count_launches(fn, readback_names=('Memcpy DtoH (Device -> Host)', 'Memcpy DtoH (Device -> Pageable)'))
        if n is not None:
            res[key].update(launches=n['ours'] + n['torch'], memsets=n['memsets'], copies=n['copies'],
                            dtoh_copies=n.get('device_to_host'))
    spread = max(res['loop']['host_spread'], res['batched']['host_spread'])
    res['batched_not_slower'] = bool(res['batched']['host_ms'] <= res['loop']['host_ms'] * (1 + spread))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--mode', choices=('train', 'eval', 'both'), default='both')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'cluster_classes_bench needs a GPU'
    results = []
    for name, make in (('fsd', fsd_case), ('argo2', argo2_case)):
        a, pts, bat = make()
        for training in ((True, False) if args.mode == 'both' else (args.mode == 'train',)):
            if name == 'fsd' and not training and args.mode == 'both':
                continue                                      # one sample: both partitions are the same graph
            results.append(run_case(name, a, pts, bat, training, args.rounds, args.iters))
    out = dict(tool='cluster_classes_bench', device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters,
               argo2_vote_counts='a guess: no Argoverse 2 sweep was measured', results=results)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
