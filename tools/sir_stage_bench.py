"""Times the fused SIR stage (csrc/sir_stage.hip) against the composed one (library GEMM -> LayerNorm row kernel -> tile
reduction, with the gather + concat in front of a second stage) with device events - warm-up, then the median of --iters
separately timed calls - and prints one JSON object.

    python tools/sir_stage_bench.py [--iters 20] [--out profiles/sir_stage/sir_stage_bench.json]
    python tools/sir_stage_bench.py --leg fused|composed [--iters 20]        # one stage only, for a profiler run
    python tools/sir_stage_bench.py --merge-stats fused=A.csv composed=B.csv --iters 20 --stats-out OUT.csv [--out JSON]

- one stage, forward and forward + backward, at N = 20 000 and 60 000 points in clusters of about 30 points with a long tail
  (a few of thousands), K = 84, 133, 213 and K = 128 with the previous stage's pooled rows (`add_rows` / concat);
- a three-block SIR (K = 84 / 133 / 133, LN + GELU, max pooling) forward + backward with the switch off and on;
- bytes: the stage's compulsory traffic (x and W read, pre / y / stats written, pooled + argmax written) over the fused time
  as a fraction of 8 TB/s.
--leg runs warm-up + --iters forward + backward calls of the split second stage at N = 20 000 and nothing else, so that the
`Calls` column of `rocprofv3 --kernel-trace --stats` divided by the number of calls is the launch count of the leg;
--merge-stats turns two such kernel-stats files into one table (kernels called at least once per iteration) and adds the
launch counts to the JSON object.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sst_amd  # noqa: E402
from sst_amd import kernels as K  # noqa: E402
from sst_amd.dense import add_layer_norm, tall_linear  # noqa: E402
from sst_amd.voxel_encoder import DynamicVFELayerV2  # noqa: E402

DEV = 'cuda:0'
C = 128
LEG_WARMUP = 3


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return 0.5 * (times[(len(times) - 1) // 2] + times[len(times) // 2])


def cluster_ids(n, rng):
    """cluster sizes with a mean of about 30 and a long tail: a few clusters of thousands, most of a handful to a hundred"""
    sizes = [3000, 1700, 900, 512]
    while sum(sizes) < n:
        sizes.append(int(min(2000, 1 + rng.pareto(1.6) * 12)))
    sizes[-1] -= sum(sizes) - n
    sizes = [s for s in sizes if s > 0]
    ids = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(ids)
    return ids, len(sizes)


class Stage(object):
    """one stage on a fixed input: K columns of point features, optionally the previous stage's pooled rows"""

    def __init__(self, n, k, split, rng):
        ids, self.m = cluster_ids(n, rng)
        self.n, self.k, self.split = n, k, split
        self.plan = K.unique_rows(torch.from_numpy(ids).reshape(-1, 1).contiguous().to(DEV))
        assert self.plan.m == self.m
        self.x = torch.randn(n, k, device=DEV).requires_grad_(True)
        self.prev = torch.randn(self.m, C, device=DEV).requires_grad_(True) if split else None
        self.layer = DynamicVFELayerV2(k + C if split else k, C, dict(type='LN', eps=1e-3), act='gelu').to(DEV)
        self.gy = torch.randn(n, C, device=DEV)
        self.gp = torch.randn(self.m, C, device=DEV)
        self.group_sum = lambda part: K.segment_reduce(part, self.plan, 'sum')

    def fused(self):
        w = self.layer.linear.weight
        if self.split:
            return sst_amd.sir_stage(self.x, w[:, :self.k], self.layer.norm, self.layer.act, self.plan,
                                     add_rows=tall_linear(self.prev, w[:, self.k:]))
        return sst_amd.sir_stage(self.x, w, self.layer.norm, self.layer.act, self.plan)

    def composed(self):
        xin = K.concat_gather(self.x, self.prev, self.plan.inverse, self.group_sum) if self.split else self.x
        y = add_layer_norm(tall_linear(xin, self.layer.linear.weight), None, self.layer.norm, act=self.layer.act)
        return y, K.segment_reduce(y, self.plan, 'max')

    def fwd_bwd(self, path):
        def run():
            y, pooled = path()
            torch.autograd.backward([y, pooled], [self.gy, self.gp])
        return run

    def bytes_moved(self):
        """compulsory traffic of the forward: x, W, add rows read; pre, y, stats, pooled, argmax written"""
        return 4 * (self.n * self.k + C * self.k + (self.m * C if self.split else 0) + self.n * (2 * C + 2) + 2 * self.m * C)


def build_sir(n, rng):
    ids, m = cluster_ids(n, rng)
    sir = sst_amd.build_backbone(dict(type='SIR', num_blocks=3, in_channels=[84, 133, 133], feat_channels=[[128, 128]] * 3,
                                      rel_mlp_hidden_dims=[[16, 32]] * 3, norm_cfg=dict(type='LN', eps=1e-3), mode='max',
                                      xyz_normalizer=[20, 20, 4], act='gelu', unique_once=True)).to(DEV).train()
    points = torch.randn(n, 5, device=DEV)
    feats = torch.randn(n, 79, device=DEV).requires_grad_(True)
    coors = torch.from_numpy(ids).reshape(-1, 1).to(DEV)
    f_cluster = torch.randn(n, 3, device=DEV)

    def run():
        pf, cf, _ = sir(points, feats, coors, f_cluster)
        (pf.sum() + cf.sum()).backward()
    return sir, run, m


def measure(iters):
    res = {'device': torch.cuda.get_device_name(0), 'iters': iters, 'statistic': 'median', 'unit': 'ms',
           'tile_rows': sst_amd.sir_stage_tile_rows(), 'stage': [], 'sir': []}
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    for n in (20000, 60000):
        for k, split in ((84, False), (133, False), (213, False), (128, True)):
            st = Stage(n, k, split, rng)
            with torch.no_grad():
                ff = median_ms(st.fused, iters)
                cf = median_ms(st.composed, iters)
            fb = median_ms(st.fwd_bwd(st.fused), iters)
            cb = median_ms(st.fwd_bwd(st.composed), iters)
            res['stage'].append(dict(N=n, groups=st.m, K=k, add_rows=split, fused_fwd_ms=round(ff, 4), composed_fwd_ms=round(cf, 4),
                                     fused_fwd_bwd_ms=round(fb, 4), composed_fwd_bwd_ms=round(cb, 4),
                                     fwd_fused_over_composed=round(ff / cf, 3), fwd_bwd_fused_over_composed=round(fb / cb, 3),
                                     fwd_MB=round(st.bytes_moved() / 1e6, 2),
                                     fwd_fraction_of_8TBs=round(st.bytes_moved() / (ff * 1e-3) / 8e12, 4)))
        sir, run, m = build_sir(n, rng)
        sst_amd.enable_fused_sir(sir, False)
        off = median_ms(run, iters)
        sst_amd.enable_fused_sir(sir, True)
        on = median_ms(run, iters)
        res['sir'].append(dict(N=n, groups=m, blocks=3, fwd_bwd_switch_off_ms=round(off, 4), fwd_bwd_switch_on_ms=round(on, 4),
                               on_over_off=round(on / off, 3)))
    return res


def run_leg(leg, iters):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    st = Stage(20000, 128, True, rng)
    fn = st.fwd_bwd(st.fused if leg == 'fused' else st.composed)
    for _ in range(LEG_WARMUP + iters):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(leg=leg, calls=LEG_WARMUP + iters, N=st.n, groups=st.m)))


def merge_stats(pairs, iters, stats_out):
    calls = LEG_WARMUP + iters
    rows, counts = [], {}
    for leg, path in pairs:
        with open(path) as f:
            for r in csv.DictReader(f):
                c = int(r['Calls'])
                if c < calls:          # set-up of the inputs (sorted-unique, random fills): not part of a call
                    continue
                rows.append(dict(leg=leg, Name=r['Name'], Calls=c, calls_per_iteration=round(c / calls, 2),
                                 TotalDurationNs=r['TotalDurationNs'], AverageNs=r['AverageNs']))
                counts[leg] = counts.get(leg, 0) + c / calls
    os.makedirs(os.path.dirname(os.path.abspath(stats_out)), exist_ok=True)
    with open(stats_out, 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=['leg', 'Name', 'Calls', 'calls_per_iteration', 'TotalDurationNs', 'AverageNs'])
        w.writeheader()
        w.writerows(rows)
    return {leg: round(v, 2) for leg, v in counts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', choices=('fused', 'composed'), default=None)
    ap.add_argument('--merge-stats', nargs='+', default=None, metavar='LEG=CSV')
    ap.add_argument('--stats-out', default='profiles/sir_stage/sir_stage_kernel_stats.csv')
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.leg, args.iters)
    if args.merge_stats:
        counts = merge_stats([p.split('=', 1) for p in args.merge_stats], args.iters, args.stats_out)
        res = {}
        if args.out and os.path.exists(args.out):
            with open(args.out) as f:
                res = json.loads(f.read())
        res['launches_per_fwd_bwd_call_split_stage_N20000'] = counts
    else:
        res = measure(args.iters)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
