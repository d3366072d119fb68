"""Times the FSDv2 grouped sampling stage (csrc/fg_group_sample.hip: the sampling and the virtual projector's input rows;
forward + backward) with device events after warm-up (the median of --iters separately timed steps, three alternating rounds),
against the same stage in the reference's data flow - softmax, grouped scores, boolean-mask indexing per group and tensor, the
concatenations, the clip and the column concatenation (tests/fsdv2_sample_ref.py) - in torch on the same device and in the same
process.  Prints one JSON object.

    python tools/fg_group_sample_bench.py [--iters 20] [--out profiles/fg_group_sample/fg_group_sample_bench.json] [--no-profiler]

Sizes: 300 000 points, F = 131 feature columns, P = 5 point columns; K = 11 logits with the six nuScenes groups and K = 4 logits
with three single-class groups; B = 1 and 2; 5 %, 20 % and 50 % of the points selected by at least one group (the background logit
is shifted until that share is met).  Per path: milliseconds, kernel launches (torch.profiler, separate untimed step), host
synchronisations (one step under torch.cuda.set_sync_debug_mode('warn'), warnings counted), and the stage's algorithmic bytes
 over the fused time."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import _bench_common  # noqa: E402
from _bench_common import median_ms  # noqa: E402
import fsdv2_sample_ref as R  # noqa: E402
from fg_sample_bench import count_syncs  # noqa: E402
from sst_amd import fg_group_sample as GS  # noqa: E402

DEV = 'cuda:0'
N, F, P = 300000, 131, 5
PC_RANGE = [-51.2, -51.2, -5, 51.2, 51.2, 3]
SHAPES = {'K11_G6': (11, R.groups_by_names(R.NUSC_GROUPS, R.NUSC_CLASSES), R.NUSC_THRESH),
          'K4_C3': (4, [[0], [1], [2]], [0.3, 0.25, 0.25])}


def stage_bytes(n, k, groups, f, p, rows):
    """what the stage has to move: launch A reads logits + batch index and writes the mask word; launch C reads
    word + batch index, writes slot and mask per group, and per selected row reads the group's logits and votes and the point
    and writes src, centre, batch index, point; the gather reads src, centre and the F + K + P source floats of a row and writes
    F + 3 + K + (P - 3) + 3; the backward reads the F gradient columns of every row and the slots and writes N x F"""
    g = len(groups)
    per_group = sum(len(x) for x in groups) / g
    a = n * (4 * k + 8 + 4)
    c = n * (4 + 8 + 5 * g) + rows * (4 + 16 * per_group + 4 * p + 12 + 8 + 4 * p)
    fwd = rows * (4 + 12 + 4 * (f + k + p) + 4 * (f + 3 + k + p - 3) + 12)
    bwd = rows * 4 * f + n * 4 * g + n * 4 * f
    return int(a + c + fwd + bwd)


def make_data(k, groups, thr32, b, share, seed):
    """logits whose background column is shifted until ``share`` of the points pass some group; every grouped score clear of
    its threshold (the restatement's margin), so both paths select the same rows"""
    data = R.make_case(N, k, b, F, seed, groups, thr32, p_cols=P, fg=0.5, int_feats=False)
    base = data['seg_logits'].clone()
    t = torch.tensor(thr32)
    lo, hi = -20.0, 20.0
    for _ in range(30):
        mid = (lo + hi) / 2
        lg = base.clone()
        lg[:, -1] += mid
        got = float((R.grouped_scores(lg, groups) > t[None]).any(1).float().mean())
        lo, hi = (mid, hi) if got > share else (lo, mid)
    base[:, -1] += (lo + hi) / 2
    data['seg_logits'] = R.redraw_until_clear(base, groups, thr32, torch.Generator().manual_seed(seed + 1))
    data['seg_points'][:, 2] *= 0.3                      # some centres leave the range in z: the clip works
    return {name: v.to(DEV) for name, v in data.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'fg_group_sample_bench needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), points=N, feat_cols=F, point_cols=P, iters=args.iters, cases=[])
    for shape, (k, groups, thresh) in SHAPES.items():
        thr = R.thresholds32(thresh)
        for b in (1, 2):
            for share in (0.05, 0.2, 0.5):
                data = make_data(k, groups, thr, b, share, seed=int(share * 100) + b + k)
                feats = data['seg_feats'].clone().requires_grad_(True)

                def fused():
                    feats.grad = None
                    smp = GS.group_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], groups,
                                          thr, b)
                    rows, clipped = GS.virtual_rows(smp, feats, data['seg_logits'], data['seg_points'], PC_RANGE)
                    rows.sum().backward()
                    return rows, clipped

                def composed():
                    feats.grad = None
                    smp = R.group_sample(dict(data, seg_feats=feats), groups, thr)
                    rows, clipped = R.virtual_input(R.combine(smp), PC_RANGE)
                    rows.sum().backward()
                    return rows, clipped

                a, c2 = fused(), composed()
                same = bool(torch.equal(a[0], c2[0]) and torch.equal(a[1], c2[1]))
                rounds = dict(fused=[], composed=[])
                for _ in range(3):                   # alternate the paths: other work shares the machine
                    rounds['fused'].append(median_ms(fused, args.iters))
                    rounds['composed'].append(median_ms(composed, args.iters))
                n_rows = int(a[0].size(0))
                case = dict(shape=shape, logits=k, groups=len(groups), samples=b, share=share, selected_rows=n_rows,
                            selected_points=round(float((R.grouped_scores(data['seg_logits'], groups)
                                                         > torch.tensor(thr, device=DEV)[None]).any(1).float().mean()), 4),
                            outputs_equal=same, fused_host_syncs=count_syncs(fused), composed_host_syncs=count_syncs(composed))
                for name, v in rounds.items():
                    case[name + '_ms'] = round(sorted(x for x, _ in v)[1], 4)
                    case[name + '_min_ms'] = round(min(x for _, x in v), 4)
                    case[name + '_rounds_ms'] = [round(x, 4) for x, _ in v]
                case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
                case['algorithmic_bytes'] = stage_bytes(N, k, groups, F, P, n_rows)
                case['fused_gbytes_per_s'] = round(case['algorithmic_bytes'] / (case['fused_ms'] * 1e-3) / 1e9, 1)
                if not args.no_profiler:
                    case['fused_launches'] = _bench_common.count_launches(fused, ours='fg_')
                    case['composed_launches'] = _bench_common.count_launches(composed)
                res['cases'].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
