"""Times the FSD foreground sampling stage (csrc/fg_sample.hip: sampling, the composed gather after the cluster filter, the RoI
input; forward + backward) with device events after warm-up (the median of --iters separately timed steps, three alternating
rounds), against the same stage in the reference's data flow - boolean-mask indexing per class and tensor, a second indexing by
the valid mask, the concatenations, a stable sort (tests/fsd_sample_ref.py) - in torch on the same device.  Prints one JSON object.

    python tools/fg_sample_bench.py [--iters 20] [--out profiles/fg_sample/fg_sample_bench.json] [--no-profiler]

Sizes: the FSD workload's 160 000 points, C = 3, F = 67, 128 cluster feature columns, B = 1 and 2, foreground shares of 5 %, 20 %
and 50 % per class; the cluster filter keeps 90 % of the rows (drawn once, index lists for both paths).  Per path: milliseconds,
kernel launches (torch.profiler, separate untimed step), host synchronisations (one step under
torch.cuda.set_sync_debug_mode('warn'), warnings counted, as tools/sync_sites.py does), and the stage's algorithmic bytes
 over the fused time."""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _bench_common  # noqa: E402
from _bench_common import median_ms  # noqa: E402
import fsd_sample_ref as R  # noqa: E402
from sst_amd import fg_sample as FS  # noqa: E402

DEV = 'cuda:0'
N, C, F, FC, P = 160000, 3, 67, 128, 5


def count_syncs(fn):
    seen = [0]
    old = warnings.showwarning

    def hook(message, *a, **k):
        if 'synchroniz' in str(message):
            seen[0] += 1
    warnings.showwarning = hook
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('always')
            warnings.showwarning = hook
            torch.cuda.set_sync_debug_mode('warn')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
        warnings.showwarning = old
    return seen[0]


def stage_bytes(n, c, f, fc, p, m, rows):
    """what the stage has to move: launch A reads logits + batch index and writes the mask word; launch C reads
    word + batch index and writes slot, mask, and per selected row src, centre (reads point + vote), batch index, point; the
    gather reads and writes M rows of C + 3C + F floats and P point columns; the RoI input writes R rows of Fc + F (+ P + index);
    the backward reads M x F and R x (Fc + F) and writes N x F twice and M x Fc"""
    sel = m / 0.9
    a = n * (4 * c + 8 + 4)
    cc = n * (4 + 8 + 5 * c) + sel * (4 + 24 + 12 + 8 + 8 * p)
    gather = m * (2 * 4 * (4 * c + f) + 8 * p + 4) + n * c * 9
    roi = 2 * n * (c + 1) * 9 + rows * (4 * (fc + f) * 2 + 8 * p + 16)
    bwd = m * 4 * f + 2 * n * 4 * f + rows * 4 * (fc + f) + m * 4 * fc + n * 4 * (2 * c + 1)
    return int(a + cc + gather + roi + bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-profiler', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'fg_sample_bench needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), points=N, classes=C, feat_cols=F, cluster_cols=FC, iters=args.iters, cases=[])
    for b in (1, 2):
        for share in (0.05, 0.2, 0.5):
            data, thr = R.make_case(N, C, b, F, seed=int(share * 100) + b, p_cols=P, fg=share, device=DEV)
            want = R.sample(data, thr)
            g = torch.Generator().manual_seed(1)
            valid = [(torch.rand(t.size(0), generator=g) < 0.9).to(DEV) for t in want['seg_points']]
            keeps = [torch.nonzero(v)[:, 0] for v in valid]
            upd = R.update_by_mask(want, valid)
            m = sum(k.numel() for k in keeps)
            rows = int((torch.stack(upd['fg_mask_list']).sum(0) == 0).sum()) + m
            cluster = torch.randn(m, FC, device=DEV, requires_grad=True)
            feats = data['seg_feats'].clone().requires_grad_(True)

            def fused():
                feats.grad = cluster.grad = None
                smp = FS.fg_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, b)
                out = FS.fg_gather_cat(smp, keeps, data['seg_logits'], data['seg_vote_preds'], feats, data['seg_points'])
                _, cat_feats, _, _ = FS.roi_input(data['seg_points'], cluster, feats, out['fg_mask_list'], data['batch_idx'], b,
                                                  slot2=out['slot2'], num_rows=rows)
                (out['pts_feats'].sum() + cat_feats.sum()).backward()
                return out['pts_feats'], cat_feats

            def composed():
                feats.grad = cluster.grad = None
                d = dict(data, seg_feats=feats)
                smp = R.sample(d, thr)
                u = R.update_by_mask(smp, valid)
                comb = R.combine(u)
                _, cat_feats, _ = R.roi_multi(d['seg_points'], cluster, feats, u['fg_mask_list'], d['batch_idx'])
                (comb['pts_feats'].sum() + cat_feats.sum()).backward()
                return comb['pts_feats'], cat_feats

            a, c2 = fused(), composed()
            same = bool(torch.equal(a[0], c2[0]) and torch.equal(a[1], c2[1]))
            rounds = dict(fused=[], composed=[])
            for _ in range(3):                   # alternate the paths: other work shares the machine
                rounds['fused'].append(median_ms(fused, args.iters))
                rounds['composed'].append(median_ms(composed, args.iters))
            case = dict(samples=b, share=share, selected_rows=int(sum(t.size(0) for t in want['seg_points'])), kept_rows=m,
                        roi_rows=rows, outputs_equal=same, fused_host_syncs=count_syncs(fused), composed_host_syncs=count_syncs(composed))
            for k, v in rounds.items():
                case[k + '_ms'] = round(sorted(x for x, _ in v)[1], 4)
                case[k + '_min_ms'] = round(min(x for _, x in v), 4)
                case[k + '_rounds_ms'] = [round(x, 4) for x, _ in v]
            case['composed_over_fused'] = round(case['composed_ms'] / case['fused_ms'], 2)
            case['algorithmic_bytes'] = stage_bytes(N, C, F, FC, P, m, rows)
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
