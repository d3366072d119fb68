"""Times furthest point sampling and the SSG assignment (csrc/fps.hip) with device events - warm-up, then the median of
--iters separately timed calls - and prints one JSON object.

    python tools/fps_bench.py [--iters 20] [--out profiles/fps/fps_bench.json] [--quick]

- furthest_point_sample at N in {2 000, 20 000, 100 000} x M in {128, 1024}: microseconds per sample, the storage tier the
  size ran in, and the same for a torch-composed sampling on the same device (per sample: subtract, square-sum, minimum,
  arg-max, and the gather of the next centre; nothing is read back inside the loop);
- ssg() for three samples x 20 000 centres at num_fps 1024, against a torch port of the reference's flow
  (detectors/single_stage_fsd.py:83-142: a Python loop over the samples, dense [K, K] and [K, N] matrices, nonzero, sort and
  the asserts with their read-backs) that uses this library's sampling kernel for its `fps`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sst_amd  # noqa: E402
from sst_amd import cluster  # noqa: E402

DEV = 'cuda:0'


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


def tier(n):
    for ppt in (1, 2, 4, 8, 16):
        if n <= 1024 * ppt:
            return f'registers, {ppt} per thread'
    return '12 per thread in registers, the rest streamed'


def composed_fps(pts, m):
    """the same recurrence from torch ops (ties: torch's arg-max, i.e. not the reference's rule); all on the device"""
    n = pts.size(0)
    temp = torch.full((n,), 1e10, device=pts.device)
    idx = torch.zeros(m, dtype=torch.long, device=pts.device)
    old = idx[0:1]
    for j in range(1, m):
        d = ((pts - pts.index_select(0, old)) ** 2).sum(1)
        temp = torch.minimum(temp, d)
        old = torch.argmax(temp).view(1)
        idx[j:j + 1] = old
    return idx


def reference_flow_ssg(points, batch_idx, num_fps, radius):
    """ssg / ssg_single_sample of the reference as it is written, on the device"""
    bsz = batch_idx.max().item() + 1
    base = 0
    out = torch.zeros_like(batch_idx) - 2
    for i in range(bsz):
        mask = batch_idx == i
        if mask.any():
            pts = points[mask]
            keys = pts if num_fps >= len(pts) else cluster.fps(pts, num_fps)
            kd = ((keys[:, None, :2] - keys[None, :, :2]) ** 2).sum(2) ** 0.5
            close = kd < radius * 2 + 0.01
            ar = torch.arange(len(keys), device=pts.device)
            close[ar[None, :].expand(len(keys), -1) <= ar[:, None]] = False
            keys = keys[~close.any(0)]
            inside = (((keys[:, None, :2] - pts[None, :, :2]) ** 2).sum(2) ** 0.5) < radius
            assert (inside.sum(0) <= 1).all()
            valid = inside.sum(0) == 1
            assert valid.any()
            pos = torch.nonzero(inside)
            cols, order = torch.sort(pos[:, 1])
            ids = pos[:, 0][order]
            assert (cols == torch.nonzero(valid).reshape(-1)).all()
            full = ids.new_zeros(len(pts)) - 1
            full[valid] = ids
            full[full > -1] += base
            base = full.max().item() + 1
            out[mask] = full
    assert (out > -2).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='native kernels only, few repeats (for a profiler run)')
    args = ap.parse_args()
    it = 3 if args.quick else args.iters
    res = {'device': torch.cuda.get_device_name(0), 'iters': it, 'statistic': 'median', 'fps': []}
    g = torch.Generator().manual_seed(0)
    for n in (2000, 20000, 100000):
        pts = ((torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([75.0, 75.0, 3.0])).to(DEV)
        for m in (128, 1024):
            native = median_ms(lambda: sst_amd.furthest_point_sample(pts[None], m), it)
            row = dict(N=n, M=m, tier=tier(n), native_ms=round(native, 4), native_us_per_sample=round(1e3 * native / m, 3))
            if not args.quick:
                comp = median_ms(lambda: composed_fps(pts, m), it, warmup=1)
                same = bool(torch.equal(composed_fps(pts, m).int(), sst_amd.furthest_point_sample(pts[None], m)[0]))
                row.update(torch_composed_ms=round(comp, 4), torch_composed_us_per_sample=round(1e3 * comp / m, 3),
                           composed_over_native=round(comp / native, 2), same_indices_as_composed=same)
            res['fps'].append(row)

    n, samples, num_fps, radius = 20000, 3, 1024, 1.0
    pts = ((torch.rand(n * samples, 3, generator=g) * 2 - 1) * torch.tensor([75.0, 75.0, 3.0])).to(DEV)
    batch = torch.arange(samples).repeat_interleave(n).to(DEV)
    native = median_ms(lambda: sst_amd.ssg(pts, batch, num_fps, radius), it)
    row = dict(samples=samples, centres_per_sample=n, num_fps=num_fps, radius=radius, native_ms=round(native, 4))
    if not args.quick:
        ref = median_ms(lambda: reference_flow_ssg(pts, batch, num_fps, radius), it, warmup=1)
        row.update(reference_flow_ms=round(ref, 4), reference_flow_over_native=round(ref / native, 2),
                   same_ids=bool(torch.equal(reference_flow_ssg(pts, batch, num_fps, radius), sst_amd.ssg(pts, batch, num_fps, radius))))
    res['ssg'] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
