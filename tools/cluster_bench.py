"""Times the connected-components call (csrc/cluster.hip: sst_connected_components_xy_f32, five launches and a scan) with
device events - warm-up, then the median of --iters separately timed calls - and prints one JSON object.

    python tools/cluster_bench.py [--n 8192] [--samples 2] [--iters 30] [--tag NAME] [--out profiles/cluster/NAME.json]

The input is seeded: cluster centres of a scene (60 objects per sample on 150 m x 150 m, centres scattered 0.4 m around them),
samples stored one after the other, dist 0.6.  The library is the one sst_amd loads (SST_AMD_LIB selects another build of it),
so two builds are compared by running the tool once per build, alternating, in one session; `labels_crc` tells whether both
computed the same labels.
"""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sst_amd  # noqa: E402
from _bench_common import median_ms  # noqa: E402

DEV = 'cuda:0'


def scene(n, samples, seed=0):
    rng = np.random.default_rng(seed)
    objects = rng.uniform(-75, 75, (samples, 60, 2))
    batch = np.sort(rng.integers(0, samples, n))
    xy = objects[batch, rng.integers(0, 60, n)] + rng.normal(0, 0.4, (n, 2))
    pts = np.concatenate([xy, rng.uniform(-1, 1, (n, 1))], 1).astype(np.float32)
    return pts, batch.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--samples', type=int, default=2)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--dist', type=float, default=0.6)
    ap.add_argument('--tag', default='cluster_bench')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'cluster_bench needs a GPU'
    pts, batch = scene(args.n, args.samples)
    d_pts, d_batch = torch.from_numpy(pts).to(DEV), torch.from_numpy(batch).to(DEV)
    labels, count = sst_amd.connected_components_xy(d_pts, d_batch, args.dist, return_count=True)
    med, low = median_ms(lambda: sst_amd.connected_components_xy(d_pts, d_batch, args.dist), args.iters, warmup=5)
    res = dict(tag=args.tag, library=os.environ.get('SST_AMD_LIB', 'sst_amd/csrc/libsst_amd.so'), n=args.n, samples=args.samples,
               dist=args.dist, iters=args.iters, median_us=round(1e3 * med, 2), min_us=round(1e3 * low, 2),
               components=int(count), labels_crc=zlib.crc32(labels.cpu().numpy().tobytes()),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
