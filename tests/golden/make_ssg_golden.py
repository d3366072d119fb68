"""Writes tests/golden/ssg.npz: the reference's own `ssg` and the `forward_single_class` of its SSGAssigner / HybridAssigner
(detectors/single_stage_fsd.py:83-142, 1002-1194), executed from their source text on CPU through oracle.ref_loader, with
the sampling kernel replaced by its float32 restatement (tests/fps_ref.py, pinned to a thread-by-thread simulation of the
kernel by tests/test_fps_host.py).  Needs the reference tree; run from the repository root:

    python tests/golden/make_ssg_golden.py

Inputs: three clustered families (60 centres in +-50 m, three samples, coordinates multiples of 1/64 so that the voxel
sums of the assigners are exact in any order); `short` takes ssg_single_sample's `num_fps >= len(points)` branch.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import fps_ref as R  # noqa: E402


def main():
    ref = R.load_reference_ssg()
    out = {}
    for name in R.FAMILIES:
        pts, batch, num_fps, radius = R.family(name)
        ids = ref.ssg(torch.from_numpy(pts), torch.from_numpy(batch), num_fps, radius)     # all of its asserts hold
        out[f'{name}_points'], out[f'{name}_batch'], out[f'{name}_ssg'] = pts, batch, ids.numpy().astype(np.int64)
        print(name, 'points', len(pts), 'clusters', int(ids.max()) + 1, 'unassigned %.1f %%' % (100 * float((ids < 0).float().mean())))
    for tag, cls, cfg in (('ssgassigner', ref.SSGAssigner, R.SSG_ASSIGNER), ('hybrid', ref.HybridAssigner, R.HYBRID_ASSIGNER)):
        module = cls(**copy.deepcopy(cfg))
        for class_name, fam in R.CLASS_FAMILY.items():
            pts, batch, _, _ = R.family(fam)
            rows, mask = module.forward_single_class(torch.from_numpy(pts), torch.from_numpy(batch), class_name, None)
            out[f'{tag}_{class_name}_rows'], out[f'{tag}_{class_name}_mask'] = rows.numpy().astype(np.int64), mask.numpy()
            print(tag, class_name, 'rows', tuple(rows.shape), 'clusters', int(rows[:, 1].max()) + 1)
    path = os.path.join(HERE, 'ssg.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
