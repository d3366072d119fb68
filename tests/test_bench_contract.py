"""CPU: the part of bench.py's contract that does not need a GPU - rank 0 prints ONE JSON line on stdout and nothing else,
whoever else writes to stdout meanwhile (Python prints of modules built from a shipped config, native libraries such as gloo
announcing its peers on fd 1, child processes)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_only_the_line_reaches_stdout():
    code = '\n'.join([
        'import os, subprocess, sys',
        'sys.path.insert(0, %r)' % ROOT,
        'import bench',
        'out = bench.claim_stdout()',
        'os.write(1, b"native library noise on fd 1\\n")',
        'print("python print")',
        'subprocess.call([sys.executable, "-c", "print(\'child process noise\')"])',
        'print(\'{"metric": "x", "value": 1}\', file=out)',
        'out.flush()',
    ])
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == '{"metric": "x", "value": 1}\n', r.stdout
    for noise in ('native library noise', 'python print', 'child process noise'):
        assert noise in r.stderr


def test_help_goes_to_stdout():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and '--gpus' in r.stdout and '--steps' in r.stdout and '--warmup' in r.stdout


def test_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and '--full' in r.stdout and '--dump-outputs' in r.stdout


def test_dump_outputs_writes_float_arrays_within_budget(tmp_path):
    """--dump-outputs: every array as <name>.npy in float32 (float64 kept); arrays beyond the budget become the same fixed
    sample of rows on every run, with the indices of those rows beside them"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {'voxel_feats': torch.randn(5000, 16, generator=g), 'voxel_coors': torch.randint(0, 468, (5000, 4), dtype=torch.int32),
              'param_grads': torch.randn(3000, generator=g, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / 'all'), arrays)
    for name, t in arrays.items():
        a = np.load(tmp_path / 'all' / (name + '.npy'))
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert np.array_equal(a, t.double().numpy())
    budget = 100000
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), arrays, budget=budget)
    assert sum(f.stat().st_size for f in (tmp_path / 'a').iterdir()) <= budget + 128 * len(list((tmp_path / 'a').iterdir()))
    rows = np.load(tmp_path / 'a' / 'voxel_feats_rows.npy').astype(np.int64)
    feats = np.load(tmp_path / 'a' / 'voxel_feats.npy')
    assert np.array_equal(feats, arrays['voxel_feats'].numpy()[rows]) and np.all(np.diff(rows) > 0)
    for f in (tmp_path / 'a').iterdir():
        assert np.array_equal(np.load(f), np.load(tmp_path / 'b' / f.name))
