"""CPU: pins tests/seg_reduce_ref.py, the reference of tests/test_gpu_seg_reduce_edges.py - its reductions and gradients against
torch.scatter_reduce in float64 and against hand-worked groupings with ties, its restatement of the kernels' geometry against
the library's own size functions, and the groupings against the edges they claim to reach."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_reduce_ref as R  # noqa: E402


def _lib():
    from sst_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('seed,n,m,c', [(0, 1, 1, 1), (1, 200, 7, 3), (2, 3000, 40, 5), (3, 500, 90, 4)])
def test_reductions_equal_torch_scatter_reduce(seed, n, m, c):
    rng = np.random.default_rng(seed)
    ids = rng.integers(-1, m + 1, size=n)                  # -1 and m: rows of no group
    if m > 4:
        ids[ids == 3] = 4                                  # an empty group where there is room for one
    for feats in (R.exact_feats(n, c, seed), rng.standard_normal((n, c)).astype(np.float32)):
        ok = (ids >= 0) & (ids < m)
        idx = torch.from_numpy(ids[ok])[:, None].expand(-1, c)
        src = torch.from_numpy(feats[ok]).double()
        lens = np.bincount(ids[ok], minlength=m)
        want_sum = torch.zeros(m, c, dtype=torch.float64).scatter_reduce(0, idx, src, 'sum').numpy()
        want_max = torch.zeros(m, c, dtype=torch.float64).scatter_reduce(0, idx, src, 'amax', include_self=False).numpy()
        np.testing.assert_allclose(R.reduce_ref(feats, ids, m, 'sum'), want_sum, rtol=0, atol=1e-12)
        np.testing.assert_allclose(R.reduce_ref(feats, ids, m, 'mean'), want_sum / np.maximum(lens, 1)[:, None], rtol=0, atol=1e-12)
        vals, arg = R.reduce_ref(feats, ids, m, 'max')
        np.testing.assert_array_equal(vals, want_max)
        assert np.array_equal(R.group_lens(ids, m), lens)
        # the recorded row: of the group, attains the maximum, and no smaller row of the group does
        for g in range(m):
            rows = np.flatnonzero(ids == g)
            for ch in range(c):
                if rows.size == 0:
                    assert arg[g, ch] == n and vals[g, ch] == 0
                else:
                    col = feats[rows, ch]
                    assert arg[g, ch] == rows[np.flatnonzero(col == col.max())[0]]
        # gradients: autograd of the float64 sum / mean; MAX through the recorded rows
        gout = rng.integers(-8, 9, size=(m, c)).astype(np.float32)
        x = torch.from_numpy(feats).double().requires_grad_(True)
        y = torch.zeros(m, c, dtype=torch.float64).scatter_reduce(0, idx, x[torch.from_numpy(ok)], 'sum')
        y.backward(torch.from_numpy(gout).double())
        np.testing.assert_array_equal(R.grad_ref(gout, ids, n, 'sum'), x.grad.numpy().astype(np.float32))
        got = R.grad_ref(gout, ids, n, 'mean', lens=lens)
        want = np.zeros((n, c), np.float32)
        want[ok] = gout[ids[ok]] / lens[ids[ok]].astype(np.float32)[:, None]
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        gmax = R.grad_ref(gout, ids, n, 'max', arg=arg)
        want = np.zeros((n, c), np.float32)
        for g in range(m):
            for ch in range(c):
                if arg[g, ch] < n:
                    want[arg[g, ch], ch] = gout[g, ch]
        assert np.array_equal(gmax.view(np.int32), want.view(np.int32))


def test_hand_worked_groupings_with_ties():
    nz = np.float32(-0.0)
    # 1. two groups, interleaved rows, ties of the maximum: the smaller row is recorded
    feats = np.array([[1, 5], [2, 5], [2, 0], [1, 7], [2, 5]], np.float32)
    ids = np.array([0, 1, 0, 1, 0])
    vals, arg = R.reduce_ref(feats, ids, 2, 'max')
    assert vals.tolist() == [[2, 5], [2, 7]] and arg.tolist() == [[2, 0], [1, 3]]
    assert R.reduce_ref(feats, ids, 2, 'sum').tolist() == [[5, 10], [3, 12]]
    assert R.expect_f32(feats, ids, 2, 'mean').tolist() == [[np.float32(5) / np.float32(3), np.float32(10) / np.float32(3)], [1.5, 6]]
    g = R.grad_ref(np.array([[10, 20], [30, 40]], np.float32), ids, 5, 'max', arg=arg)
    assert g.tolist() == [[0, 20], [30, 0], [10, 0], [0, 40], [0, 0]]
    # 2. +0.0 and -0.0 tie: the smaller row wins and its sign is the value's; an all -0.0 sum is +0.0; an empty group
    feats = np.array([[nz], [0.0], [nz], [0.0], [nz], [-1.0]], np.float32)
    ids = np.array([0, 0, 2, 2, 3, 3])
    vals, arg = R.expect_f32(feats, ids, 4, 'max')
    assert arg[:, 0].tolist() == [0, 6, 2, 4]
    assert np.signbit(vals[:, 0]).tolist() == [True, False, True, True] and not vals.any()
    s = R.expect_f32(np.full((3, 1), nz), np.zeros(3, np.int64), 1, 'sum')
    assert s[0, 0] == 0 and not np.signbit(s[0, 0])
    assert R.expect_f32(feats, ids, 4, 'mean')[:, 0].tolist() == [0.0, 0.0, 0.0, -0.5]
    assert not np.signbit(R.expect_f32(feats, ids, 4, 'mean')[1, 0])
    # 3. a channel of -inf: the smallest row of the group; all but one: the finite row; rows of no group (-1) are ignored
    inf = np.float32(np.inf)
    feats = np.array([[-inf, -inf], [9, 9], [-inf, 2], [-inf, -inf]], np.float32)
    ids = np.array([0, -1, 0, 0])
    vals, arg = R.expect_f32(feats, ids, 1, 'max')
    assert arg.tolist() == [[0, 2]] and vals.tolist() == [[-inf, 2]]
    g = R.grad_ref(np.array([[3, 4]], np.float32), ids, 4, 'max', arg=arg)
    assert g.tolist() == [[3, 0], [0, 0], [0, 4], [0, 0]]
    assert R.grad_ref(np.array([[3, 4]], np.float32), ids, 4, 'sum').tolist() == [[3, 4], [0, 0], [3, 4], [3, 4]]
    # a row limit: rows at and above it receive and send nothing
    g = R.grad_ref(np.array([[1, 1], [2, 2]], np.float32), np.array([1, 0, 1]), 3, 'sum', limit=1)
    assert g.tolist() == [[0, 0], [1, 1], [0, 0]]


def _tile_cases():
    for c, n_min in R.T_CASES:
        for first in (0, 1):
            for tail in R.T_TAILS:
                yield c, n_min, first, tail, R.tile_lens(c, n_min, first, tail)


def test_tile_shape_equals_the_library_scratch_size():
    lib = _lib()
    seen = set()
    for c, n_min, first, tail, lens in _tile_cases():
        n, m = sum(lens), len(lens) - first
        assert lib.sst_segment_long_scratch_bytes(n, m, c) == R.long_scratch_bytes(c, n, m), (c, n, m)
        seen.add(R.tile_shape(c, n)[1:])
    # the shapes the widths were chosen for: (channel vectors, lanes, tile rows)
    assert seen == {(1, 8, 64), (3, 8, 64), (16, 8, 64), (33, 7, 56), (64, 4, 32), (255, 1, 8), (16, 16, 128), (1, 32, 256)}
    for c in (1, 2, 3, 4, 5, 8, 36, 68, 128, 130, 132, 252, 255, 256):
        for n in (1, 7, 8, 9, 2047, 16383, 16384, 32767, 32768, 65535, 65536, 300000):
            assert lib.sst_segment_long_scratch_bytes(n, 5, c) == R.long_scratch_bytes(c, n, 5), (c, n)


def test_tile_groupings_reach_the_edges_they_name():
    for c, n_min, first, tail, lens in _tile_cases():
        n = sum(lens)
        _, _, Ln, T = R.tile_shape(c, n)
        off = np.concatenate([[0], np.cumsum(lens)])
        beg, end, ln = off[:-1], off[1:], np.asarray(lens)
        assert n >= max(n_min, 8 * (len(lens) - first)) and n % T == {'0': 0, '1': 1, 'T-1': T - 1}[tail]
        assert n < 70000 and (n_min > 0 or n < 32768)
        ones = (ln == 1).astype(int)
        assert max(np.convolve(ones, np.ones(17, int), 'valid')) == 17             # seventeen 1-row groups in a row
        assert ((end % T == 0) & (ln < T) & (beg // T == (end - 1) // T)).any()       # ends on a tile's last row
        assert ((beg % T == 0) & (ln < T)).any()                                     # starts on a tile's first row
        assert ((ln == T) & (beg % T == 0)).any() and ((ln == T) & (beg % T != 0)).any()
        assert (ln == 2 * T + 1).any() and (ln == (Ln + 3) * T).any()
        if first:
            assert lens[0] > T and beg[0] // T != (end[0] - 1) // T


def test_work_list_capacities():
    lib = _lib()
    for n, m, c in [(0, 0, 1), (1, 1, 1), (511, 3, 3), (512, 1, 4), (513, 1, 5), (8056, 1115, 258), (100000, 7, 130)]:
        assert lib.sst_segment_reduce_work_words(n, m, c) == R.work_words(n, m, c), (n, m, c)
    # what the header promises of that size: room for every entry, every cut group and every partial slot of any grouping of n
    # rows in m groups - the groupings of the GPU test, and the worst cases (one group of all rows; as many groups of
    # kSegChunk + 1 rows as fit)
    cases = [R.work_lens(0), R.work_lens(1), R.block_lens(0), [100000], [R.CHUNK + 1] * 50, [R.WORK_LIMIT + 1] * 300]
    cases += [lens for *_, lens in _tile_cases()]
    for lens in cases:
        n, m = sum(lens), len(lens)
        cap_e, cap_m, cap_p, _ = R.work_capacities(n, m, 4)
        entries, cut, slots = R.work_demand(lens)
        assert entries <= cap_e and cut <= cap_m and slots <= cap_p, (n, m)
    assert R.work_demand([32, 33, 512, 513, 1024, 1025]) == (1 + 1 + 2 + 2 + 3, 3, 7)
    # the lists of the work-list and block classes hold every length edge, and keep n below / above 8 m
    for first in (0, 1):
        lens = R.work_lens(first)
        assert sum(lens) < 8 * (len(lens) - first) and set(R.W_LENS) <= set(lens)
        lens = R.block_lens(first)
        assert sum(lens) >= 8 * (len(lens) - first) and set(R.B_LENS) <= set(lens)
        lens = R.block_lens(first, 300)
        assert sum(lens) < 8 * (len(lens) - first)
    assert R.W_LENS == [1, 2, 3, 4, 5, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 1537]
    assert R.B_LENS == [1, 4, 5, 15, 16, 17, 255, 256, 257, 1000]


def test_grouping_is_seeded_and_scattered():
    ids, coors = R.grouping([3, 1, 4, 1, 5], 7)
    ids2, _ = R.grouping([3, 1, 4, 1, 5], 7)
    assert np.array_equal(ids, ids2) and np.bincount(ids).tolist() == [3, 1, 4, 1, 5]
    assert not np.array_equal(ids, np.sort(ids))
    ids, coors = R.grouping([2] * 600, 1)
    assert np.array_equal(coors[:, 1] * 251 + coors[:, 2], ids) and not coors[:, 0].any()
    _, inv = np.unique(coors, axis=0, return_inverse=True)
    assert np.array_equal(inv.reshape(-1), ids)             # the sorted-unique order of the rows is the id order
