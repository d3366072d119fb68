"""GPU: the segmented reduction (kernels.segment_reduce -> csrc/scatter.hip, csrc/seg_tiles.h) with a group on every length
edge of each of its five forward kernel classes, against the plain numpy reference tests/seg_reduce_ref.py:

  T   tiles               seg_tiles_k<4> / <1>                                      plan, n >= 8 m, c <= 256
  W4  work list, float4   seg_reduce_fwd_v4_k + seg_reduce_fwd_work_k<4> + merge     plan, c % 4 == 0, 16-byte aligned rows
  W1  work list, scalar   seg_reduce_fwd_k + seg_reduce_fwd_work_k<1> + merge        plan, c % 4 != 0 or misaligned rows
  B   block               seg_reduce_fwd_v4_k + seg_reduce_fwd_block_k               no work list, c % 4 == 0, n >= 8 m
  S   serial              seg_reduce_fwd_v4_k / seg_reduce_fwd_k alone               no work list, n < 8 m or c % 4 != 0

A class is forced the way the older tests do it (SST_SEG_LONG / SST_SEG_WORK and the shape itself), the precondition that
selects it is asserted, and so is the scratch the call left on the plan (tile counters / work list / none).

Operands are small integers in [-3, 3] with +0.0 / -0.0 sprinkled in: every sum is exact in fp32 in any order and a mean is one
correctly rounded division, so SUM, MEAN, MAX, the arg-max rows and all three gradients are compared BIT FOR BIT
(view(int32): the sign of a zero counts), and the MAX bits must be those of feats[argmax].  One real-valued case per class
checks SUM / MEAN against float64 within the bound of any fp32 summation order (seg_reduce_ref.sum_bound).  Before every call
a NaN block and an int32 block of a valid row index, of the output's size, are freed, so that an output row the kernels do
not write is seen.  After every call the self-cleaning counters are read back, and every call is made twice.

MAX with -inf: a channel that is -inf in every row of a group records the group's smallest row and sends its gradient there.
NaN, and inf - inf in a sum, are outside the contract and not tested."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_reduce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = ('sum', 'mean', 'max')
ENV = {'T': ('1', '1'), 'W4': ('0', '1'), 'W1': ('0', '1'), 'B': ('0', '0'), 'S': ('0', '0')}   # SST_SEG_LONG, SST_SEG_WORK


def same(got, want, what):
    """bit equality (fp32 compared as int32) with a one-line report of the first difference"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    if got.dtype == np.float32:
        a, b = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32)
    else:
        a, b = got.astype(np.int64), want.astype(np.int64)
    bad = np.argwhere(a != b)
    if bad.shape[0]:
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f'{what}: {bad.shape[0]} of {a.size} elements differ, first at {at}: got {got[at]!r}, want {want[at]!r}')


def make_plan(lens, seed):
    from sst_amd import kernels as K
    ids, coors = R.grouping(lens, seed)
    plan = K.unique_rows(torch.from_numpy(coors).to(DEV))
    assert plan.m == len(lens) and plan.native
    return ids, plan


def device_feats(x, misaligned=False):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    if not misaligned:
        return t
    n, c = t.shape
    base = torch.empty(n * c + 1, dtype=torch.float32, device=DEV)
    view = base[1:].view(n, c)          # contiguous, rows 4 bytes off a 16-byte boundary
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def make_gout(m, c, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(-8, 9, size=(m, c)).astype(np.float32)
    g[rng.random((m, c)) < 0.05] = -0.0
    return g


def check_scratch(cls, plan, n, m, c):
    """the class left its own scratch on the plan and nothing else, and the counters cleaned themselves (read on the device)"""
    scratch = getattr(plan, 'scratch', None) or {}
    work = [k for k in scratch if k[0] == 'work']
    if cls == 'T':
        assert (n, m, c) in scratch and not work, f'class T expected, scratch keys {list(scratch)}'
        assert int(scratch[(n, m, c)][:4 * m].count_nonzero()) == 0, 'tile ticket counters not zero after the call'
    elif cls in ('W4', 'W1'):
        assert len(work) == 1 and work[0][2] == (c + 3) // 4 and len(scratch) == 1, f'class {cls} expected, scratch keys {list(scratch)}'
        hdr = scratch[work[0]][:6]
        assert int(hdr.count_nonzero()) == 0, f'work list header not zero after the call: {hdr.tolist()}'
    else:
        assert not scratch, f'class {cls} expected, scratch keys {list(scratch)}'


def run(cls, monkeypatch, x, plan, mode, gout, first=0, **kw):
    """one forward + backward of kernels.segment_reduce in kernel class `cls`: (values, arg-max rows or None, gradient)"""
    from sst_amd import kernels as K
    monkeypatch.setenv('SST_SEG_LONG', ENV[cls][0])
    monkeypatch.setenv('SST_SEG_WORK', ENV[cls][1])
    n, c = x.shape
    subset = 'group_index' in kw
    m = kw['group_index'].numel() if subset else plan.m - first
    aligned = x.data_ptr() % 16 == 0
    assert x.is_contiguous()
    if cls == 'T':
        assert not subset and n >= 8 * m and c <= 256 and (c % 4 != 0 or aligned)
    elif cls == 'W4':
        assert c % 4 == 0 and aligned
    elif cls == 'W1':
        assert c % 4 != 0 or not aligned
    elif cls == 'B':
        assert not subset and c % 4 == 0 and aligned and n >= 8 * m
    else:
        assert c % 4 != 0 or not aligned or n < 8 * m
    x = x.detach().requires_grad_(True)
    # a row that is not written shows: the blocks the outputs are about to be given hold NaN / a valid row index
    p, q = torch.full((m, c), float('nan'), device=DEV), torch.full((m, c), 1, dtype=torch.int32, device=DEV)
    del p, q
    y = K.segment_reduce(x, plan, mode, first=first, **kw)
    arg = y.grad_fn.saved_tensors[2].cpu().numpy() if mode == 'max' else None
    y.backward(torch.from_numpy(gout).to(DEV))
    check_scratch(cls, plan, n, m, c)
    return y.detach().cpu().numpy(), arg, x.grad.cpu().numpy()


def check_exact(cls, monkeypatch, x_np, ids, plan, first=0, misaligned=False, modes=MODES, seed=0):
    """every mode of one grouping in one class against the reference, bit for bit, twice"""
    n, c = x_np.shape
    m = plan.m - first
    rows = ids - first
    lens = R.group_lens(rows, m)
    x = device_feats(x_np, misaligned)
    gout = make_gout(m, c, seed + 17)
    pad = np.concatenate([x_np, np.zeros((1, c), np.float32)])
    for mode in modes:
        y, arg, g = run(cls, monkeypatch, x, plan, mode, gout, first)
        what = f'{cls} c={c} n={n} m={m} first={first} {mode}'
        want_arg = None
        if mode == 'max':
            want, want_arg = R.expect_f32(x_np, rows, m, 'max')
            same(arg, want_arg, what + ' arg-max rows')
            same(y, np.take_along_axis(pad, arg.astype(np.int64), 0), what + ' values against feats[argmax]')
        else:
            want = R.expect_f32(x_np, rows, m, mode)
        same(y, want, what + ' values')
        same(g, R.grad_ref(gout, rows, n, mode, arg=want_arg, lens=lens), what + ' gradient')
        y2, arg2, g2 = run(cls, monkeypatch, x, plan, mode, gout, first)
        same(y2, y, what + ' values of the second call')
        same(g2, g, what + ' gradient of the second call')
        if mode == 'max':
            same(arg2, arg, what + ' arg-max rows of the second call')


def with_neg_inf(x, ids, k):
    """channels 0 and c - 1: -inf in every row of a third of the groups, in all rows but a middle one of another third"""
    x = x.copy()
    order, lens, starts = R._csr(ids, k)
    full = np.flatnonzero(lens > 0)
    mid = np.full(k, -1, np.int64)
    mid[full] = order[starts[full] + lens[full] // 2]
    for ch, shift in ((0, 0), (x.shape[1] - 1, 1)):
        kind = (np.arange(k) + shift) % 3
        keep = mid[(kind == 1) & (lens > 0)]
        kept = x[keep, ch].copy()
        x[kind[ids] != 2, ch] = -np.inf
        x[keep, ch] = kept
    return x


# ---- the work-list classes ----------------------------------------------------------------------------------------------
W_CASES = [('W4', c, False) for c in R.W4_WIDTHS] + [('W1', c, False) for c in R.W1_WIDTHS] + [('W1', 64, True)]


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('cls,c,misaligned', W_CASES)
def test_work_list_classes_at_the_chunk_edges(cls, c, misaligned, first, monkeypatch):
    """groups of 1 .. 33 rows (the limit of the element kernels is 32), 511 / 512 / 513, 1023 / 1024 / 1025 and 1537 rows (chunks
    of 512) among 1100 single rows (n < 8 m); widths with partly live lane groups (36, 68), a second 256-channel pass (257,
    258) and a misaligned [n, 64] view, which drops from the float4 to the scalar kernels"""
    lens = R.work_lens(first)
    ids, plan = make_plan(lens, 100 + c)
    assert ids.size < 8 * (plan.m - first)
    check_exact(cls, monkeypatch, R.exact_feats(ids.size, c, c + first), ids, plan, first, misaligned, seed=c)


# ---- the classes without a work list --------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('cls,c', [('B', c) for c in R.B_WIDTHS] + [('S', c) for c in R.S_WIDTHS])
def test_block_and_serial_classes_at_their_edges(cls, c, first, monkeypatch):
    """groups of 1 .. 17 rows (the limit of the thread-per-element kernel beside the block kernel is 16), 255 / 256 / 257 (the
    row parts of a workgroup) and 1000 rows; S: the same groups among 300 single rows (n < 8 m)"""
    lens = R.block_lens(first, 300 if cls == 'S' else 0)
    ids, plan = make_plan(lens, 200 + c)
    check_exact(cls, monkeypatch, R.exact_feats(ids.size, c, c + first), ids, plan, first, seed=c)


# ---- the tiles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tail', R.T_TAILS)
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('c,n_min', R.T_CASES)
def test_tiles_at_the_tile_edges(c, n_min, first, tail, monkeypatch):
    """seg_reduce_ref.tile_lens: seventeen 1-row groups in a row, groups that end on a tile's last row / start on its first,
    a group of exactly one tile (aligned and not), of 2 T + 1 rows and of (lanes + 3) T rows (the strided loop of
    seg_tile_finish), and n % T in {0, 1, T - 1}; first = 1: the discarded group 0 is long and crosses a tile"""
    lens = R.tile_lens(c, n_min, first, tail)
    ids, plan = make_plan(lens, 300 + c + len(tail))
    check_exact('T', monkeypatch, R.exact_feats(ids.size, c, c + first), ids, plan, first, seed=c)


# ---- -inf -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('cls,c,misaligned', [('T', 64, False), ('T', 3, False), ('W4', 36, False), ('W1', 5, False),
                                              ('W1', 64, True), ('B', 36, False), ('S', 3, False), ('S', 64, False)])
def test_max_of_a_channel_that_is_minus_infinity(cls, c, misaligned, first, monkeypatch):
    """a channel that is -inf in every row of a group: the smallest row of the group is recorded and receives the gradient;
    -inf in all rows but one: the finite row.  MAX only; NaN stays outside the contract."""
    if cls == 'T':
        lens = R.tile_lens(c, 0, first, '1')
    elif cls in ('W4', 'W1'):
        lens = R.work_lens(first)
    else:
        lens = R.block_lens(first, 300 if cls == 'S' else 0)
    ids, plan = make_plan(lens, 400 + c)
    x_np = with_neg_inf(R.exact_feats(ids.size, c, c), ids, len(lens))
    assert np.isneginf(x_np).any()
    check_exact(cls, monkeypatch, x_np, ids, plan, first, misaligned, modes=('max',), seed=c)


# ---- groups without rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls,c,dense,misaligned', [('T', 64, True, False), ('T', 3, True, False), ('W4', 64, True, False),
                                                    ('W1', 5, True, False), ('B', 64, True, False), ('S', 5, True, False),
                                                    ('W4', 64, False, False), ('W1', 64, False, True), ('S', 64, False, False)])
def test_groups_without_rows_read_zero(cls, c, dense, misaligned, monkeypatch):
    """the scatter_v2(..., unq_inv=, new_coors=) form on a slice of the points: sst_ops.plan_of_inverse keeps a group for every
    id, absent ids included.  Their rows are 0, their arg-max is n and they send no gradient, in every class, at n >= 8 m
    (dense) and below."""
    from sst_amd import sst_ops
    lens = R.block_lens(0, 0 if dense else 300) + [7]
    k = len(lens)
    for g in (0, 3, 4, 8 if not dense else 5, k - 1):      # the first, two neighbours, one in the middle, the last
        lens[g] = 0
    ids, _ = R.grouping(lens, 500 + c)
    n = ids.size
    assert (n >= 8 * k) == dense
    unq_inv = torch.from_numpy(ids).to(DEV)
    plan = sst_ops.plan_of_inverse(unq_inv, k)
    assert plan.m == k and not getattr(plan, 'native', False)
    np.testing.assert_array_equal(plan.counts().cpu().numpy(), lens)
    x_np = R.exact_feats(n, c, c)
    check_exact(cls, monkeypatch, x_np, ids, plan, 0, misaligned, seed=c)
    if cls in ('W4', 'W1'):
        from sst_amd import kernels as K
        val, arg = K.segment_argmax(device_feats(x_np, misaligned), plan)
        want, want_arg = R.expect_f32(x_np, ids, k, 'max')
        same(val.cpu().numpy(), want, 'segment_argmax values')
        same(arg.cpu().numpy(), want_arg, 'segment_argmax rows')


# ---- group_index / m_limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls,c,misaligned', [('W4', 36, False), ('W4', 256, False), ('W1', 5, False), ('W1', 257, False),
                                              ('W1', 64, True)])
def test_subset_of_the_groups_with_a_device_row_limit(cls, c, misaligned, monkeypatch):
    """group_index: a permuted subset of the groups with a few negative entries (empty rows: 0, arg-max n); m_limit on the
    device below group_index.numel(): rows at and above it are neither written nor given a gradient"""
    from sst_amd import _lib
    lens = R.work_lens(0)
    ids, plan = make_plan(lens, 600 + c)
    n, k = ids.size, len(lens)
    rng = np.random.default_rng(c)
    long_groups = np.flatnonzero(np.asarray(lens) > 1)
    short = rng.permutation(np.flatnonzero(np.asarray(lens) == 1))[:600]
    gidx = rng.permutation(np.concatenate([long_groups[1:], short]))       # one long group is left out
    gidx[[1, 77, gidx.size - 20, gidx.size - 2]] = -1
    m2, limit = gidx.size, gidx.size - 9
    row_of_group = np.full(k, -1, np.int64)
    row_of_group[gidx[gidx >= 0]] = np.flatnonzero(gidx >= 0)
    rows = row_of_group[ids]
    lens_of_row = R.group_lens(rows, m2)
    below = np.where(rows < limit, rows, -1)
    kw = dict(group_index=torch.from_numpy(gidx.astype(np.int32)).to(DEV), inverse=torch.from_numpy(rows.astype(np.int32)).to(DEV),
              m_limit=torch.tensor([limit], dtype=torch.int32).to(DEV))
    x_np = R.exact_feats(n, c, c)
    x = device_feats(x_np, misaligned)
    gout = make_gout(m2, c, c)
    for mode in MODES:
        what = f'{cls} c={c} subset {mode}'
        y, arg, g = run(cls, monkeypatch, x, plan, mode, gout, **kw)
        want_arg = None
        if mode == 'max':
            want, want_arg = R.expect_f32(x_np, below, limit, 'max')
            same(arg[:limit], want_arg, what + ' arg-max rows')
        else:
            want = R.expect_f32(x_np, below, limit, mode)
        same(y[:limit], want, what + ' values')
        same(g, R.grad_ref(gout, rows, n, mode, arg=want_arg, lens=lens_of_row, limit=limit), what + ' gradient')
        y2, _, g2 = run(cls, monkeypatch, x, plan, mode, gout, **kw)
        same(y2[:limit], y[:limit], what + ' values of the second call')
        same(g2, g, what + ' gradient of the second call')
    # rows at and above the limit are left as they were: the C entry on pre-filled buffers
    lib = _lib.load()
    out = torch.full((m2, c), 12345.0, device=DEV)
    argm = torch.full((m2, c), -7, dtype=torch.int32, device=DEV)
    work, = [v for key, v in plan.scratch.items() if key[0] == 'work']
    rc = lib.sst_segment_reduce_fwd_work_f32(_lib.ptr(x), n, c, _lib.ptr(plan.perm), _lib.ptr(plan.offsets), _lib.ptr(kw['group_index']),
                                             m2, 2, _lib.ptr(out), _lib.ptr(argm), _lib.ptr(kw['m_limit']), _lib.ptr(work),
                                             work.numel(), None, None, _lib.stream_ptr())
    assert rc == 0
    want, want_arg = R.expect_f32(x_np, below, limit, 'max')
    same(out.cpu().numpy(), np.concatenate([want, np.full((9, c), 12345.0, np.float32)]), 'values with untouched rows')
    same(argm.cpu().numpy(), np.concatenate([want_arg, np.full((9, c), -7)]), 'arg-max rows with untouched rows')
    assert int(work[:6].count_nonzero()) == 0


# ---- the pooled BatchNorm + ReLU --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [36, 68])
def test_scale_shift_relu_on_the_work_list(c, monkeypatch):
    """values read as relu(x * scale + shift): scales are powers of two and shifts small integers, so the expression is exact
    whether or not it is contracted; a quarter of the groups is negative in every row before the ReLU, which ties the maximum
    at 0 over the whole group"""
    from sst_amd import kernels as K
    monkeypatch.setenv('SST_SEG_LONG', '0')
    monkeypatch.setenv('SST_SEG_WORK', '1')
    lens = R.work_lens(0)
    ids, plan = make_plan(lens, 700 + c)
    n, m = ids.size, len(lens)
    rng = np.random.default_rng(c)
    x_np = R.exact_feats(n, c, c)
    x_np[ids % 4 == 0] = -3.0
    scale = rng.choice([0.5, 1.0, 2.0, 4.0], size=c).astype(np.float32)
    shift = rng.integers(-2, 2, size=c).astype(np.float32)
    t = x_np.astype(np.float64) * scale + shift
    act = np.where(t > 0, t, 0.0).astype(np.float32)
    assert (act[ids % 4 == 0] == 0).all() and np.array_equal(act.astype(np.float64), np.where(t > 0, t, 0.0))
    x = device_feats(x_np)
    ss = (torch.from_numpy(scale).to(DEV), torch.from_numpy(shift).to(DEV))
    assert x.data_ptr() % 16 == 0 and ss[0].data_ptr() % 16 == 0 and ss[1].data_ptr() % 16 == 0
    for mode in MODES:
        got = [K._segment_reduce_fwd(x, plan.perm, plan.offsets, m, K.REDUCE[mode], mode == 'max', plan=plan, scale_shift=ss)
               for _ in range(2)]
        check_scratch('W4', plan, n, m, c)
        y, arg = got[0]
        if mode == 'max':
            want, want_arg = R.expect_f32(act, ids, m, 'max')
            same(arg.cpu().numpy(), want_arg, f'scale_shift c={c} arg-max rows')
            same(got[1][1].cpu().numpy(), want_arg, f'scale_shift c={c} arg-max rows of the second call')
        else:
            want = R.expect_f32(act, ids, m, mode)
        same(y.cpu().numpy(), want, f'scale_shift c={c} {mode} values')
        same(got[1][0].cpu().numpy(), want, f'scale_shift c={c} {mode} values of the second call')


# ---- real values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls,c,misaligned', [('T', 64, False), ('W4', 68, False), ('W1', 5, False), ('B', 36, False),
                                              ('S', 3, False)])
def test_real_valued_sums_within_the_bound_of_any_summation_order(cls, c, misaligned, monkeypatch):
    """standard normal values: |fl(sum) - sum| <= gamma_len sum |x_i| (gamma_k = k u / (1 - k u), u = 2^-24) holds for every
    association of the fp32 additions; the mean adds the division's u |mean|.  float64 is the reference."""
    if cls == 'T':
        lens = R.tile_lens(c, 0, 0, '1')
    elif cls in ('W4', 'W1'):
        lens = R.work_lens(0)
    else:
        lens = R.block_lens(0, 300 if cls == 'S' else 0)
    ids, plan = make_plan(lens, 800 + c)
    n, m = ids.size, len(lens)
    x_np = np.random.default_rng(c).standard_normal((n, c)).astype(np.float32)
    x = device_feats(x_np, misaligned)
    gout = make_gout(m, c, c)
    b_sum, b_mean = R.sum_bound(x_np, ids, m)
    for mode, bound in (('sum', b_sum), ('mean', b_mean)):
        y, _, _ = run(cls, monkeypatch, x, plan, mode, gout)
        err = np.abs(y.astype(np.float64) - R.reduce_ref(x_np.astype(np.float64), ids, m, mode))
        assert (bound > 0).all()
        worst = np.unravel_index(np.argmax(err / bound), err.shape)
        print(f'{cls} c={c} {mode}: largest error {err.max():.3e}; closest to its bound: {err[worst]:.3e} of {bound[worst]:.3e}')
        assert (err <= bound).all(), f'{cls} c={c} {mode}: error {err[worst]:.3e} above the bound {bound[worst]:.3e} at {worst}'


# ---- the classes against each other -----------------------------------------------------------------------------------------
def test_the_five_classes_agree_bit_for_bit(monkeypatch):
    """one grouping every class accepts (c = 64, n >= 8 m; the scalar classes through a misaligned view): values, arg-max rows
    and gradients of all three modes are the same bits in all five"""
    c = 64
    lens = R.tile_lens(c, 0, 0, '1')
    x_np = with_neg_inf(R.exact_feats(sum(lens), c, 5), R.grouping(lens, 900)[0], len(lens))
    res = {}
    for cls, misaligned in (('T', False), ('W4', False), ('W1', True), ('B', False), ('S', True)):
        ids, plan = make_plan(lens, 900)
        x = device_feats(x_np, misaligned)
        gout = make_gout(len(lens), c, 3)
        x_mode = {'max': x, 'sum': device_feats(np.where(np.isneginf(x_np), np.float32(1.0), x_np), misaligned)}
        res[cls] = {mode: run(cls, monkeypatch, x_mode.get(mode, x_mode['sum']), plan, mode, gout) for mode in MODES}
    for cls in ('W4', 'W1', 'B', 'S'):
        for mode in MODES:
            for got, want, what in zip(res[cls][mode], res['T'][mode], ('values', 'arg-max rows', 'gradient')):
                if want is not None:
                    same(got, want, f'{cls} against T, {mode} {what}')
