"""GPU: the two loops of the exact-split weight-gradient kernel (csrc/wgrad_x6.hip) - the lean steady-state loop (no row clamp,
no `t < t_end` mask, scalar base + lane offset addressing) and the general loop that ends every slice - at the token counts
where a workgroup changes from one to the other, bit for bit.

The sweeps of tests/test_gpu_wgrad_edges.py (m = 1 .. 130 and 4090 .. 4230) give most slices one step, five at most: a loop
that needs its requests kPf + 2 steps ahead inside [0, m) is barely reached there.  Here the boundaries come from the library's
own plan (sst_weight_grad_group_f32x6_plan: the function the launch uses):
    m = slices * 32 * s + d,   s in {3, 4, 5, 6},   d in {-33, -32, -31, -1, 0, 1, 31, 32, 33}
- both parities of the two-set register ring, the last slice full, partial, or one step long, and in every shape slices that
run the lean loop beside slices that do not (asserted: a test that silently ran one loop only would hide a failure) - and the
smallest m whose plan has a lean slice at all, with m - 1 (which has none).  A slice is lean only with three steps or more, so
the lean-slice count jumps from 0 to several there; a shape with exactly one lean slice does not exist under this plan.

Operands are the exact recipes of test_gpu_wgrad_edges.py (its helpers are imported, every comparison is `==` against
float64): A at every m, B (either side fine) up to its cap of 4300 rows.  Recipe D's cap (130 rows) lies below the smallest m
with a lean slice (2049), so no m of this file is within it.

Out-of-range reads: every operand is the leading rows of a buffer whose rows at and beyond m are NaN, the index of the
positional rows continues with entries that point at a NaN row of the table, and the table's unused rows are NaN.  dW and db
are windows of sentinel-filled buffers whose surroundings are compared afterwards.

Groups: the five-problem layer group (8 tiles; q | k with positional rows added on load), a two-problem group (384 x 128 and
512 x 128: 7 tiles) with / without bias gradient and with / without positional rows, and a single 128 x 128 problem at the
layer group's token counts - one tile has 2 steps per slice at most below 7 000 rows, i.e. no lean slice: the general loop on
its own, many slices."""
import ctypes
import functools

import pytest
import torch

from test_gpu_wgrad_edges import (DEV, M_CAP, NAN, P_ROWS, SENTINEL, _Layer, _Prob, _Tally, _assert_exact, _layer, _problem_array,
                                  _values)

pytestmark = pytest.mark.gpu
PAD = 256                   # NaN rows behind the m rows of every operand (the ring requests at most 4 steps = 128 rows ahead)
S_VALUES = (3, 4, 5, 6)
D_VALUES = (-33, -32, -31, -1, 0, 1, 31, 32, 33)
ROWS_A = 6400               # rows of the pre-generated recipe-A operands: 32 slices * 32 * 6 + 33 and a margin
M_LIMIT = 7000
ENTRY = 'sst_weight_grad_group_f32x6'


def _plan(arr, n):
    """(tiles, slices, tokens_per_slice, lean_slices) of a problem array, from the library"""
    from sst_amd import _lib
    t, s, tps, lean = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()
    rc = _lib.load().sst_weight_grad_group_f32x6_plan(arr, n, ctypes.byref(t), ctypes.byref(s), ctypes.byref(tps), ctypes.byref(lean))
    assert rc == 0, rc
    return t.value, s.value, tps.value, lean.value


@functools.lru_cache(maxsize=None)
def _base(recipe, fine):
    """pre-generated operands: recipe A with ROWS_A rows, recipe B the layer of test_gpu_wgrad_edges.py (shared with it);
    + a 512-column dy of the two-problem group"""
    L = _Layer('A', 'dy', ROWS_A, seed=5) if recipe == 'A' else _layer(recipe, fine)
    rows = L.ds1.size(0)
    gen = torch.Generator(device=DEV).manual_seed(512 + ord(recipe) + (7 if fine == 'x' else 0))
    return L, _values(recipe, fine == 'dy', (rows, 512), gen)


def _padded(t, m):
    """the rows [:m] of t as a view of a buffer that goes on with PAD rows of NaN"""
    buf = torch.full((m + PAD,) + tuple(t.shape[1:]), NAN, device=DEV)
    buf[:m] = t[:m]
    return buf[:m]


def _padded_xadd(L, m):
    """(table with 8 NaN rows behind its P_ROWS, index [:m] of a buffer whose later entries point at the first NaN row)"""
    table = torch.full((P_ROWS + 8, L.table.size(1)), NAN, device=DEV)
    table[:P_ROWS] = L.table
    index = torch.full((m + PAD,), P_ROWS, dtype=torch.int32, device=DEV)
    index[:m] = L.index[:m]
    return table, index[:m]


def _groups(recipe, fine, m):
    """{name: [problems]} on NaN-padded copies of the first m rows"""
    L, dy512 = _base(recipe, fine)
    P = lambda t: _padded(t, m)                                    # noqa: E731
    dqkv, xadd = P(L.dqkv), _padded_xadd(L, m)
    ds1, o, x, xq, xp = P(L.ds1), P(L.o), P(L.x), P(L.xq), P(L.xp)
    wo = _Prob(ds1, o)
    five = [_Prob(P(L.ds2), P(L.h)), _Prob(P(L.dpre), P(L.y1)), wo, _Prob(dqkv[:, :256], xq, xadd), _Prob(dqkv[:, 256:], x)]
    out = {'layer group': five, 'single 128x128': [wo]}
    d512 = P(dy512)
    for bias in (True, False):
        for pos in (True, False):
            if recipe != 'A' and not (bias and pos):            # the four variants on recipe A, the fullest one on B as well
                continue
            first = _Prob(dqkv, xq, xadd, bias=bias) if pos else _Prob(dqkv, xp, bias=bias)
            out['two problems, bias=%d positional=%d' % (bias, pos)] = [first, _Prob(d512, o, bias=bias)]
    return out


def _run(probs, m, tally, what):
    """the C entry on windows of sentinel-filled destinations; exact results inside, the sentinel outside -> the plan"""
    from sst_amd import _lib
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=DEV)
    bigs = [(torch.full((p.out + 16, p.inn), SENTINEL, **f32), torch.full((p.out + 16,), SENTINEL, **f32)) for p in probs]
    dests = [(bw[8:8 + p.out], bb[8:8 + p.out] if p.bias else None) for p, (bw, bb) in zip(probs, bigs)]
    arr = _problem_array(probs, m, dests)
    need = lib.sst_weight_grad_group_f32x6_workspace_bytes(arr, len(probs))
    assert need > 0, (what, m, need)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = getattr(lib, ENTRY)(arr, len(probs), _lib.ptr(ws), _lib.stream_ptr())
    assert rc == 0, (what, m, rc)
    for i, (p, got, (bw, bb)) in enumerate(zip(probs, dests, bigs)):
        tally.check(got, p.want(m), m, '%s problem %d (%d x %d)' % (what, i, p.out, p.inn))
        outside = [bw[:8], bw[8 + p.out:], bb[:8], bb[8 + p.out:]] + ([] if p.bias else [bb])
        for t in outside:
            tally.check((t,), (torch.full_like(t, SENTINEL).double(),), m, '%s problem %d surroundings' % (what, i))
    return _plan(arr, len(probs))


def _recipes(m):
    return [r for r in (('A', 'dy'), ('B', 'dy'), ('B', 'x')) if m <= min(M_CAP[r[0]], _base(*r)[0].ds1.size(0))]


def _layer_group_slices():
    """the slice count of the 8- and 7-tile groups at the token counts of this file (constant there), from the library"""
    probs = _groups('A', 'dy', 4096)['layer group']
    return _plan(_problem_array(probs, 4096, [p.dest() for p in probs]), len(probs))[1]


@pytest.mark.parametrize('s', S_VALUES)
def test_boundaries_between_the_lean_and_the_general_loop(s):
    slices = _layer_group_slices()
    tally = _Tally()
    for d in D_VALUES:
        m = slices * 32 * s + d
        assert m < M_LIMIT
        for recipe, fine in _recipes(m):
            for name, probs in _groups(recipe, fine, m).items():
                _assert_exact(recipe, m, probs)
                what = '%s %s/%s' % (name, recipe, fine)
                tiles, n_slices, tps, lean = _run(probs, m, tally, what)
                print('m=%d s=%d d=%+d %s: tiles %d slices %d tokens/slice %d lean %d' % (m, s, d, what, tiles, n_slices, tps, lean))
                assert tps % 32 == 0 and n_slices * tps >= m
                if name == 'single 128x128':
                    continue
                # both loops run: lean slices, and behind them at least one slice that holds tokens and is not lean
                assert n_slices == slices and 1 <= lean < n_slices and lean * tps < m, (what, m, n_slices, tps, lean)
                assert tps // 32 in (s, s + 1)
    tally.finish()


def test_smallest_token_count_with_a_lean_slice():
    """the smallest m at which the layer group's plan has a lean slice, and m - 1 (none): found by asking the plan"""
    probs = _groups('A', 'dy', 4096)['layer group']
    arr = _problem_array(probs, 4096, [p.dest() for p in probs])      # host-side query only: m is varied in place
    first = None
    for m in range(1, 4097):
        for q in arr:
            q.m = m
        if _plan(arr, 5)[3] > 0:
            first = m
            break
    assert first is not None and first > 1
    tally = _Tally()
    leans = {}
    for m in (first - 1, first):
        for recipe, fine in _recipes(m):
            for name, probs in _groups(recipe, fine, m).items():
                _assert_exact(recipe, m, probs)
                plan = _run(probs, m, tally, '%s %s/%s' % (name, recipe, fine))
                print('m=%d %s %s/%s: tiles %d slices %d tokens/slice %d lean %d' % ((m, name, recipe, fine) + plan))
                if name == 'layer group':
                    leans[m] = plan[3]
    tally.finish()
    assert leans[first - 1] == 0 and leans[first] >= 1, leans
