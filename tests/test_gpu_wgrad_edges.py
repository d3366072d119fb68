"""GPU: the weight / bias gradient kernels (csrc/wgrad.hip, csrc/wgrad_x6.hip, the bf16 group of csrc/dense_bf16.hip) token by
token, with EXACT operands.

dW = dY^T X and db = colsum(dY) are sums over the tokens.  When every product and every partial sum of them is a multiple of
one granule and stays below 2^24 granules, each of them is an fp32 number: a correct kernel then returns the float64 result bit
for bit whatever its summation order, its split into slices or its split of the operands into bf16 parts, and one token or
column that is dropped, doubled, swapped or misplaced changes the result.  So every comparison below is `==`, tolerance zero,
and the sweeps run EVERY token count of a range at least twice as wide as the 32- / 64-token steps of the kernels (slice tails,
the last 4-token quad, empty trailing slices) without a copy of any launch plan.

Recipes (`_values`):
  A  dy, x integers in [-4, 4]                                                  (m up to 2^19; every kernel, bf16 included)
  B  one operand in {-1, 0, 1}, the other k / 1024, |k| <= 2047: 12 significant bits = two non-zero bf16 parts (m <= 4300)
  C  one operand in {-1, 0, 1}, the other k / 2^17, |k| < 2^17: 17 bits, which still are TWO non-zero bf16 parts - under
     round-to-nearest each part gains nine bits (eight and the sign of the remainder); none of the 262 143 values has a
     third part (tests/test_spconv_exact_host.py)                                                                 (m <= 64)
  D  one operand k / 2^20, |k| < 2^20: three non-zero bf16 parts in half of the entries; the other in {-1, 0, 1} with at most
     4 non-zero tokens in any column of it, so that at most 4 terms reach an element of dW at any m               (m <= 130)
     With the fine operand on the dy side db would be a sum of m fine values (exact only for m < 8): those problems carry no
     bias gradient.  The recipe that notices a dropped or misplaced x2 w0 / x0 w2 product or third LDS image.
B, C and D are exact in the exact-split mode because the unit operand has one part and every product d_i x_0, i <= 2, is kept.
The caps of B and C are half of what the condition allows: the leading bf16 part of a value rounds up to at most twice it; D
asserts the sum of the absolute products themselves, below 2^23 granules."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
SENTINEL = -12345.5
P_ROWS = 144                               # rows of the positional table
M_SWEEP = 4230                             # rows of the pre-generated operands the sweeps cut their prefixes from
SWEEP_A = range(1, 131)                    # C entries, no gate
SWEEP_B = range(4090, 4231)                # across the Python gate at 4096 rows
GRANULE = {'A': 1.0, 'B': 2.0 ** -10, 'C': 2.0 ** -17, 'D': 2.0 ** -20}
M_CAP = {'A': 1 << 19, 'B': 4300, 'C': 64, 'D': 130}
RECIPES_B = [('A', 'dy'), ('B', 'dy'), ('B', 'x')]      # (recipe, the many-valued side): B both ways round
RECIPES_C = [('A', 'dy'), ('C', 'dy'), ('C', 'x'), ('D', 'dy'), ('D', 'x')]


# ------------------------------------------------------------------------------------------------------------------------------
# exact operands
# ------------------------------------------------------------------------------------------------------------------------------
def _values(recipe, fine, shape, gen, part=None):
    """fp32 [shape] of the recipe: `fine` = this operand is the many-valued one (else the unit one; recipe A has one kind).
    part 'x' / 'table': the two summands of an "x + table[index]" operand whose SUM is a value of the recipe.  Every entry is
    drawn on its own from the seeded generator: no two rows or columns alike, zeros and both signs everywhere."""
    ri = lambda lo, hi: torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()     # noqa: E731
    if recipe == 'A':
        return ri(-4, 4)
    if recipe == 'D' and not fine and part is None:
        return _unit_d(shape, gen)
    scale = {'B': 1024.0, 'C': 2.0 ** 17, 'D': 2.0 ** 20}[recipe]
    top = {'B': 2047, 'C': 2 ** 17 - 1, 'D': 2 ** 20 - 1}[recipe]
    if part is None:
        return ri(-top, top) / scale if fine else ri(-1, 1)
    if fine:
        return (ri(-(top // 2), top // 2) if part == 'x' else ri(-(top // 2) - 1, top // 2 + 1)) / scale
    return ri(0, 1) if part == 'x' else ri(-1, 0)


def _unit_d(shape, gen):
    """the unit operand of recipe D: [rows, cols] of {-1, 0, 1} with 4 non-zero tokens (fewer than 4 rows: all of them) in
    every column, at rows drawn per column"""
    rows, cols = shape
    t = torch.zeros(shape, device=DEV)
    at = torch.rand(shape, generator=gen, device=DEV).argsort(0)[:4]
    sign = torch.randint(0, 2, at.shape, generator=gen, device=DEV).float() * 2 - 1
    return t.scatter_(0, at, sign)


class _Prob:
    """one problem dW[out, in] = dy^T xs, db = colsum(dy) on the rows [:m] of pre-generated operands, xs = x or
    x + table[index]; keeps the float64 operands of the reference and the largest magnitudes for the exactness condition"""

    def __init__(self, dy, x, xadd=None, bias=True, rows=None):
        self.dy, self.x, self.xadd, self.bias, self.rows = dy, x, xadd, bias, rows
        self.xs = x if xadd is None else x + xadd[0][xadd[1].long()]
        self.dyd, self.xd = self.dy.double(), self.xs.double()
        self.dy_max, self.x_max = float(dy.abs().max()), float(self.xs.abs().max())
        self.out, self.inn = dy.size(1), x.size(1)

    def m_of(self, m):
        return m if self.rows is None else min(m, self.rows)

    def want(self, m):
        m = self.m_of(m)
        return self.dyd[:m].t() @ self.xd[:m], (self.dyd[:m].sum(0) if self.bias else None)

    def dest(self):
        return (torch.full((self.out, self.inn), NAN, device=DEV), torch.full((self.out,), NAN, device=DEV) if self.bias else None)

    def wrapper_args(self, m, dw, db, materialised=False):
        m = self.m_of(m)
        if self.xadd is None:
            return (self.dy[:m], self.x[:m], dw, db)
        if materialised:
            return (self.dy[:m], self.xs[:m], dw, db)
        return (self.dy[:m], self.x[:m], dw, db, (self.xadd[0], self.xadd[1][:m]))


def _assert_exact(recipe, m, probs):
    """the condition under which every partial sum is an fp32 number - before anything is launched"""
    assert 1 <= m <= M_CAP[recipe], (recipe, m)
    if recipe == 'D':               # no bound from m: the absolute products themselves, summed
        for p in probs:
            mm = p.m_of(m)
            assert float((p.dyd[:mm].abs().t() @ p.xd[:mm].abs()).max()) / GRANULE['D'] < 2 ** 23, (m, p.out, p.inn)
            assert not p.bias or float(p.dyd[:mm].abs().sum(0).max()) / GRANULE['D'] < 2 ** 23, (m, p.out)
        return
    for p in probs:
        assert m * p.dy_max * p.x_max / GRANULE[recipe] < 2 ** 24, (recipe, m, p.dy_max, p.x_max)
        assert m * p.dy_max / GRANULE[recipe] < 2 ** 24


class _Layer:
    """operands of the five parameter gradients of an encoder layer as its backward pass groups them: (ds2, h) (dpre, y1) |
    (ds1, o) (dqkv[:, :256], xp) (dqkv[:, 256:], x), the last two as column views of one [M, 384] buffer; `pos`: the fourth
    problem reads xq + table[index] instead of xp"""

    def __init__(self, recipe, fine, rows, seed=0, gaussian=False, bias=True):
        gen = torch.Generator(device=DEV).manual_seed(1000 * seed + rows + ord(recipe) + (7 if fine == 'x' else 0))
        if gaussian:
            mk = lambda side, cols, part=None: torch.randn((rows, cols), generator=gen, device=DEV)      # noqa: E731
            self.table = torch.randn((P_ROWS, 128), generator=gen, device=DEV)
        else:
            mk = lambda side, cols, part=None: _values(recipe, fine == side, (rows, cols), gen, part)    # noqa: E731
            self.table = _values(recipe, fine == 'x', (P_ROWS, 128), gen, 'table')
        self.dqkv, self.ds2, self.ds1, self.dpre = mk('dy', 384), mk('dy', 128), mk('dy', 128), mk('dy', 256)
        self.h, self.y1, self.o, self.xp, self.x = mk('x', 256), mk('x', 128), mk('x', 128), mk('x', 128), mk('x', 128)
        unit_d_x = recipe == 'D' and fine != 'x' and not gaussian
        self.xq = None if unit_d_x else mk('x', 128, 'x')
        index = torch.randint(0, P_ROWS, (rows,), generator=gen, device=DEV, dtype=torch.int32)
        # the first and the last row of the table and repeats, from the first tokens on and at the very end
        head = torch.tensor([P_ROWS - 1, 0, 0, P_ROWS - 1, 7, 7, 7, P_ROWS - 1], dtype=torch.int32, device=DEV)[:rows]
        index[:head.numel()] = head
        index[-1] = P_ROWS - 1 if rows > 1 else index[-1]
        self.index = index
        if unit_d_x:                # x + table[index] is a unit operand of recipe D; x and the table hold small integers
            self.xq = _unit_d((rows, 128), gen) - self.table[index.long()]
        self.w2, self.w1 = _Prob(self.ds2, self.h, bias=bias), _Prob(self.dpre, self.y1, bias=bias)
        self.wo, self.wv = _Prob(self.ds1, self.o, bias=bias), _Prob(self.dqkv[:, 256:], self.x, bias=bias)
        self.wqk = _Prob(self.dqkv[:, :256], self.xp, bias=bias)
        self.wqk_pos = _Prob(self.dqkv[:, :256], self.xq, (self.table, self.index), bias=bias)
        self.group1, self.group2 = [self.w2, self.w1], [self.wo, self.wqk, self.wv]
        self.group2_pos = [self.wo, self.wqk_pos, self.wv]
        self.five, self.five_pos = self.group1 + self.group2, self.group1 + self.group2_pos


def _with_bias(recipe, fine):
    """recipe D with the fine operand on the dy side: db would be a sum of m fine values - those problems carry none"""
    return not (recipe == 'D' and fine == 'dy')


@functools.lru_cache(maxsize=None)
def _layer(recipe, fine):
    return _Layer(recipe, fine, min(M_SWEEP, M_CAP[recipe]), bias=_with_bias(recipe, fine))


@functools.lru_cache(maxsize=None)
def _extra(recipe, fine, out, inn):
    """a single problem of its own operands, cut like the layer's"""
    rows = min(M_SWEEP, M_CAP[recipe])
    gen = torch.Generator(device=DEV).manual_seed(out * 4099 + inn + ord(recipe))
    return _Prob(_values(recipe, fine == 'dy', (rows, out), gen), _values(recipe, fine == 'x', (rows, inn), gen),
                 bias=_with_bias(recipe, fine))


class _Tally:
    """bit-for-bit comparisons whose verdicts stay on the device until the sweep is over; then every failing token count is
    named with its residues modulo the quad, the step and two steps"""

    def __init__(self):
        self.flags, self.names = [], []

    def check(self, got, want, m, what):
        for g, w, part in zip(got, want, ('dW', 'db')):
            if w is None:
                assert g is None
                continue
            self.flags.append((g.double() != w).any())            # NaN (a destination that was never written) != anything
            self.names.append('m=%d (%%4=%d %%32=%d %%64=%d) %s %s' % (m, m % 4, m % 32, m % 64, what, part))

    def finish(self):
        assert self.flags
        bad = torch.stack(self.flags).cpu().tolist()
        failed = [n for n, b in zip(self.names, bad) if b]
        assert not failed, '%d of %d comparisons are not exact: %s' % (len(failed), len(bad), '; '.join(failed[:60]))


def _modes(D, fn):
    """fn(mode) under the fp32-pipe kernels and under the exact split; the default restored whatever happens"""
    try:
        for mode in ('f32', 'f32x6'):
            D.set_matmul_mode(mode)
            fn(mode)
    finally:
        D.set_matmul_mode(D.DEFAULT_MATMUL_MODE)


def _wrapper(D, probs, m, materialised=False):
    """dense.weight_bias_grad_group on fresh NaN destinations -> [(dW, db | None)]"""
    dests = [p.dest() for p in probs]
    D.weight_bias_grad_group([p.wrapper_args(m, dw, db, materialised) for p, (dw, db) in zip(probs, dests)])
    return dests


_QUERY = {'sst_weight_grad_group_f32x6': 'sst_weight_grad_group_f32x6_workspace_bytes',
          'sst_weight_grad_group_f32': 'sst_weight_grad_group_workspace_bytes'}
GUARD_BYTE = 0xA5


def _problem_array(probs, m, dests):
    from sst_amd import _lib
    arr = (_lib.WgradProblemF32 * len(probs))()
    for q, p, (dw, db) in zip(arr, probs, dests):
        mm = p.m_of(m)
        dy, x = p.dy[:mm], p.x[:mm]
        q.dy, q.x, q.m, q.ld_dy, q.ld_x = dy.data_ptr(), x.data_ptr(), mm, dy.stride(0), x.stride(0)
        q.dw, q.db, q.out, q.inn = dw.data_ptr(), (db.data_ptr() if db is not None else None), p.out, p.inn
        if p.xadd is not None:
            q.x_add_rows, q.x_add_index = p.xadd[0].data_ptr(), p.xadd[1][:mm].data_ptr()
    return arr


def _c_group(entry, probs, m, guard=0):
    """a group entry of include/sst_amd.h called as dense.py calls it, on a workspace of exactly the queried size (+ `guard`
    bytes of a pattern behind it, in the same allocation) -> ([(dW, db | None)], workspace, queried bytes)"""
    from sst_amd import _lib
    lib = _lib.load()
    dests = [p.dest() for p in probs]
    arr = _problem_array(probs, m, dests)
    need = getattr(lib, _QUERY[entry])(arr, len(probs))
    assert need > 0, (entry, m, need)
    ws = torch.full((need + guard,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    rc = getattr(lib, entry)(arr, len(probs), _lib.ptr(ws), _lib.stream_ptr())
    assert rc == 0, (entry, m, rc)
    return dests, ws, need


def _c_single(p, m, guard=0):
    """sst_weight_grad_f32 on one problem, same conventions"""
    from sst_amd import _lib
    lib = _lib.load()
    dw, db = p.dest()
    dy, x = p.dy[:m], p.x[:m]
    need = lib.sst_weight_grad_workspace_bytes(m, p.out, p.inn)
    assert need > 0
    ws = torch.full((need + guard,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    rc = lib.sst_weight_grad_f32(_lib.ptr(dy), _lib.ptr(x), m, p.out, p.inn, dy.stride(0), x.stride(0), _lib.ptr(dw), _lib.ptr(db),
                                 _lib.ptr(ws), _lib.stream_ptr())
    assert rc == 0, (m, rc)
    return (dw, db), ws, need


# ------------------------------------------------------------------------------------------------------------------------------
# token sweeps
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('recipe,fine', RECIPES_C)
def test_sweep_a_c_entries_every_m_from_1_to_130(recipe, fine):
    """the public C entries accept any m >= 1 and no Python caller goes below 4096: the five-problem layer group through
    sst_weight_grad_group_f32x6 (up to 7 of its 8 slices empty) and sst_weight_grad_group_f32, sst_weight_grad_f32 on 128 x 128
    and on 1024 x 256 (32 tiles), every m of 1 .. 130 (recipe C: 1 .. 64, where it is exact; recipe D, the one with a third
    bf16 part: 1 .. 130, 4 terms per element at any m)"""
    L = _layer(recipe, fine)
    big = _extra(recipe, fine, 1024, 256)
    tally = _Tally()
    for m in SWEEP_A:
        if m > M_CAP[recipe]:
            break
        _assert_exact(recipe, m, L.five + [big])
        want = [p.want(m) for p in L.five]
        for entry in ('sst_weight_grad_group_f32x6', 'sst_weight_grad_group_f32'):
            got, _, _ = _c_group(entry, L.five, m)
            for i, (g, w) in enumerate(zip(got, want)):
                tally.check(g, w, m, '%s problem %d' % (entry, i))
        tally.check(_c_single(L.wo, m)[0], want[2], m, 'sst_weight_grad_f32 128x128')
        tally.check(_c_single(big, m)[0], big.want(m), m, 'sst_weight_grad_f32 1024x256')
    tally.finish()


def _sweep_b_problem_sets(L, recipe, fine):
    """the two groups of test_weight_gradients_admissible, a single 128 x 128 problem (128 slices of one step) and a single
    384 x 128 one (80 slices: not a power of two)"""
    return [('group1', L.group1), ('group2', L.group2), ('128x128', [L.wo]), ('384x128', [_extra(recipe, fine, 384, 128)])]


@pytest.mark.parametrize('recipe,fine', RECIPES_B)
def test_sweep_b_wrapper_every_m_from_4090_to_4230(recipe, fine):
    """dense.weight_bias_grad_group in both modes at every m of 4090 .. 4230: all residues of the 4-token quad, the 32-token
    step and the 64-row chunk several times over, odd and even step counts per slice, and the Python gate at 4096 rows (below
    it: the library's GEMM and the column-sum kernel - exact on these operands as well, fp32 FMA chains of fp32 numbers)"""
    from sst_amd import dense as D
    L = _layer(recipe, fine)
    sets = _sweep_b_problem_sets(L, recipe, fine)
    tally = _Tally()
    wants = {}
    for m in SWEEP_B:
        _assert_exact(recipe, m, [p for _, probs in sets for p in probs])
        wants[m] = [[p.want(m) for p in probs] for _, probs in sets]

    def run(mode):
        for m in SWEEP_B:
            for (name, probs), want in zip(sets, wants[m]):
                for i, (g, w) in enumerate(zip(_wrapper(D, probs, m), want)):
                    tally.check(g, w, m, '%s %s problem %d' % (mode, name, i))

    _modes(D, run)
    tally.finish()


def test_long_spot_checks_exact():
    """m = 8191, 8193 and 90107 (recipe A), both modes: many steps per slice on either side of a power of two, and the token
    count of a full frame - where one lost row of 90 107 sits a factor of four below the relative bar of test_gpu_dense.py"""
    from sst_amd import dense as D
    L = _Layer('A', 'dy', 90107, seed=1)
    single = _Prob(L.dqkv, L.y1)
    sets = [('group1', L.group1), ('group2', L.group2), ('group2 + positional rows', L.group2_pos), ('384x128', [single])]
    tally = _Tally()
    for m in (8191, 8193, 90107):
        _assert_exact('A', m, L.five_pos + [single])
        wants = [[p.want(m) for p in probs] for _, probs in sets]

        def run(mode):
            for (name, probs), want in zip(sets, wants):
                for i, (g, w) in enumerate(zip(_wrapper(D, probs, m), want)):
                    tally.check(g, w, m, '%s %s problem %d' % (mode, name, i))

        _modes(D, run)
    tally.finish()


def test_bf16_group_every_m_exact():
    """bf16.wgrad_group on the five-problem call of test_wgrad_group_bf16 (bar there: 8e-5 sqrt(m)) - small integers are bf16
    numbers, so the fp32 accumulation of the bf16 kernel is exact too: m = 1 .. 130 and 4090 .. 4160"""
    from sst_amd import bf16
    L = _layer('A', 'dy')
    B = torch.bfloat16
    dqkv, xp, x, ds1, o, dpre, y1, h, ds2 = (t.to(B) for t in (L.dqkv, L.xp, L.x, L.ds1, L.o, L.dpre, L.y1, L.h, L.ds2))
    tally = _Tally()
    f32 = dict(dtype=torch.float32, device=DEV)
    for m in list(SWEEP_A) + list(range(4090, 4161)):
        _assert_exact('A', m, L.five)
        dw_in, db_in = torch.full((384, 128), NAN, **f32), torch.full((384,), NAN, **f32)
        dwo, dbo = torch.full((128, 128), NAN, **f32), torch.full((128,), NAN, **f32)
        dw1, db1 = torch.full((256, 128), NAN, **f32), torch.full((256,), NAN, **f32)
        dw2, db2 = torch.full((128, 256), NAN, **f32), torch.full((128,), NAN, **f32)
        bf16.wgrad_group([(dqkv[:m, :256], xp[:m], dw_in[:256], db_in[:256], 1, 0), (dqkv[:m, 256:], x[:m], dw_in[256:], db_in[256:], 1, 0),
                          (ds1[:m], o[:m], dwo, dbo, 1, 0), (dpre[:m], y1[:m], dw1, db1, 1, 0), (h[:m], ds2[:m], dw2, db2, 2, 1)])
        for name, p, got in (('dW2', L.w2, (dw2, db2)), ('dW1', L.w1, (dw1, db1)), ('dWo', L.wo, (dwo, dbo)),
                             ('dWqk', L.wqk, (dw_in[:256], db_in[:256])), ('dWv', L.wv, (dw_in[256:], db_in[256:]))):
            tally.check(got, p.want(m), m, 'bf16 ' + name)
    tally.finish()


# ------------------------------------------------------------------------------------------------------------------------------
# positional rows added on load (x_add_rows / x_add_index)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('recipe,fine', RECIPES_B)
def test_positional_rows_wrapper_sweep_b(recipe, fine):
    """dW_q | dW_k from x + table[index] through the fifth tuple element, against float64 of the materialised sum - an
    independent reference (the layer executor tests compare the kernel with itself).  The other problems of the group carry
    no table; in 'f32' mode and below 4096 rows the wrapper forms the sum first."""
    from sst_amd import dense as D
    L = _layer(recipe, fine)
    tally = _Tally()
    wants = {}
    for m in SWEEP_B:
        _assert_exact(recipe, m, L.group2_pos)
        wants[m] = [p.want(m) for p in L.group2_pos]

    def run(mode):
        for m in SWEEP_B:
            for i, (g, w) in enumerate(zip(_wrapper(D, L.group2_pos, m), wants[m])):
                tally.check(g, w, m, '%s group2 + positional rows, problem %d' % (mode, i))

    _modes(D, run)
    tally.finish()


@pytest.mark.parametrize('recipe,fine', RECIPES_C)
def test_positional_rows_c_entry_sweep_a(recipe, fine):
    """the same through sst_weight_grad_group_f32x6 itself, five problems, every m of 1 .. 130: the index of a token is loaded
    one request ahead of its table row and clamped at the end of the slice"""
    L = _layer(recipe, fine)
    tally = _Tally()
    for m in SWEEP_A:
        if m > M_CAP[recipe]:
            break
        _assert_exact(recipe, m, L.five_pos)
        got, _, _ = _c_group('sst_weight_grad_group_f32x6', L.five_pos, m)
        for i, (g, p) in enumerate(zip(got, L.five_pos)):
            tally.check(g, p.want(m), m, 'f32x6 + positional rows, problem %d' % i)
    tally.finish()


@pytest.mark.parametrize('m', [4097, 5001, 90107])
def test_positional_rows_gaussian_admissible(m):
    """Gaussian operands: the exact split with the rows added on load against float64, beside the fp32-pipe group on the
    materialised x + table[index] - the project's admissibility bar (test_gpu_dense_f32x6._admissible)"""
    from sst_amd import dense as D
    from test_gpu_dense_f32x6 import _admissible
    L = _Layer('A', 'dy', m, seed=2, gaussian=True)
    out = {}
    _modes(D, lambda mode: out.__setitem__(mode, _wrapper(D, L.group2_pos, m, materialised=(mode == 'f32'))))
    for p, (wn, bn), (ws, bs) in zip(L.group2_pos, out['f32'], out['f32x6']):
        want_w, want_b = p.want(m)
        _admissible(wn, ws, want_w, 'dW %s' % (tuple(want_w.shape),), floor=2e-7)
        _admissible(bn, bs, want_b, 'db', floor=1e-6)
        assert not torch.equal(wn, ws)                  # the split kernel really ran


def test_positional_rows_in_256():
    """the contract of x_add_rows: `in` a multiple of 128 with a table of the same width (the table row stride is `in`, the
    column offset that of the dW tile) - one exact case at in = 256, through the C entry and through the wrapper"""
    from sst_amd import dense as D
    L = _layer('A', 'dy')
    gen = torch.Generator(device=DEV).manual_seed(256)
    table = _values('A', True, (P_ROWS, 256), gen)
    p = _Prob(L.ds2, L.h, (table, L.index))
    tally = _Tally()
    for m in (97, 4131):
        _assert_exact('A', m, [p, L.wo])
        got, _, _ = _c_group('sst_weight_grad_group_f32x6', [p, L.wo], m)
        tally.check(got[0], p.want(m), m, 'in = 256 with positional rows (C entry)')
        tally.check(got[1], L.wo.want(m), m, 'its neighbour')
    with D.matmul_mode_scope('f32x6'):
        tally.check(_wrapper(D, [p, L.wo], 4131)[0], p.want(4131), 4131, 'in = 256 with positional rows (wrapper)')
    tally.finish()


def test_positional_rows_wrapper_validates_what_the_kernel_reads():
    """the kernel takes the table and the index as raw pointers: an int64 index, a strided index or a strided table must not
    reach it (the wrapper then forms the sum first) - each gives the exact result; a table of another width is an error"""
    from sst_amd import dense as D
    L = _layer('A', 'dy')
    m = 4131
    p = L.wqk_pos
    _assert_exact('A', m, L.group2_pos)
    want = [q.want(m) for q in L.group2_pos]
    twice = torch.stack([L.index[:m], L.index[:m] + 1], 1).contiguous()        # [m, 2]: column 0 is a strided view of the index
    wide = torch.cat([L.table, L.table + 1], 1).contiguous()                   # [P, 256]: columns :128 a strided view of the table
    variants = [('int64 index', (L.table, L.index[:m].long())), ('strided index', (L.table, twice[:, 0])),
                ('strided table', (wide[:, :128], L.index[:m])), ('int32, contiguous', (L.table, L.index[:m]))]
    tally = _Tally()

    def run(mode):
        for name, xadd in variants:
            dests = [q.dest() for q in L.group2_pos]
            args = [q.wrapper_args(m, dw, db) for q, (dw, db) in zip(L.group2_pos, dests)]
            args[1] = args[1][:4] + (xadd,)
            D.weight_bias_grad_group(args)
            for i, (g, w) in enumerate(zip(dests, want)):
                tally.check(g, w, m, '%s %s problem %d' % (mode, name, i))

    _modes(D, run)
    tally.finish()
    assert D._xadd_on_load_ok(p.x[:m], (L.table, L.index[:m]))
    assert not D._xadd_on_load_ok(p.x[:m], (L.table, L.index[:m].long()))
    assert not D._xadd_on_load_ok(p.x[:m], (wide, L.index[:m]))
    dw, db = p.dest()
    with pytest.raises(RuntimeError):
        D.weight_bias_grad_group([(p.dy[:m], p.x[:m], dw, db, (wide, L.index[:m]))])


# ------------------------------------------------------------------------------------------------------------------------------
# group structure and dispatch (recipe A, m = 4131)
# ------------------------------------------------------------------------------------------------------------------------------
M_GROUP = 4131


@functools.lru_cache(maxsize=None)
def _pool():
    gen = torch.Generator(device=DEV).manual_seed(4131)
    return _values('A', True, (M_GROUP, 1024), gen), _values('A', True, (M_GROUP, 1024), gen)


def _carve(out, inn, dy_off, x_off, bias=True, rows=None):
    """a problem on column windows of the pool (offsets % 4 == 0: 16-byte aligned views with a row stride)"""
    dy, x = _pool()
    return _Prob(dy[:, dy_off:dy_off + out], x[:, x_off:x_off + inn], bias=bias, rows=rows)


def _check_groups_both_modes(cases, m=M_GROUP):
    from sst_amd import dense as D
    tally = _Tally()
    for _, probs in cases:
        _assert_exact('A', m, probs)
    wants = [[p.want(m) for p in probs] for _, probs in cases]

    def run(mode):
        for (name, probs), want in zip(cases, wants):
            for i, (g, w) in enumerate(zip(_wrapper(D, probs, m), want)):
                tally.check(g, w, m, '%s %s problem %d (%d x %d)' % (mode, name, i, probs[i].out, probs[i].inn))

    _modes(D, run)
    tally.finish()


EIGHT = [(128, 128), (256, 128), (128, 256), (384, 128), (128, 384), (256, 256), (512, 128), (128, 128)]


def _eight():
    return [_carve(o, i, 28 * k, 20 * k + 4, bias=(k != 3)) for k, (o, i) in enumerate(EIGHT)]


def test_group_structure_exact():
    """eight problems of unequal sizes (the most a launch takes; 20 tiles, so the tile -> problem lookup walks unequal strides
    and the slice count clamps to 8), nine (the wrapper must still fill every destination), (512, 512) + (128, 128) = 17 tiles,
    problems without a bias gradient between problems with one, and different m inside one group"""
    from sst_amd import _lib
    eight = _eight()
    nine = eight + [_carve(128, 128, 640, 512, bias=False)]
    seventeen = [_carve(512, 512, 0, 8), _carve(128, 128, 516, 520)]
    some_bias = [_carve(128, 256, 0, 0), _carve(256, 128, 132, 260, bias=False), _carve(128, 128, 392, 392),
                 _carve(256, 128, 524, 524, bias=False), _carve(128, 128, 784, 656)]
    mixed_m = [_carve(128, 128, 0, 0), _carve(256, 128, 128, 128, rows=4100), _carve(128, 256, 384, 256)]
    # the exact-split kernel shares one token count between its problems: it must say so, and the wrapper must go elsewhere
    arr = _problem_array(mixed_m, M_GROUP, [p.dest() for p in mixed_m])
    assert _lib.load().sst_weight_grad_group_f32x6_workspace_bytes(arr, 3) < 0
    _check_groups_both_modes([('eight problems', eight), ('nine problems', nine), ('17 tiles', seventeen),
                              ('bias / no bias', some_bias), ('different m', mixed_m)])


def test_more_problems_than_a_launch_takes_is_an_error_and_launches_nothing():
    from sst_amd import _lib
    lib = _lib.load()
    nine = _eight() + [_carve(128, 128, 640, 512)]
    dests = [(torch.full((p.out, p.inn), SENTINEL, device=DEV), torch.full((p.out,), SENTINEL, device=DEV)) for p in nine]
    arr = _problem_array(nine, M_GROUP, dests)
    assert lib.sst_weight_grad_group_f32x6_workspace_bytes(arr, 9) < 0
    ws = torch.zeros(max(int(lib.sst_weight_grad_group_workspace_bytes(arr, 9)), 1 << 20), dtype=torch.uint8, device=DEV)
    assert lib.sst_weight_grad_group_f32x6(arr, 9, _lib.ptr(ws), _lib.stream_ptr()) != 0
    assert lib.sst_weight_grad_group_f32(arr, 9, _lib.ptr(ws), _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert all(bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all()) for dw, db in dests)
    assert not bool(ws.any())


def test_unaligned_and_ragged_operands_exact():
    """operands that are only 4-byte aligned (columns 1 .. 128 of a [m, 388] buffer: no 16-byte loads, so the exact split must
    refuse them and the fp32 dispatch must pick the narrow kernel; an X that is 8-byte aligned may still go to the wide one) and
    ragged widths (84, 128), (133, 130), (3, 16): exact in both modes, alone and beside an aligned problem"""
    from sst_amd import _lib
    gen = torch.Generator(device=DEV).manual_seed(388)
    bdy, bx = _values('A', True, (M_GROUP, 388), gen), _values('A', True, (M_GROUP, 388), gen)
    off1 = _Prob(bdy[:, 1:129], bx[:, 1:129])
    off_dy = _Prob(bdy[:, 131:387], bx[:, 132:260])              # dy 4-byte aligned, x 16-byte aligned
    off_x = _Prob(bdy[:, 132:260], bx[:, 2:130])                 # x 8-byte aligned only
    assert bdy[:, 1:129].data_ptr() % 16 == 4 and bdy.stride(0) % 4 == 0
    for p in (off1, off_dy, off_x):
        arr = _problem_array([p], M_GROUP, [p.dest()])
        assert _lib.load().sst_weight_grad_group_f32x6_workspace_bytes(arr, 1) < 0
    dy, x = _pool()
    ragged = [_Prob(dy[:, 4:4 + o].contiguous(), x[:, 8:8 + i].contiguous()) for o, i in ((84, 128), (133, 130), (3, 16))]
    _check_groups_both_modes([('4-byte aligned', [off1]), ('4-byte aligned beside aligned', [_carve(128, 128, 0, 0), off1, off_dy, off_x]),
                              ('ragged', ragged), ('ragged views', [_carve(84, 128, 4, 8), _carve(136, 132, 100, 200)])])


def test_destinations_inside_larger_buffers_keep_their_surroundings():
    """destinations that are row slices of larger buffers (as dw_in[:256] / dw_in[256:] of the packed in-projection gradient):
    exact inside, the sentinel untouched outside"""
    from sst_amd import dense as D
    L = _layer('A', 'dy')
    m = M_GROUP
    probs = [L.wo, L.wqk, L.wv, L.w1]
    _assert_exact('A', m, probs)
    want = [p.want(m) for p in probs]
    tally = _Tally()

    def run(mode):
        f32 = dict(dtype=torch.float32, device=DEV)
        big_w, big_b = torch.full((640, 128), SENTINEL, **f32), torch.full((640,), SENTINEL, **f32)
        dw_in, db_in = torch.full((384, 128), SENTINEL, **f32), torch.full((384,), SENTINEL, **f32)
        dests = [(big_w[512:640], big_b[512:640]), (dw_in[:256], db_in[:256]), (dw_in[256:], db_in[256:]), (big_w[128:384], big_b[128:384])]
        D.weight_bias_grad_group([p.wrapper_args(m, dw, db) for p, (dw, db) in zip(probs, dests)])
        for i, (g, w) in enumerate(zip(dests, want)):
            tally.check(g, w, m, '%s sliced destination %d' % (mode, i))
        for name, t in (('dW rows 0..127', big_w[:128]), ('dW rows 384..511', big_w[384:512]), ('db 0..127', big_b[:128]),
                        ('db 384..511', big_b[384:512])):
            tally.check((t,), (torch.full_like(t, SENTINEL).double(),), m, '%s sentinel %s' % (mode, name))

    _modes(D, run)
    tally.finish()


@pytest.mark.parametrize('m', [1, 257, 4097])
def test_workspace_queries_cover_what_the_kernels_write(m):
    """each of the three workspace queries: the call runs on a workspace of exactly the queried size whose allocation goes on
    with a few KB of a pattern - the pattern is intact afterwards and the result exact"""
    L = _layer('A', 'dy')
    dy, x = _pool()
    ragged = _Prob(dy[:, 4:137].contiguous(), x[:, 8:138].contiguous())        # (133, 130): the narrow kernel's split count
    tiled = _extra('A', 'dy', 1024, 256)
    _assert_exact('A', m, L.five_pos + [ragged, tiled])
    tally = _Tally()
    guard = 4096
    runs = [('sst_weight_grad_group_f32x6', L.five_pos) + _c_group('sst_weight_grad_group_f32x6', L.five_pos, m, guard),
            ('sst_weight_grad_group_f32', L.five + [ragged]) + _c_group('sst_weight_grad_group_f32', L.five + [ragged], m, guard)]
    for p in (L.wo, ragged, tiled):
        got, ws, need = _c_single(p, m, guard)
        runs.append(('sst_weight_grad_f32 %dx%d' % (p.out, p.inn), [p], [got], ws, need))
    for entry, probs, got, ws, need in runs:
        for i, (g, p) in enumerate(zip(got, probs)):
            tally.check(g, p.want(m), m, '%s problem %d' % (entry, i))
        assert ws.numel() == need + guard
        tally.check((ws[need:],), (torch.full((guard,), GUARD_BYTE, dtype=torch.float64, device=DEV),), m, entry + ' guard region')
    tally.finish()


def test_repeat_launches_bit_identical():
    """one sweep point (m = 4097, the layer group with the positional rows, Gaussian operands - with exact ones any order gives
    the same bits) 20 times: identical bits, through the C entry of the exact split and through the wrapper in both modes"""
    from sst_amd import dense as D
    m = 4097
    L = _Layer('A', 'dy', m, seed=3, gaussian=True)
    first = {}
    same = []

    def keep(key, dests):
        cur = [t for pair in dests for t in pair if t is not None]
        ref = first.setdefault(key, cur)
        same.extend((a != b).any() for a, b in zip(ref, cur))

    for _ in range(20):
        keep('c entry', _c_group('sst_weight_grad_group_f32x6', L.five_pos, m)[0])
        _modes(D, lambda mode: keep(mode, _wrapper(D, L.five_pos, m)))
    assert not bool(torch.stack(same).any())
    want = L.wqk_pos.want(m)[0]
    assert float((first['c entry'][6].double() - want).abs().max()) <= 2e-6 * float(want.abs().max())     # and it is the gradient
