"""GPU: the global-memory side of the exact-split linears (csrc/dense_f32x6.hip, tall_linear_f32x6_k): row-shaped loads and
stores through a wave-private LDS block (csrc/tile_io.h), the rolling prefetch of the X tiles and of the epilogue operands.

Exact operands: integers, x and aux in [-8, 8], weights in [-4, 4], bias in [-8, 8].  Every part of the three-way bf16 split,
every product and every partial sum is then exact in fp32 (K <= 384: |sum| <= 384 * 16 * 4 + 16 < 2^24 even with the
positional rows added to x), so the result must be torch.equal to the float64 product cast to fp32: a wrong row, column,
swizzle slot or stale block is a hard mismatch.  GELU and LayerNorm epilogues are compared as tests/test_gpu_dense_f32x6.py
compares them (_admissible, same bars).

Token counts: 1, 15, 16, 17, 33, and per column-group count of a launch (1, 2, 3) the smallest M at which a wave walks exactly
two and exactly three 16-row tiles, asked of the library (sst_tall_linear_f32x6_partition: the arithmetic launch_x6 itself uses;
10 241 / 20 481, 16 385 / 32 769 and 32 769 / 65 537 with the partition as it is): there the last wave has a partial tile (one row)
and the trailing waves of the last row blocks have none."""
import pytest
import torch

from test_gpu_dense_f32x6 import _admissible, _both

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.0
SMALL = [1, 15, 16, 17, 33]


def _partition(m, groups):
    """the library's own partition of m rows over `groups` column groups -> (row blocks, rows per wave)"""
    import ctypes
    from sst_amd import _lib
    rb, rpw = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().sst_tall_linear_f32x6_partition(m, groups, ctypes.byref(rb), ctypes.byref(rpw)),
               'sst_tall_linear_f32x6_partition')
    return rb.value, rpw.value


def _tile_sizes(groups):
    """the smallest M at which a wave walks two / three 16-row tiles, found in the library's partition (rows per wave never
    shrinks as M grows)"""
    sizes = []
    for tiles in (2, 3):
        lo, hi = 1, 1 << 20
        assert _partition(hi, groups)[1] >= 16 * tiles
        while lo < hi:
            mid = (lo + hi) // 2
            if _partition(mid, groups)[1] >= 16 * tiles:
                hi = mid
            else:
                lo = mid + 1
        sizes.append(lo)
    return sizes


def test_token_counts_follow_the_partition():
    """what the other tests rely on: at these sizes a wave walks exactly two / three tiles and one row fewer gives one tile
    fewer, the last wave with rows has a partial (one-row) tile, trailing waves have no rows"""
    for groups in (1, 2, 3):
        for tiles, m in zip((2, 3), _tile_sizes(groups)):
            rb, rpw = _partition(m, groups)
            assert rpw == 16 * tiles and _partition(m - 1, groups)[1] == 16 * (tiles - 1)
            assert m % 16 == 1 and -(-m // rpw) < rb * 8


def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _in_wide(t, ld, col):
    """t as a column slice of a wider tensor (row stride ld)"""
    wide = torch.full((t.size(0), ld), 7.0, device=t.device)
    wide[:, col:col + t.size(1)] = t
    return wide[:, col:col + t.size(1)]


class _Out:
    """an `out=` view inside a wider, taller buffer filled with a sentinel; check(): nothing outside [:m, :n] changed"""

    def __init__(self, m, n):
        self.big = torch.full((m + 3, n + 24), SENTINEL, device=DEV)
        self.view = self.big[1:m + 1, 8:8 + n]
        self.m, self.n = m, n

    def check(self):
        rest = self.big.clone()
        rest[1:self.m + 1, 8:8 + self.n] = SENTINEL
        assert bool((rest == SENTINEL).all())


def _f32x6(fn):
    from sst_amd import dense as D
    with D.matmul_mode_scope('f32x6'):
        return fn()


@pytest.mark.parametrize('k,n,groups', [(128, 128, 1), (128, 256, 2), (256, 128, 2)])
@pytest.mark.parametrize('trans_w', [False, True])
def test_exact_epilogues_every_token_count(k, n, groups, trans_w):
    from sst_amd import dense as D
    for m in SMALL + _tile_sizes(groups):
        g = torch.Generator().manual_seed(m + k + 2 * n + int(trans_w))
        x = _in_wide(_ints((m, k), 8, g).to(DEV), 384, 384 - k)
        w = _ints((k, n) if trans_w else (n, k), 4, g).to(DEV)
        b = _ints((n,), 8, g).to(DEV)
        aux = _in_wide(_ints((m, n), 8, g).to(DEV), n + 12, 4)
        assert x.stride(0) == 384 and aux.stride(0) != n
        ref = x.double() @ (w.double() if trans_w else w.double().t()) + b.double()
        for name, epi, a, want in (('bias', D.EPI_BIAS, None, ref), ('add', D.EPI_ADD, aux, ref + aux.double()),
                                   ('mul_relu_grad', D.EPI_MUL_RELU_GRAD, aux, ref * (aux.double() > 0))):
            out = _Out(m, n)
            got = _f32x6(lambda: D.lds_linear(x, w, b, epi, trans_w, aux_in=a, out=out.view))
            assert torch.equal(got, want.float()), (name, m)
            out.check()
        out = _Out(m, n)
        y, pre = _f32x6(lambda: D.lds_linear(x, w, b, D.EPI_RELU, trans_w, want_pre=True, out=out.view))
        assert torch.equal(pre, ref.float()) and torch.equal(y, torch.relu(ref).float()), ('relu', m)
        out.check()


def _epi2(x, x2, x2_from, w, b, n, trans_w=False, epi=0, aux=None, out=None):
    """sst_tall_linear_epi2_f32x6: the column groups from x2_from on read x2"""
    from sst_amd import _lib
    m, k = x.shape
    y = out if out is not None else torch.empty((m, n), device=DEV)
    rc = _lib.load().sst_tall_linear_epi2_f32x6(_lib.ptr(x), _lib.ptr(x2), x2_from, x.stride(0), _lib.ptr(w), w.stride(0), int(trans_w),
                                               _lib.ptr(b), m, k, n, epi, _lib.ptr(aux), None, aux.stride(0) if aux is not None else 0,
                                               _lib.ptr(y), y.stride(0), _lib.stream_ptr())
    _lib.check(rc, 'sst_tall_linear_epi2_f32x6')
    return y


def test_exact_qkv_one_launch_both_group_boundaries():
    from sst_amd import dense as D
    for m in SMALL + _tile_sizes(3):
        g = torch.Generator().manual_seed(3 * m)
        xp = _in_wide(_ints((m, 128), 8, g).to(DEV), 384, 0)
        x = _in_wide(_ints((m, 128), 8, g).to(DEV), 384, 256)
        w, b = _ints((384, 128), 4, g).to(DEV), _ints((384,), 8, g).to(DEV)
        full = [t.double() @ w.double().t() + b.double() for t in (xp, x)]
        one = _f32x6(lambda: D.lds_linear_qkv(xp, x, w, b))
        assert torch.equal(one, torch.cat([full[0][:, :256], full[1][:, 256:]], 1).float()), m
        for x2_from in (128, 256):
            out = _Out(m, 384)
            got = _epi2(xp, x, x2_from, w, b, 384, out=out.view)
            assert torch.equal(got, torch.cat([full[0][:, :x2_from], full[1][:, x2_from:]], 1).float()), (m, x2_from)
            out.check()


def test_exact_second_input_on_64_column_groups():
    """K = 256 and K = 384 (two 64-column groups): the second group reads x2"""
    for k in (256, 384):
        for m in (17, _tile_sizes(2)[0]):
            g = torch.Generator().manual_seed(k + m)
            xa, xb = _ints((m, k), 8, g).to(DEV), _ints((m, k), 8, g).to(DEV)
            w, b = _ints((k, 128), 4, g).to(DEV), _ints((128,), 8, g).to(DEV)
            got = _epi2(xa, xb, 64, w, b, 128, trans_w=True)
            want = torch.cat([(xa.double() @ w.double())[:, :64], (xb.double() @ w.double())[:, 64:]], 1) + b.double()
            assert torch.equal(got, want.float()), (k, m)


def test_exact_inproj_pos_rows_added_on_load():
    from sst_amd import dense as D
    for m in SMALL + _tile_sizes(3):
        g = torch.Generator().manual_seed(7 * m)
        x = _ints((m, 128), 8, g).to(DEV)
        table = _ints((144, 128), 8, g).to(DEV)
        idx = torch.randint(0, 144, (m,), generator=g, dtype=torch.int32)
        idx[0], idx[-1] = 143, 0                                       # the last and the first row of the table
        idx[m // 2:m // 2 + 3] = 5                                     # repeated rows
        idx = idx.to(DEV)
        w, b = _ints((384, 128), 4, g).to(DEV), _ints((384,), 8, g).to(DEV)
        assert _f32x6(lambda: D.inproj_pos_ok(x, (table, idx), w))
        got = _f32x6(lambda: D.inproj_pos(x, (table, idx), w, b))
        xp = x.double() + table.double()[idx.long()]
        want = torch.cat([xp @ w[:256].double().t(), x.double() @ w[256:].double().t()], 1) + b.double()
        assert torch.equal(got, want.float()), m


def test_exact_k384_data_gradient_and_its_three_parts():
    """d(x) = ds1 + [dq | dk | dv] W over K = 384 in one launch: against float64, in place and with a strided aux, and - without
    the residual - bit for bit the sum of the three K = 128 products of the same entry point"""
    from sst_amd import dense as D
    for m in SMALL + _tile_sizes(2):
        g = torch.Generator().manual_seed(11 * m)
        dqkv = _ints((m, 384), 8, g).to(DEV)
        w = _ints((384, 128), 4, g).to(DEV)
        ds1 = _ints((m, 128), 8, g).to(DEV)
        want = ds1.double() + dqkv.double() @ w.double()
        inplace = ds1.clone()
        _f32x6(lambda: D.lds_linear(dqkv, w, None, D.EPI_ADD, trans_w=True, aux_in=inplace, out=inplace))
        assert torch.equal(inplace, want.float()), m
        aux, out = _in_wide(ds1, 140, 8), _Out(m, 128)
        got = _f32x6(lambda: D.lds_linear(dqkv, w, None, D.EPI_ADD, trans_w=True, aux_in=aux, out=out.view))
        assert torch.equal(got, want.float()), m
        out.check()
        one = _f32x6(lambda: D.lds_linear(dqkv, w, None, D.EPI_BIAS, trans_w=True))
        parts = [_f32x6(lambda: D.lds_linear(dqkv[:, j:j + 128], w[j:j + 128], None, D.EPI_BIAS, trans_w=True)) for j in (0, 128, 256)]
        assert torch.equal(one, parts[0] + parts[1] + parts[2]), m
        assert torch.equal(one, (dqkv.double() @ w.double()).float()), m


@pytest.mark.parametrize('n', [128, 64])
def test_exact_add_rows_gather(n):
    """y = x W^T + rows[index] (K = 64), negative index -> row 0"""
    from sst_amd import _lib
    for m in SMALL + _tile_sizes(1):
        g = torch.Generator().manual_seed(13 * m + n)
        x = _in_wide(_ints((m, 64), 8, g).to(DEV), 384, 64)
        w = _ints((n, 64), 4, g).to(DEV)
        p = 1 + m // 3
        rows = _in_wide(_ints((p, n), 8, g).to(DEV), n + 20, 12)
        idx = torch.randint(0, p, (m,), generator=g, dtype=torch.int32)
        idx[0], idx[-1] = p - 1, 0
        idx[m // 2] = -1
        idx[m // 3:m // 3 + 2] = p // 2
        idx = idx.to(DEV)
        out = _Out(m, n)
        rc = _lib.load().sst_tall_linear_add_rows_f32x6(_lib.ptr(x), x.stride(0), _lib.ptr(w), w.stride(0), m, 64, n, _lib.ptr(rows),
                                                       rows.stride(0), _lib.ptr(idx), _lib.ptr(out.view), out.view.stride(0),
                                                       _lib.stream_ptr())
        _lib.check(rc, 'sst_tall_linear_add_rows_f32x6')
        want = x.double() @ w.double().t() + rows.double()[idx.long().clamp(min=0)]
        assert torch.equal(out.view, want.float()), m
        out.check()


@pytest.mark.parametrize('k,n,groups', [(128, 128, 1), (128, 256, 2), (256, 128, 2)])
def test_gelu_epilogues_admissible_every_token_count(k, n, groups):
    from sst_amd import dense as D
    for m in SMALL + _tile_sizes(groups):
        g = torch.Generator().manual_seed(m + k + n)
        x = torch.randn(m, k, generator=g).to(DEV)
        w = (torch.randn(n, k, generator=g) * 0.2).to(DEV)
        b = torch.randn(n, generator=g).to(DEV)
        aux = torch.randn(m, n, generator=g).to(DEV)
        ref = x.double() @ w.double().t() + b.double()
        ad = aux.double().requires_grad_(True)
        torch.nn.functional.gelu(ad).sum().backward()
        nat, spl = _both(D, lambda: D.lds_linear(x, w, b, D.EPI_MUL_GELU_GRAD, aux_in=aux))
        _admissible(nat, spl, ref * ad.grad, 'mul_gelu_grad', floor=1e-6)
        (yn, pn), (ys, ps) = _both(D, lambda: D.lds_linear(x, w, b, D.EPI_GELU, want_pre=True))
        _admissible(pn, ps, ref, 'gelu pre-activation')
        _admissible(yn, ys, torch.nn.functional.gelu(ref), 'gelu', floor=1e-6)


def test_add_layernorm_admissible_every_token_count():
    from sst_amd import _lib
    from sst_amd import dense as D
    for m in SMALL + _tile_sizes(1):
        g = torch.Generator().manual_seed(m)
        x = torch.randn(m, 128, generator=g).to(DEV)
        w = (torch.randn(128, 128, generator=g) * 0.2).to(DEV)
        b, lw, lb = (torch.randn(128, generator=g).to(DEV) for _ in range(3))
        res = torch.randn(m, 128, generator=g).to(DEV)
        table = torch.randn(144, 128, generator=g).to(DEV)
        idx = torch.randint(0, 144, (m,), generator=g, dtype=torch.int32)
        idx[0], idx[-1] = 143, 0
        idx = idx.to(DEV)
        ssum = x.double() @ w.double().t() + b.double() + res.double()
        ref = torch.nn.functional.layer_norm(ssum, (128,), lw.double(), lb.double(), 1e-5)
        nat, spl = _both(D, lambda: D.lds_linear_add_ln(x, w, b, res, lw, lb, 1e-5, pos=(table, idx)))
        spl_pos = spl
        _admissible(nat[1], spl[1], ssum, 'sum')
        _admissible(nat[0], spl[0], ref, 'layer norm', floor=1e-6)
        _admissible(nat[3], spl[3], ref + table.double()[idx.long()], 'layer norm + pos', floor=1e-6)
        mean, rstd = ssum.mean(1), (ssum.var(1, unbiased=False) + 1e-5).rsqrt()
        # the saved statistics: a 128-term fp32 sum is within 128 * 2^-24 of the largest addend's scale; the variance within twice
        # that relative to itself, its inverse root within half of it again (+ the rsqrt instruction's own 2^-22)
        assert float((spl[2][:, 0].double() - mean).abs().max()) <= 128 * 2.0 ** -24 * float(ssum.abs().max())
        assert float((spl[2][:, 1].double() / rstd - 1).abs().max()) <= 128 * 2.0 ** -24 + 2.0 ** -22
        nat, spl = _both(D, lambda: D.lds_linear_add_ln(x, w, b, res, lw, lb, 1e-5, save_sum=False))
        _admissible(nat[0], spl[0], ref, 'layer norm without sum and pos', floor=1e-6)
        # the C entry with a strided residual and sum (row stride ldres = 140 for both), every output inside a sentinel frame
        resw = _in_wide(res, 140, 8)
        sumw = torch.full((m + 2, 140), SENTINEL, device=DEV)
        outs = [torch.full((m + 2, c), SENTINEL, device=DEV) for c in (128, 128, 2)]
        y, yp, st = (t[1:m + 1] for t in outs)
        lib = _lib.load()
        rc = lib.sst_tall_linear_ln_f32x6(_lib.ptr(x), x.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(b), m, 128, _lib.ptr(resw), 140,
                                          _lib.ptr(lw), _lib.ptr(lb), 1e-5, _lib.ptr(y), _lib.ptr(sumw[1:m + 1, 4:132]), _lib.ptr(st),
                                          _lib.ptr(table), _lib.ptr(idx), _lib.ptr(yp), _lib.stream_ptr())
        _lib.check(rc, 'sst_tall_linear_ln_f32x6')
        assert torch.equal(y, spl_pos[0]) and torch.equal(sumw[1:m + 1, 4:132], spl_pos[1]) and torch.equal(st, spl_pos[2]) \
            and torch.equal(yp, spl_pos[3]), m
        sumw[1:m + 1, 4:132] = SENTINEL
        assert bool((sumw == SENTINEL).all())
        for t in outs:
            assert bool((t[0] == SENTINEL).all()) and bool((t[m + 1] == SENTINEL).all())
