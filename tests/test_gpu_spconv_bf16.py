"""GPU: the 'bf16' operand mode of the sparse convolutions (csrc/spconv_os_bf16.hip; sst_amd.spconv / sst_amd.sparse_unet).

The mode rounds every operand of the contraction to bf16 once (ties to even), multiplies bf16 x bf16 and accumulates in fp32;
results, storage and master weights are fp32.  So
  * on operands that are bf16 numbers whose sums are fp32 numbers (recipes A and E of tests/spconv_bf16_ref.py) the kernels return
    the float64 reference of tests/spconv_exact_ref.py BIT FOR BIT - tests 1-7 have no tolerance;
  * on general operands the result is the contraction of the ROUNDED operands up to the fp32 summation order - the quantity the
    parent's 'f32x6' / 'f32' kernels return on operands rounded beforehand.  Bar of tests 8 and 10 (the project's bar for a new
    arithmetic of the same class, tests/test_gpu_spconv.py::test_exact_split_convolution_kernel): error against the float64
    contraction of the rounded operands <= max(2 x the fp32-pipe kernel's error on the same rounded operands, 2e-7 x scale).
The C entries are called directly with sentinel-filled destinations and NaN workspaces; the split a call takes is asked of the
library (sst_spconv_conv_os_plan)."""
import copy

import numpy as np
import pytest
import torch

import spconv_bf16_ref as B
import spconv_exact_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.5
N_X = 97
THREE = [('A', 'x'), ('E', 'x'), ('E', 'w')]          # (recipe, the fine side)


def _lib():
    from sst_amd import _lib as L
    return L, L.load()


def _nan_bytes(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=DEV)


class _Tally:
    """bit-for-bit comparisons whose verdicts stay on the device until the test is over; then every failing one is named"""

    def __init__(self):
        self.flags, self.names = [], []

    def same(self, got, want, what):
        assert got.shape == want.shape and got.dtype == want.dtype, what
        self.flags.append((got != want).any())            # NaN (never written, or a NaN that leaked in) != anything
        self.names.append(what)

    def finish(self):
        assert self.flags
        bad = torch.stack(self.flags).cpu().tolist()
        failed = [n for n, b in zip(self.names, bad) if b]
        assert not failed, '%d of %d comparisons are not exact: %s' % (len(failed), len(bad), '; '.join(failed[:40]))


# ------------------------------------------------------------------------------------------------------------------------------
# the contraction, exact
# ------------------------------------------------------------------------------------------------------------------------------
class _Conv:
    """operands of one contraction on the device: x as [n_x, cin] and inside a [n_x, cin + 4] buffer of sentinels, w as
    [K, cin, cout] and as [K, cout, cin] (trans_w), the bias 16-byte aligned and offset by one float"""

    def __init__(self, recipe, fine, kvol, cin, cout, seed, n_x=N_X, nan_row0=False, operands=None):
        gen = torch.Generator().manual_seed(seed)
        self.recipe, self.fine, self.kvol, self.cin, self.cout, self.n_x = recipe, fine, kvol, cin, cout, n_x
        x, w, bias = operands if operands is not None else B.conv_operands(recipe, fine, n_x, kvol, cin, cout, gen)
        self.x = x.to(DEV)
        if nan_row0:
            self.x[0] = float('nan')
        self.x_wide = torch.full((n_x, cin + 4), SENTINEL, device=DEV)
        self.x_wide[:, :cin] = self.x
        self.w = w.to(DEV)
        self.w_stored = (self.w.contiguous(), self.w.transpose(1, 2).contiguous())
        b0, b1 = torch.full((cout + 8,), SENTINEL, device=DEV), torch.full((cout + 8,), SENTINEL, device=DEV)
        b0[4:4 + cout] = bias.to(DEV)
        b1[1:1 + cout] = bias.to(DEV)
        self.bias, self.bias_off1 = b0[4:4 + cout], b1[1:1 + cout]
        assert self.bias.data_ptr() % 16 == 0 and self.bias_off1.data_ptr() % 16 == 4 and self.x.data_ptr() % 16 == 0

    def want(self, mp, bias=True, rounded=False):
        """float64 reference (of the rounded operands if asked), its exactness asserted from the operands, as fp32"""
        x = self.x.clone()
        x[0] = torch.nan_to_num(x[0])
        w = self.w
        if rounded:
            x, w = B.round_bf16(x), B.round_bf16(w)
        b = self.bias if bias else None
        if self.recipe is not None:
            R.assert_conv_exact(self.recipe, x, mp, w, b)
        y = R.conv_ref(x, mp, w, b)
        out = y.float()
        assert torch.equal(out.double(), y)
        return out


def _pack_bytes(c):
    return _lib()[1].sst_spconv_conv_os_bf16_workspace_bytes_rows(c.kvol, c.cin, c.cout, 0)


def _full_bytes(c, m):
    return _lib()[1].sst_spconv_conv_os_bf16_workspace_bytes_rows(c.kvol, c.cin, c.cout, m)


def _call(c, mp, m, y, ldy, trans_w=0, bias=None, x=None, ldx=None, order=None, nbytes=None, ws=None, kvol=None, cin=None):
    """sst_spconv_conv_os_rows_bf16 on a NaN workspace of nbytes (default: all the call asks for)"""
    L, lib = _lib()
    x = c.x if x is None else x
    ldx = c.cin if ldx is None else ldx
    nbytes = _full_bytes(c, m) if nbytes is None else nbytes
    if ws is None:
        ws = _nan_bytes(nbytes)
        assert ws.data_ptr() % 256 == 0
    return lib.sst_spconv_conv_os_rows_bf16(L.ptr(x), ldx, L.ptr(mp), m, c.kvol if kvol is None else kvol,
                                            L.ptr(c.w_stored[trans_w]), c.cin if cin is None else cin, c.cout, trans_w, L.ptr(bias),
                                            L.ptr(y), ldy, 0, L.ptr(order), L.ptr(ws), nbytes, L.stream_ptr())


def _run_layout(tally, c, mp, m, want, what, trans_w=0, layout=0, order=None, bias=True, nbytes=None):
    """one call into a sentinel-filled destination with two spare rows; the whole buffer is compared: rows at and beyond m and
    columns beyond cout must keep the sentinel.
    layout 0: ldx = cin, ldy = cout, bias 16-byte aligned (the vector stores when cout % 4 == 0)
           1: ldx = cin + 4 and ldy = cout + 1, sentinels between the rows
           2: y offset by one float (ldy a multiple of 4): the scalar stores
           3: the bias offset by one float (y aligned, ldy a multiple of 4): the scalar stores"""
    cout = c.cout
    ldy = {0: cout, 1: cout + 1}.get(layout, (cout + 3) // 4 * 4 + 4)
    buf = torch.full(((m + 2) * ldy + 4,), SENTINEL, device=DEV)
    y0 = buf[1:] if layout == 2 else buf
    b = None if not bias else (c.bias_off1 if layout == 3 else c.bias)
    x, ldx = (c.x_wide, c.cin + 4) if layout == 1 else (c.x, c.cin)
    rc = _call(c, mp, m, y0, ldy, trans_w, b, x, ldx, order, nbytes)
    assert rc == 0, (what, rc)
    expect = torch.full_like(buf, SENTINEL)
    off = 1 if layout == 2 else 0
    expect[off:off + (m + 2) * ldy].view(m + 2, ldy)[:m, :cout] = want[:m]
    tally.same(buf, expect, what)


def _split(c, m, nbytes):
    rc, _, _, split, _ = R.conv_plan(B.ROWS_BF16, m, c.kvol, c.cin, c.cout, 0, nbytes)
    assert rc == 0
    return split


@pytest.mark.parametrize('cin,cout', [(12, 20), (64, 64)])
@pytest.mark.parametrize('recipe,fine', THREE)
def test_row_sweep_every_m_from_1_to_130(recipe, fine, cin, cout):
    """1. every m of 1 .. 130 on column prefixes of one map (tile edges 63 / 64 / 65 / 127 / 128 / 129), kvol 27, both weight
    orientations, with the workspace the call asks for (thin level: the offsets are dealt out) and with the packed weights alone
    (unsplit), with and without bias"""
    c = _Conv(recipe, fine, 27, cin, cout, seed=100 + ord(recipe) + (fine == 'w') + cin)
    rng = np.random.default_rng(130)
    full = R.make_map('random', 27, 130, N_X, rng)
    R.check_map(full, N_X)
    mp_full = torch.from_numpy(full).to(DEV)
    wants = {True: c.want(mp_full, True), False: c.want(mp_full, False)}
    pack = _pack_bytes(c)
    assert _split(c, 130, _full_bytes(c, 130)) > 1 and _split(c, 130, pack) == 1
    tally = _Tally()
    for m in range(1, 131):
        mp = mp_full[:, :m].contiguous()
        for trans_w in (0, 1):
            for nbytes, bias in ((None, True), (pack, True), (None, False)):
                _run_layout(tally, c, mp, m, wants[bias], 'm=%d trans_w=%d nbytes=%s bias=%d' % (m, trans_w, nbytes, bias),
                            trans_w, 0, None, bias, nbytes)
    tally.finish()


@pytest.mark.parametrize('kvol', [1, 8, 27, 32])
def test_map_families(kvol):
    """2. every map family at m = 130 and kvol = 1, 8, 27, 32 (the most the index image holds); the variant lo = 1 never
    references row 0 of x, which is NaN there (rows without a partner read it and must contribute zero)"""
    rng = np.random.default_rng(kvol)
    tally = _Tally()
    m = 130
    for i, (recipe, fine) in enumerate(THREE):
        for lo in (0, 1):
            c = _Conv(recipe, fine, kvol, 16, 32, seed=200 + kvol + 7 * i + lo, nan_row0=lo == 1)
            for fam in R.MAP_FAMILIES + ('empty',):
                mp_np = R.make_map(fam, kvol, m, N_X, rng, lo=lo)
                R.check_map(mp_np, N_X)
                assert lo == 0 or (mp_np != 0).all()
                mp = torch.from_numpy(mp_np).to(DEV)
                want = c.want(mp)
                for nbytes in (None, _pack_bytes(c)):
                    _run_layout(tally, c, mp, m, want, 'kvol=%d %s %s%s lo=%d nbytes=%s' % (kvol, fam, recipe, fine, lo, nbytes),
                                nbytes=nbytes)
    tally.finish()


@pytest.mark.parametrize('cin,cout', [(4, 4), (12, 20), (16, 7), (64, 64), (64, 66), (68, 132), (128, 160), (256, 256)])
def test_channel_shapes(cin, cout):
    """3. channel counts with tails in every position (one and several channel chunks and column groups) at m = 200, both weight
    orientations, the four memory layouts, with and without bias"""
    tally = _Tally()
    rng = np.random.default_rng(cin * 1000 + cout)
    m = 200
    for i, (recipe, fine) in enumerate(THREE):
        c = _Conv(recipe, fine, 27, cin, cout, seed=300 + cin + cout + 11 * i)
        mp_np = R.make_map('random', 27, m, N_X, rng)
        R.check_map(mp_np, N_X)
        mp = torch.from_numpy(mp_np).to(DEV)
        wants = {True: c.want(mp, True), False: c.want(mp, False)}
        for trans_w in (0, 1):
            for layout, bias in ((0, True), (1, False), (2, True), (3, True), (0, False)):
                _run_layout(tally, c, mp, m, wants[bias], '%d->%d %s%s trans_w=%d layout %d bias %d'
                            % (cin, cout, recipe, fine, trans_w, layout, bias), trans_w, layout, None, bias)
    tally.finish()


@pytest.mark.parametrize('cin,cout', [(16, 32), (64, 64), (68, 132)])
def test_offset_split_and_permuted_tile_order(cin, cout):
    """4. m chosen so that the plan reports more than one split over several tiles: the split call, in natural and in a permuted
    tile order, equals the unsplit call (packed weights only) and the reference"""
    tally = _Tally()
    rng = np.random.default_rng(cin + cout)
    m = 64 * 7 - 9
    for i, (recipe, fine) in enumerate(THREE):
        c = _Conv(recipe, fine, 27, cin, cout, seed=400 + cin + 5 * i)
        full, pack = _full_bytes(c, m), _pack_bytes(c)
        natural = _split(c, m, full)
        assert natural > 1 and _split(c, m, pack) == 1
        splits = sorted({_split(c, m, pack + s * m * ((cout + 3) // 4 * 4) * 4) for s in (1, 2, 4, 8)})
        assert splits[0] == 1 and splits[-1] == natural and len(splits) > 1
        mp_np = R.make_map('random', 27, m, N_X, rng)
        mp = torch.from_numpy(mp_np).to(DEV)
        want = c.want(mp)
        order = torch.from_numpy(rng.permutation(-(-m // 64)).astype(np.int32)).to(DEV)
        for s in (1, 2, 4, 8):
            nbytes = pack + (s * m * ((cout + 3) // 4 * 4) * 4 if s > 1 else 0)
            for o, oname in ((None, 'natural'), (order, 'permuted')):
                _run_layout(tally, c, mp, m, want, '%d->%d %s%s room for %d splits, %s order' % (cin, cout, recipe, fine, s, oname),
                            order=o, nbytes=nbytes)
    tally.finish()


# ------------------------------------------------------------------------------------------------------------------------------
# the filter gradient, exact
# ------------------------------------------------------------------------------------------------------------------------------
WG_THREE = [('A', 'x'), ('E', 'x'), ('E', 'dy')]


class _Wgrad:
    def __init__(self, recipe, fine, cin, cout, seed, wide=False, operands=None):
        gen = torch.Generator().manual_seed(seed)
        self.recipe, self.cin, self.cout = recipe, cin, cout
        self.rows_x, self.rows_dy = max(90, cin + 7), max(70, cout + 5)
        x, dy = operands if operands is not None else B.wgrad_operands(recipe, fine, self.rows_x, self.rows_dy, cin, cout, gen)
        self.rows_x, self.rows_dy = x.size(0), dy.size(0)
        self.ldx, self.lddy = (cin + 4, cout + 8) if wide else (cin, cout)
        bx = torch.full((self.rows_x, self.ldx), SENTINEL, device=DEV)
        bdy = torch.full((self.rows_dy, self.lddy), SENTINEL, device=DEV)
        bx[:, :cin], bdy[:, :cout] = x.to(DEV), dy.to(DEV)
        self.x, self.dy = bx[:, :cin], bdy[:, :cout]

    def pairs(self, num, pair_ld, x_side, rng):
        rows = (self.rows_x, self.rows_dy) if x_side == 0 else (self.rows_dy, self.rows_x)
        p = R.make_pairs(num, pair_ld, rows[0], rows[1], rng)
        for side in (0, 1):
            assert p[:, side].min() >= -1 and p[:, side].max() < rows[side]
        return torch.from_numpy(p).to(DEV)

    def want(self, pairs, num, x_side, rounded=False):
        x, dy = (B.round_bf16(self.x), B.round_bf16(self.dy)) if rounded else (self.x, self.dy)
        if self.recipe is not None:
            R.assert_wgrad_exact(self.recipe, x, dy, pairs, num, x_side)
        dw = R.wgrad_ref(x, dy, pairs, num, x_side)
        out = dw.float()
        assert torch.equal(out.double(), dw)
        for k, n in enumerate(num):
            assert n or not bool(out[k].any())
        return out


def _wgrad_call(g, pairs, num_dev, total, x_side):
    L, lib = _lib()
    kvol, pair_ld = pairs.size(0), pairs.size(2)
    ws = _nan_bytes(lib.sst_spconv_wgrad_os_workspace_bytes(kvol, pair_ld, total, g.cin, g.cout))
    dw = torch.full((kvol, g.cin, g.cout), SENTINEL, device=DEV)
    rc = lib.sst_spconv_wgrad_os_bf16(L.ptr(g.x), g.ldx, L.ptr(g.dy), g.lddy, L.ptr(pairs), pair_ld, total, x_side, L.ptr(num_dev),
                                      kvol, g.cin, g.cout, L.ptr(dw), L.ptr(ws), L.stream_ptr())
    assert rc == 0, rc
    return dw


def _wgrad_run(tally, g, num, pair_ld, rng, what):
    num = [int(v) for v in num]
    num_dev = torch.tensor(num, dtype=torch.int32, device=DEV)
    for x_side in (0, 1):
        pairs = g.pairs(num, pair_ld, x_side, rng)
        want = g.want(pairs, num, x_side)
        for total in (sum(num), -1):
            tally.same(_wgrad_call(g, pairs, num_dev, total, x_side), want, '%s x_side=%d total_pairs=%d' % (what, x_side, total))


@pytest.mark.parametrize('recipe,fine', WG_THREE)
def test_filter_gradient_every_pair_count_from_0_to_161(recipe, fine):
    """5a. num[k] = base + k over six launches: every count of 0 .. 161 (the 64-pair stage tail in all of its positions, one and
    several stages), then all offsets empty, and a single pair in one offset; 16 -> 32 channels, both x_side"""
    g = _Wgrad(recipe, fine, 16, 32, seed=600 + ord(recipe) + (fine == 'x'))
    rng = np.random.default_rng(161)
    tally = _Tally()
    launches = [[base + k for k in range(27)] for base in range(0, 136, 27)] + [[0] * 27, [0] * 13 + [1] + [0] * 13]
    assert sorted(set(v for n in launches for v in n)) == list(range(162))
    for num in launches:
        _wgrad_run(tally, g, num, 192, rng, '%s%s counts %d..%d' % (recipe, fine, min(num), max(num)))
    tally.finish()


def test_filter_gradient_chunk_edges():
    """5b. the chunk edges of tests/test_gpu_spconv_exact.py, (16, 32, 5000, 1100, 512): counts of c - 1, c, c + 1, 2 c and
    2 c + 1 pairs, c the chunk size asked of the plan query, beside an empty offset, a single pair and three pairs"""
    cin, cout, total, pair_ld, chunk = 16, 32, 5000, 1100, 512
    rc, c, _ = R.wgrad_plan(27, pair_ld, total, cin, cout)
    assert rc == 0 and c == chunk
    num = [0, 1, 3, c - 1, c, c + 1, 2 * c, 2 * c + 1]
    rest, free = total - sum(num), 27 - len(num) - 1
    assert rest >= 0 and max(num) <= pair_ld <= B.GPU_WGRAD_MAX_PAIRS
    num += [rest // free + (i < rest % free) for i in range(free)] + [0]
    assert len(num) == 27 and sum(num) == total and max(num) <= pair_ld
    rng = np.random.default_rng(total)
    tally = _Tally()
    for i, (recipe, fine) in enumerate(WG_THREE):
        for wide in (False, True):
            _wgrad_run(tally, _Wgrad(recipe, fine, cin, cout, seed=700 + i, wide=wide), num, pair_ld, rng,
                       '%s%s wide=%d chunk edges' % (recipe, fine, wide))
    tally.finish()


@pytest.mark.parametrize('cin,cout', [(4, 4), (16, 32), (64, 64), (68, 132), (256, 256)])
def test_filter_gradient_channel_shapes(cin, cout):
    """5c. one and several 64 x 64 blocks of dW[k] with channel tails, both x_side, rows with sentinels between them"""
    rng = np.random.default_rng(cin + cout)
    tally = _Tally()
    num = [0, 1, 63, 64, 65, 130, 200] + [int(v) for v in rng.integers(0, 150, 20)]
    for i, (recipe, fine) in enumerate(WG_THREE):
        _wgrad_run(tally, _Wgrad(recipe, fine, cin, cout, seed=800 + i + cin, wide=i == 1), num, 256, rng,
                   '%d->%d %s%s' % (cin, cout, recipe, fine))
    tally.finish()


# ------------------------------------------------------------------------------------------------------------------------------
# 6. round to nearest even
# ------------------------------------------------------------------------------------------------------------------------------
RNE_IN = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20]
RNE_OUT = [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 1 + 2.0 ** -7]


def _rne_values(shape, gen):
    pick = torch.randint(0, len(RNE_IN), tuple(shape), generator=gen)
    return torch.tensor(RNE_IN, dtype=torch.float32)[pick]


def test_operands_are_rounded_to_nearest_even():
    """6. ties go to the even neighbour (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6, their negatives), anything above a tie goes up
    (1 + 2^-8 + 2^-20 -> 1 + 2^-7): on the row side and the weight side of the contraction and on both sides of the filter
    gradient, the other operand one-hot units, so that every output is ONE product = +- round_bf16(input), gathered.  Normal
    numbers only."""
    assert torch.equal(B.round_bf16(torch.tensor(RNE_IN)), torch.tensor(RNE_OUT)) and not B.is_bf16(torch.tensor(RNE_IN))
    gen = torch.Generator().manual_seed(6)
    rng = np.random.default_rng(6)
    tally = _Tally()
    kvol, cin, cout, m = 27, 16, 32, 130
    mp_np = np.full((kvol, m), -1, np.int32)                     # one partner per row, in offset r % kvol
    mp_np[np.arange(m) % kvol, np.arange(m)] = rng.integers(0, N_X, m)
    mp = torch.from_numpy(mp_np).to(DEV)
    bias = torch.zeros(cout)
    for side in ('x', 'w'):
        x = _rne_values((N_X, cin), gen) if side == 'x' else R.one_hot_rows(N_X, cin, gen)
        w = _rne_values((kvol, cin, cout), gen) if side == 'w' else R.one_hot_weights(kvol, cin, cout, gen)
        c = _Conv(None, side, kvol, cin, cout, 0, operands=(x, w, bias))
        want = c.want(mp, bias=False, rounded=True)
        gathered = torch.isin(want.abs(), torch.tensor(RNE_OUT + [0.0], device=DEV).abs())
        assert bool(gathered.all()) and float((want != 0).float().mean()) > (0.9 if side == 'x' else 0.03)
        assert not torch.equal(want, c.want(mp, bias=False, rounded=False))
        for trans_w in (0, 1):
            for nbytes in (None, _pack_bytes(c)):
                _run_layout(tally, c, mp, m, want, 'rne %s side trans_w=%d nbytes=%s' % (side, trans_w, nbytes), trans_w, 0, None,
                            False, nbytes)
    # filter gradient: the unit side has one-hot rows, and the pairs of an offset pick rows of distinct channels
    for side in ('x', 'dy'):
        rows = 64
        x = _rne_values((rows, cin), gen) if side == 'x' else R.one_hot_rows(rows, cin, gen)
        dy = _rne_values((rows, cout), gen) if side == 'dy' else R.one_hot_rows(rows, cout, gen)
        unit = dy if side == 'x' else x
        channel = unit.abs().argmax(1).numpy()
        g = _Wgrad(None, side, cin, cout, 0, operands=(x, dy))
        num = [int(v) for v in rng.integers(0, unit.size(1) + 1, kvol)]
        for x_side in (0, 1):
            p = np.full((kvol, 2, 40), -1, np.int32)
            for k, n in enumerate(num):
                chans = rng.permutation(unit.size(1))[:n]
                hot_rows = np.array([rng.choice(np.nonzero(channel == ch)[0]) for ch in chans], dtype=np.int64)
                other = rng.integers(0, rows, n)
                x_rows, dy_rows = (other, hot_rows) if side == 'x' else (hot_rows, other)
                p[k, x_side, :n], p[k, 1 - x_side, :n] = x_rows, dy_rows
            pairs = torch.from_numpy(p).to(DEV)
            want = g.want(pairs, num, x_side, rounded=True)
            assert bool(torch.isin(want.abs(), torch.tensor(RNE_OUT + [0.0], device=DEV).abs()).all()) and bool(want.any())
            got = _wgrad_call(g, pairs, torch.tensor(num, dtype=torch.int32, device=DEV), sum(num), x_side)
            tally.same(got, want, 'rne filter gradient %s side x_side=%d' % (side, x_side))
    tally.finish()


# ------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """7. cin = 6, kvol = 33, a misaligned x, a row stride that is no multiple of 4, a tile_cfg, and a workspace one byte short of
    the packed weights (the least a call accepts; with the split: one byte short of everything at kvol = 1, where the call takes
    no split): the error code, and neither the sentinel-filled output nor the workspace is touched"""
    L, lib = _lib()
    c = _Conv('A', 'x', 27, 16, 32, seed=7)
    m = 130
    mp = torch.from_numpy(R.make_map('random', 33, m, N_X, np.random.default_rng(7))).to(DEV)
    y = torch.full((m, 32), SENTINEL, device=DEV)
    ws = _nan_bytes(1 << 20)
    xbuf = torch.full((N_X * 16 + 8,), 1.0, device=DEV)
    UNS, ARG = L.SST_ERR_UNSUPPORTED, L.SST_ERR_ARG
    assert _call(c, mp, m, y, 32, x=xbuf, ldx=8, cin=6, ws=ws, nbytes=1 << 20) == UNS
    assert _call(c, mp, m, y, 32, kvol=33, ws=ws, nbytes=1 << 20) == UNS
    assert _call(c, mp, m, y, 32, x=xbuf[1:], ws=ws, nbytes=1 << 20) == UNS
    assert _call(c, mp, m, y, 32, x=xbuf, ldx=18, ws=ws, nbytes=1 << 20) == UNS
    assert _call(c, mp, m, y, 32, ws=ws[16:], nbytes=1 << 19) == UNS                   # the workspace itself misaligned
    pack = _pack_bytes(c)
    assert _call(c, mp, m, y, 32, ws=ws, nbytes=pack - 1) == ARG
    assert lib.sst_spconv_conv_os_rows_bf16(L.ptr(c.x), 16, L.ptr(mp), m, 27, L.ptr(c.w), 16, 32, 0, None, L.ptr(y), 32, 41, None,
                                            L.ptr(ws), 1 << 20, L.stream_ptr()) == ARG
    c1 = _Conv('A', 'x', 1, 16, 32, seed=8)
    full1 = _full_bytes(c1, m)
    assert _split(c1, m, full1) == 1 and full1 == _pack_bytes(c1)
    assert _call(c1, mp, m, y, 32, ws=ws, nbytes=full1 - 1) == ARG
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((ws == 0xFF).all())
    assert _call(c, mp, m, y, 32, ws=ws, nbytes=pack) == 0                              # and the least it accepts is accepted
    assert bool((y != SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------
# general operands
# ------------------------------------------------------------------------------------------------------------------------------
def _cloud(rng, n, batch, shape):
    vol = int(np.prod(shape))
    lin = rng.choice(batch * vol, n, replace=False)
    b, r = lin // vol, lin % vol
    return np.stack([b, r // (shape[1] * shape[2]), (r // shape[2]) % shape[1], r % shape[2]], 1).astype(np.int32)


def _err(got, ref):
    return float((got.double() - ref).abs().max())


def _scale(ref):
    return max(1.0, float(ref.abs().max()))


def _admissible(err_bf16, err_f32, scale, what):
    print('%s: bf16 %.3e  fp32 pipe %.3e  scale %.3e' % (what, err_bf16, err_f32, scale))
    assert err_bf16 <= max(2.0 * err_f32, 2e-7 * scale), (what, err_bf16, err_f32, scale)


@pytest.mark.parametrize('cin,cout', [(64, 64), (16, 32), (128, 160), (256, 256)])
def test_general_operands_admissible_and_deterministic(cin, cout):
    """8. + 9. the cloud of test_exact_split_convolution_kernel (batch 2, [6, 40, 44], 6000 voxels), SubM and stride 2: y, dx and dw
    of the 'bf16' mode against the float64 contraction of the ROUNDED operands, beside the fp32-pipe kernel on the same rounded
    operands; the mode was really taken (the output differs from 'f32x6' on the unrounded operands); two calls agree bit for bit"""
    from sst_amd import spconv
    rng = np.random.default_rng(cin + cout)
    batch, shape, n = 2, [6, 40, 44], 6000
    ind = torch.from_numpy(_cloud(rng, n, batch, shape)).to(DEV)
    for subm, st in ((True, 1), (False, 2)):
        outids, pairs, num = spconv.get_indice_pairs(ind, batch, shape, [3] * 3, [st] * 3, [1] * 3, [1] * 3, 0, subm, False)
        rb = pairs._sst_rulebook
        m = outids.size(0)
        gen = torch.Generator().manual_seed(7)
        x = (torch.randn(n, cin, generator=gen) * 3).to(DEV)
        w = (torch.randn(27, cin, cout, generator=gen) * 0.2).to(DEV)
        gy = torch.randn(m, cout, generator=gen).to(DEV)
        xr, wr, gyr = B.round_bf16(x), B.round_bf16(w), B.round_bf16(gy)
        assert not torch.equal(xr, x) and not torch.equal(wr, w) and not torch.equal(gyr, gy)
        num_l = [int(v) for v in num.cpu()]
        refs = (R.conv_ref(xr, rb.out2in, wr), R.conv_ref(gyr, rb.in2out, wr.transpose(1, 2)), R.wgrad_ref(xr, gyr, pairs, num_l, 0))

        def run(mode, a, b, g):
            return (spconv._gather_gemm(a, rb.out2in, m, b, False, cout, rb, precision=mode),
                    spconv._gather_gemm(g, rb.in2out, n, b, True, cin, rb, precision=mode),
                    spconv._wgrad(a, g, rb, pairs, 0, (27, cin, cout), precision=mode))

        bf = run('bf16', x, w, gy)
        f32 = run('f32', xr, wr, gyr)
        x6 = run('f32x6', x, w, gy)
        for name, got, base, other, ref in zip(('y', 'dx', 'dw'), bf, f32, x6, refs):
            _admissible(_err(got, ref), _err(base, ref), _scale(ref), '%d->%d subm=%d %s' % (cin, cout, subm, name))
            assert not torch.equal(got, other), name
        again = run('bf16', x, w, gy)
        for name, a, b2 in zip(('y', 'dx', 'dw'), bf, again):
            assert torch.equal(a, b2), name
    assert spconv.conv_precision() == spconv.DEFAULT_CONV_PRECISION


# ------------------------------------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------------------------------------
def _module_setup(kind, cin, cout, seed):
    """-> (make(): a fresh module with the same parameters, tensor(features): its input, rows of the input, x_side, inverse, subm)"""
    from sst_amd import spconv
    rng = np.random.default_rng(seed)
    batch, shape, n = 2, [6, 20, 22], 1500
    ind = torch.from_numpy(_cloud(rng, n, batch, shape)).to(DEV)
    ctor = {'subm': lambda: spconv.SubMConv3d(cin, cout, 3, padding=1, bias=True, indice_key='k'),
            'conv': lambda: spconv.SparseConv3d(cin, cout, 3, stride=2, padding=1, bias=True, indice_key='k'),
            'transpose': lambda: spconv.SparseConvTranspose3d(cin, cout, 3, stride=2, padding=1, bias=True, indice_key='k'),
            'inverse': lambda: spconv.SparseInverseConv3d(cin, cout, 3, indice_key='d', bias=True)}[kind]
    torch.manual_seed(seed)
    state = ctor().state_dict()
    coarse = None
    if kind == 'inverse':       # the rulebook of its couple: a stride-2 convolution from the fine voxels onto the coarse ones
        down = spconv.SparseConv3d(cout, cin, 3, stride=2, padding=1, bias=False, indice_key='d')
        fine = spconv.SparseConvTensor(None, ind, shape, batch)
        coarse = down.dry(fine)

    def make():
        mod = ctor()
        mod.load_state_dict(state)
        return mod.to(DEV)

    def tensor(features):
        if coarse is None:
            return spconv.SparseConvTensor(features, ind, shape, batch)
        t = spconv.SparseConvTensor(features, coarse.indices, coarse.spatial_shape, batch)
        t.indice_dict = coarse.indice_dict
        return t

    rows = n if coarse is None else coarse.indices.size(0)
    return make, tensor, rows


def _module_run(mod, tensor, x, gy=None):
    xa = x.clone().requires_grad_(True)
    out = mod(tensor(xa))
    if gy is None:
        return out
    out.features.backward(gy)
    return out.features.detach(), xa.grad, mod.weight.grad, mod.bias.grad


@pytest.mark.parametrize('cin,cout', [(16, 32), (5, 7)])
@pytest.mark.parametrize('kind', ['subm', 'conv', 'inverse', 'transpose'])
def test_modules_at_bf16(kind, cin, cout):
    """10. SubMConv3d, SparseConv3d (stride 2), SparseInverseConv3d and SparseConvTranspose3d with set_precision('bf16'): forward
    and the three gradients against the float64 contraction of the rounded operands, beside the same module at 'f32' and at 'f32x6'
    fed rounded operands (backward: indice_conv_backward on rounded dY, x and w), bar of test 8; the bias and its gradient are
    untouched; a default module created beside the bf16 one is bit-equal to one that ran before any bf16 module existed.
    (5, 7) channels: no kernel of the new entry takes them - the rounded fallback, same bar."""
    from sst_amd import spconv
    make, tensor, rows = _module_setup(kind, cin, cout, seed=10 + cin)
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(rows, cin, generator=gen) * 2).to(DEV)
    first = make()                                            # before any bf16 module exists in this test
    assert first.precision is None
    probe = _module_run(first, tensor, x)
    gy = torch.randn(probe.features.shape, generator=gen).to(DEV)
    base = _module_run(first, tensor, x, gy)
    mb = make().set_precision('bf16')
    got = _module_run(mb, tensor, x, gy)
    beside = make()
    assert beside.precision is None and mb.precision == 'bf16'
    for a, b2, name in zip(base, _module_run(beside, tensor, x, gy), ('y', 'dx', 'dw', 'db')):
        assert torch.equal(a, b2), ('leak into a default module', name)
    assert not torch.equal(got[0], base[0]) and not torch.equal(got[1], base[1]) and not torch.equal(got[2], base[2])
    assert torch.equal(got[3], base[3])                       # the bias gradient: a column sum of dY, untouched
    # float64 references of the rounded operands, through the rulebook the module filed
    w = first.weight.detach()
    xr, wr, gyr = B.round_bf16(x), B.round_bf16(w), B.round_bf16(gy)
    t = tensor(x)
    outids, pairs, num, _ = mb._geometry(t)
    inverse, subm = kind == 'inverse', kind == 'subm'
    rb = spconv.rulebook_of(pairs, num, rows if inverse else outids.size(0))
    w3 = wr.reshape(-1, cin, cout)
    fwd_map, bwd_map, x_side = (rb.in2out, rb.out2in, 1) if inverse else (rb.out2in, rb.in2out, 0)
    num_l = [int(v) for v in num.cpu()]
    refs = (R.conv_ref(xr, fwd_map, w3, first.bias.detach()), R.conv_ref(gyr, bwd_map, w3.transpose(1, 2)),
            R.wgrad_ref(xr, gyr, pairs, num_l, x_side).reshape(w.shape))
    for mode in ('f32', 'f32x6'):
        em = make().set_precision(mode)
        with torch.no_grad():
            em.weight.copy_(wr)
        y_e = _module_run(em, tensor, xr).features.detach()
        dx_e, dw_e = spconv.indice_conv_backward(xr, wr, gyr, pairs, num, inverse, subm, precision=mode)
        if mode == 'f32':
            pipe = (y_e, dx_e, dw_e)
        else:
            x6 = (y_e, dx_e, dw_e)
    for name, g, p, e, ref in zip(('y', 'dx', 'dw'), got, pipe, x6, refs):
        what = '%s %d->%d %s' % (kind, cin, cout, name)
        _admissible(_err(g, ref), _err(p, ref), _scale(ref), what)
        _admissible(_err(e, ref), _err(p, ref), _scale(ref), what + " (the 'f32x6' module fed rounded operands)")


UNET_CFG = dict(in_channels=8, sparse_shape=[16, 40, 40], order=('conv', 'norm', 'act'),
                norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), base_channels=16, output_channels=32,
                encoder_channels=((16, ), (16, 16, 16), (32, 32, 32), (32, 32, 32)),
                encoder_paddings=((1, ), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)),
                decoder_channels=((32, 32, 32), (32, 32, 16), (16, 16, 16), (16, 16, 16)),
                decoder_paddings=((1, 0), (1, 0), (0, 0), (0, 1)))       # the construction of tests/test_gpu_sparse_unet.py


class _RoundForward(torch.autograd.Function):
    """round_bf16 on the way in, the gradient passes: what the 'bf16' mode does to a convolution's gathered rows"""

    @staticmethod
    def forward(ctx, t):
        return B.round_bf16(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBackward(torch.autograd.Function):
    """identity on the way in, round_bf16 on the gradient: what the 'bf16' mode does to a convolution's output gradient"""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return B.round_bf16(g)


def _emulated(net, mode):
    """a copy of the net whose every convolution runs the parent's kernels at `mode` on operands rounded around it: weights
    rounded (their gradients are the gradients of the masters: the rounding passes them), rows rounded in front, dY behind"""
    from sst_amd import spconv
    em = copy.deepcopy(net)
    for mod in em.modules():
        if isinstance(mod, spconv.SparseConvolution):
            mod.set_precision(mode)
            with torch.no_grad():
                mod.weight.copy_(B.round_bf16(mod.weight))
            mod.register_forward_pre_hook(lambda _m, args: (args[0].replace_feature(_RoundForward.apply(args[0].features)),))
            mod.register_forward_hook(lambda _m, _a, out: out.replace_feature(_RoundBackward.apply(out.features)))
    return em


def _unet_and_input():
    import sst_amd
    g = load_golden('sparse_unet.npz')
    net = sst_amd.SimpleSparseUNet(**UNET_CFG)
    net.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g if k.startswith('w::')}, strict=True)
    return (net.to(DEV), torch.from_numpy(g['in::features']).to(DEV), torch.from_numpy(g['in::indices']).to(DEV),
            torch.from_numpy(g['in::grad_out']).to(DEV))


def _unet_run(net, x, ind, gout, train):
    net.train(train)
    net.zero_grad(set_to_none=True)
    out = net({'voxel_feats': x, 'voxel_coors': ind})[0]['voxel_feats']
    (out.float() * gout).sum().backward()
    return out.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def test_simple_sparse_unet_at_bf16():
    """11. the small SimpleSparseUNet with set_precision('bf16') against the emulated net (operands rounded at every convolution,
    the parent's kernels at 'f32x6').  Bar max(4 G, 1e-6 x scale), G the gap - measured here - between that emulated net at 'f32x6'
    and at 'f32': the net's own fp32 ordering noise.  Output features with training-mode batch norm; every parameter gradient
    with batch norm in eval mode, each against its own G."""
    net, x, ind, gout = _unet_and_input()
    nb = copy.deepcopy(net).set_precision('bf16')
    e6, e32 = _emulated(net, 'f32x6'), _emulated(net, 'f32')
    y_b, _ = _unet_run(nb, x, ind, gout, True)
    y_6, _ = _unet_run(e6, x, ind, gout, True)
    y_32, _ = _unet_run(e32, x, ind, gout, True)
    y_d, _ = _unet_run(net, x, ind, gout, True)
    gap, err, scale = _err(y_6, y_32.double()), _err(y_b, y_6.double()), _scale(y_6)
    print('features: bf16 vs emulated %.3e  G %.3e  scale %.3e' % (err, gap, scale))
    assert err <= max(4 * gap, 1e-6 * scale), (err, gap, scale)
    assert _err(y_b, y_d.double()) > 100 * err                   # and the mode is another arithmetic than the default's
    _, g_b = _unet_run(nb, x, ind, gout, False)
    _, g_6 = _unet_run(e6, x, ind, gout, False)
    _, g_32 = _unet_run(e32, x, ind, gout, False)
    assert set(g_b) == set(g_6) == set(g_32) and len(g_b) > 40
    bad = []
    for name in sorted(g_b):
        gap, err, scale = _err(g_6[name], g_32[name].double()), _err(g_b[name], g_6[name].double()), _scale(g_6[name])
        print('%s: bf16 vs emulated %.3e  G %.3e  scale %.3e' % (name, err, gap, scale))
        if not err <= max(4 * gap, 1e-6 * scale):
            bad.append((name, err, gap, scale))
    assert not bad, bad


def test_fp16_key_of_the_sparse_unet():
    """12. model.half() on the U-Net: float16 features in, float16 features out, equal to the 'bf16' net's output (fed the same
    features as fp32) cast to half; the parameters are still fp32; an explicit set_precision wins over the request"""
    from sst_amd import _lib as L
    net, x, ind, _ = _unet_and_input()
    net.eval()
    nb = copy.deepcopy(net).set_precision('bf16')
    nh = copy.deepcopy(net).half()
    assert L.wants_half(nh) and all(p.dtype == torch.float32 for p in nh.parameters())
    assert all(b.dtype != torch.float16 for b in nh.buffers())
    xh = x.half()
    with torch.no_grad():
        out_h = nh({'voxel_feats': xh, 'voxel_coors': ind})[0]['voxel_feats']
        out_b = nb({'voxel_feats': xh.float(), 'voxel_coors': ind})[0]['voxel_feats']
        out_d = net({'voxel_feats': xh.float(), 'voxel_coors': ind})[0]['voxel_feats']
        assert out_h.dtype == torch.float16 and out_b.dtype == torch.float32
        assert torch.equal(out_h, out_b.half())
        nh.set_precision('f32x6')
        out_x = nh({'voxel_feats': xh, 'voxel_coors': ind})[0]['voxel_feats']
    assert out_x.dtype == torch.float16 and torch.equal(out_x, out_d.half()) and not torch.equal(out_b, out_d)
    assert all(p.dtype == torch.float32 for p in nh.parameters())
