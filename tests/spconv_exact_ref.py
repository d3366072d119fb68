"""Exact operands, adversarial maps / pair lists and the float64 reference of the sparse convolution kernels
(tests/test_spconv_exact_host.py without a GPU, tests/test_gpu_spconv_exact.py on one).

The contraction Y[r] = sum_k X[map[k][r]] W[k] (+ bias) and the filter gradient dW[k] = sum_p X[a_p]^T dY[b_p] are sums of
products.  When every product and every partial sum is a multiple of one granule and stays below 2^24 granules, each of them
is an fp32 number: a correct kernel returns the float64 result bit for bit, whatever its order, its split into tiles, offsets
or chunks, or its split of the operands into bf16 parts - and one wrong row, slab, column or offset is a hard mismatch.

Recipes ("fine" = the many-valued operand, "unit" = the other one; every entry drawn on its own, both signs and zeros):
  A  both operands integers in [-4, 4]                                   one bf16 part            every kernel
  B  unit in {-1, 0, 1}, fine = k / 1024, |k| <= 2047                    two parts                every kernel (the two-way
     split of the x3 kernel holds 16 bits and the product lo * lo it drops is zero: the unit side has one part)
  D  unit in {-1, 0, 1} with at most 4 non-zero terms per output element, fine = k / 2^20, |k| < 2^20
                                                                         three parts              fp32-pipe and x6 kernels
The condition (`assert_exact`) is asserted from the operands: the reference evaluated on |x|, |w| (|bias|) stays below 2^23
granules - half of what fp32 holds, because the leading bf16 part of a value rounds up to at most twice it."""
import ctypes

import numpy as np
import torch

GRANULE = {'A': 1.0, 'B': 2.0 ** -10, 'D': 2.0 ** -20}
LIMIT = 2 ** 23
MAP_FAMILIES = ('dense', 'random', 'sparse4', 'one_block', 'last_row', 'empty_tile', 'single_offset')


# ------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------
def values(recipe, fine, shape, gen):
    """fp32 CPU tensor of the recipe, `fine`: the many-valued operand (recipe A has one kind)"""
    ri = lambda lo, hi: torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()     # noqa: E731
    if recipe == 'A':
        return ri(-4, 4)
    if not fine:
        return ri(-1, 1)
    if recipe == 'B':
        return ri(-2047, 2047) / 1024.0
    assert recipe == 'D'
    return ri(-(2 ** 20 - 1), 2 ** 20 - 1) / 2.0 ** 20


def one_hot_rows(rows, c, gen):
    """unit operand of recipe D on the row side: every row has exactly one non-zero channel, +-1; the channels are dealt out
    evenly over the rows (every channel occurs when rows >= c), in random order"""
    t = torch.zeros(rows, c)
    ch = (torch.arange(rows) % c)[torch.randperm(rows, generator=gen)]
    t[torch.arange(rows), ch] = torch.randint(0, 2, (rows,), generator=gen).float() * 2 - 1
    return t


def one_hot_weights(kvol, cin, cout, gen):
    """unit operand of recipe D on the weight side: every (k, n) has exactly one non-zero input channel, +-1"""
    w = torch.zeros(kvol, cin, cout)
    ch = torch.randint(0, cin, (kvol, cout), generator=gen)
    sg = torch.randint(0, 2, (kvol, cout), generator=gen).float() * 2 - 1
    w.scatter_(1, ch[:, None, :], sg[:, None, :])
    return w


def conv_operands(recipe, fine, n_x, kvol, cin, cout, gen):
    """x [n_x, cin], w [kvol, cin, cout], bias [cout] of the recipe; fine: 'x' | 'w' (the bias is of the fine kind)"""
    if recipe == 'D':
        x = values('D', True, (n_x, cin), gen) if fine == 'x' else one_hot_rows(n_x, cin, gen)
        w = values('D', True, (kvol, cin, cout), gen) if fine == 'w' else one_hot_weights(kvol, cin, cout, gen)
    else:
        x = values(recipe, fine == 'x', (n_x, cin), gen)
        w = values(recipe, fine == 'w', (kvol, cin, cout), gen)
    return x, w, values(recipe, True, (cout,), gen)


def bf16_parts(x):
    """the three bf16 parts of fp32 values (round to nearest even), as fp32: p0 + p1 + p2 == x exactly"""
    r = lambda t: t.to(torch.bfloat16).to(torch.float32)     # noqa: E731
    p0 = r(x)
    p1 = r(x - p0)
    p2 = x - p0 - p1
    assert torch.equal(r(p2), p2) and torch.equal(p0 + p1 + p2, x)
    return p0, p1, p2


# ------------------------------------------------------------------------------------------------------------------------------
# maps of the contraction: [kvol, m] int32, -1 = no partner, partners in [lo, n_x)
# ------------------------------------------------------------------------------------------------------------------------------
def make_map(family, kvol, m, n_x, rng, lo=0):
    """the families of the module docstring of tests/test_gpu_spconv_exact.py; partners include the first and the last row of
    x and repeats (lo = 1: row 0 of x is never referenced)"""
    part = lambda shape: rng.integers(lo, n_x, shape).astype(np.int32)     # noqa: E731
    mp = np.full((kvol, m), -1, np.int32)
    rows = np.arange(m)
    if family == 'dense':
        mp = part((kvol, m))
    elif family == 'random':
        mp = np.where(rng.random((kvol, m)) < 0.5, part((kvol, m)), -1).astype(np.int32)
    elif family == 'sparse4':       # row r: exactly the offsets (4 r + j) mod kvol, j < 4 - every offset live in every 16-row block
        for j in range(4):
            mp[(4 * rows + j) % kvol, rows] = part(m)
    elif family == 'one_block':     # offset k of tile t: populated in the 16-row block (k + t) % 4 alone
        for k in range(kvol):
            sel = (rows // 16) % 4 == (k + rows // 64) % 4
            mp[k, sel] = part(int(sel.sum()))
    elif family == 'last_row':      # the last 64-row tile: one partner, in row m - 1; the tiles before it: about half of the slots
        mp = np.where(rng.random((kvol, m)) < 0.5, part((kvol, m)), -1).astype(np.int32)
        mp[:, (m - 1) // 64 * 64:] = -1
        mp[kvol // 2, m - 1] = n_x - 1
        return mp
    elif family == 'empty_tile':    # rows 0 .. 63 (a whole tile) and rows 80 .. 95 (the second wave's block of the next one) empty
        mp = np.where(rng.random((kvol, m)) < 0.5, part((kvol, m)), -1).astype(np.int32)
        mp[:, :64] = -1
        mp[:, 80:96] = -1
        return mp
    elif family == 'single_offset':
        mp[kvol - 1] = np.where(rng.random(m) < 0.5, part(m), -1)
    elif family == 'empty':
        return mp
    else:
        raise ValueError(family)
    # the first and the last row of x and a repeat, on slots the family populates
    live = np.argwhere(mp >= 0)
    if len(live) >= 3:
        (k0, r0), (k1, r1), (k2, r2) = live[0], live[-1], live[len(live) // 2]
        mp[k0, r0], mp[k1, r1], mp[k2, r2] = lo, n_x - 1, n_x - 1
    return mp


def check_map(mp, n_x):
    assert mp.dtype == np.int32 and mp.min() >= -1 and mp.max() < n_x


# ------------------------------------------------------------------------------------------------------------------------------
# pair lists of the filter gradient: [kvol, 2, pair_ld] int32, -1 behind num[k]; side 0 indexes rows0, side 1 rows1
# ------------------------------------------------------------------------------------------------------------------------------
def make_pairs(num, pair_ld, rows0, rows1, rng, hot=None):
    """random pairs with repeats, the first and the last row of either side among them.  hot = (side, channel of every row of
    that side, cap): the side carries one-hot rows (recipe D) and no channel may occur more than `cap` times among the rows an
    offset picks on it, so that no element of dW[k] receives more than `cap` terms"""
    kvol = len(num)
    assert max(num, default=0) <= pair_ld
    pairs = np.full((kvol, 2, pair_ld), -1, np.int32)
    by_channel = None
    if hot is not None:
        side, channel, cap = hot
        n_ch = int(channel.max()) + 1
        by_channel = [np.nonzero(channel == c)[0] for c in range(n_ch)]
        avail = np.array([c for c in range(n_ch) if len(by_channel[c])])
    for k, n in enumerate(num):
        if n == 0:
            continue
        a = rng.integers(0, rows0, n)
        b = rng.integers(0, rows1, n)
        a[0], b[0], a[-1], b[-1] = 0, rows1 - 1, rows0 - 1, 0
        if hot is not None:
            assert n <= cap * len(avail), (n, cap, len(avail))
            chans = rng.permutation(np.repeat(avail, cap))[:n]
            pick = np.array([by_channel[c][rng.integers(0, len(by_channel[c]))] for c in chans])
            if side == 0:
                a = pick
            else:
                b = pick
        pairs[k, 0, :n], pairs[k, 1, :n] = a, b
    return pairs


# ------------------------------------------------------------------------------------------------------------------------------
# the reference: the definition in float64, per offset gather / matmul / index-add (as oracle/spconv_oracle.py), in torch so
# that it may run on the device
# ------------------------------------------------------------------------------------------------------------------------------
def conv_ref(x, mp, w, bias=None):
    """x [n_x, cin], mp [kvol, m] (tensor), w [kvol, cin, cout] -> float64 [m, cout]"""
    xd, wd = x.double(), w.double()
    y = torch.zeros(mp.size(1), w.size(2), dtype=torch.float64, device=x.device)
    for k in range(mp.size(0)):
        rows = torch.nonzero(mp[k] >= 0)[:, 0]
        if rows.numel():
            y.index_add_(0, rows, xd[mp[k][rows].long()] @ wd[k])
    if bias is not None:
        y += bias.double()
    return y


def wgrad_ref(x, dy, pairs, num, x_side):
    """x [*, cin], dy [*, cout], pairs [kvol, 2, pair_ld] (tensor), num: list -> float64 [kvol, cin, cout]"""
    xd, dyd = x.double(), dy.double()
    dw = torch.zeros(len(num), x.size(1), dy.size(1), dtype=torch.float64, device=x.device)
    for k, n in enumerate(num):
        if n:
            dw[k] = xd[pairs[k, x_side, :n].long()].t() @ dyd[pairs[k, 1 - x_side, :n].long()]
    return dw


def assert_exact(recipe, abs_ref):
    """the exactness condition, from the reference on the absolute values of the operands - before anything is launched"""
    top = float(abs_ref.max()) / GRANULE[recipe] if abs_ref.numel() else 0.0
    assert top < LIMIT, 'recipe %s: %.0f granules reach an output element, the condition allows %d' % (recipe, top, LIMIT)


def assert_conv_exact(recipe, x, mp, w, bias=None):
    assert_exact(recipe, conv_ref(x.abs(), mp, w.abs(), None if bias is None else bias.abs()))


def assert_wgrad_exact(recipe, x, dy, pairs, num, x_side):
    assert_exact(recipe, wgrad_ref(x.abs(), dy.abs(), pairs, num, x_side))


# ------------------------------------------------------------------------------------------------------------------------------
# CPU emulation of the three accumulation schemes on a list of products (terms [T, n] of a [T, n] x [T, n] pair)
# ------------------------------------------------------------------------------------------------------------------------------
def _chain(terms, gen):
    """fp32 accumulation one term after the other, in random order"""
    s = torch.zeros(terms.size(1))
    for t in torch.randperm(terms.size(0), generator=gen).tolist():
        s = s + terms[t]
    return s


def emulate(mode, a, b, gen):
    """sum_t a[t] * b[t] as the kernels form it: 'f32' one fp32 chain; 'x3' the two-way bf16 split, a0 b0 + a1 b0 + a0 b1 in
    one chain; 'x6' the three-way split, the leading product a0 b0 in one chain and the five corrections in another, the
    chains added at the end.  Every product of two bf16 parts is an fp32 number."""
    if mode == 'f32':
        return _chain(a * b, gen)
    pa, pb = bf16_parts(a), bf16_parts(b)
    if mode == 'x3':
        return _chain(torch.cat([pa[0] * pb[0], pa[1] * pb[0], pa[0] * pb[1]]), gen)
    assert mode == 'x6'
    cor = torch.cat([pa[i] * pb[j] for i, j in ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0))])
    return _chain(pa[0] * pb[0], gen) + _chain(cor, gen)


# ------------------------------------------------------------------------------------------------------------------------------
# the launch plan, asked of the library (include/sst_amd.h: sst_spconv_conv_os_plan, sst_spconv_wgrad_os_plan)
# ------------------------------------------------------------------------------------------------------------------------------
F32, F32X3, F32X6, ROWS_F32X6 = 0, 1, 2, 3      # SST_SPCONV_OS_ENTRY_*


def conv_plan(entry, m, kvol, cin, cout, tile_cfg=0, workspace_bytes=0):
    """(return code, rows per tile, columns per workgroup, n_split, workgroups launched)"""
    from sst_amd import _lib
    rows, cols, split, wgs = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = _lib.load().sst_spconv_conv_os_plan(entry, m, kvol, cin, cout, tile_cfg, workspace_bytes, ctypes.byref(rows),
                                             ctypes.byref(cols), ctypes.byref(split), ctypes.byref(wgs))
    return rc, rows.value, cols.value, split.value, wgs.value


def wgrad_plan(kvol, pair_ld, total_pairs, cin, cout):
    """(return code, pairs per chunk, chunk slots)"""
    from sst_amd import _lib
    chunk, slots = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = _lib.load().sst_spconv_wgrad_os_plan(kvol, pair_ld, total_pairs, cin, cout, ctypes.byref(chunk), ctypes.byref(slots))
    return rc, chunk.value, slots.value
