"""GPU: the sparse 3-D convolution kernels (csrc/spconv_os.hip, csrc/spconv_os_x3.hip, csrc/spconv_os_x6.hip and the
first-generation kernels of csrc/spconv.hip) with EXACT operands at every edge.

Operands, maps, pair lists, the float64 reference and the exactness condition: tests/spconv_exact_ref.py (host tests of them:
tests/test_spconv_exact_host.py).  Under the condition a correct kernel returns the float64 result bit for bit, so every
comparison below is `==` - there is no tolerance in this file.  The C entries are called directly, on synthetic maps and pair
lists (every index in range), with destinations pre-filled with a sentinel and workspaces pre-filled with NaN; which kernel
shape, offset split and chunk size a call takes is asked of the library (sst_spconv_conv_os_plan, sst_spconv_wgrad_os_plan),
never restated here.

Map families (R.make_map): dense | random (half of the slots absent) | sparse4 (row r has exactly the offsets (4 r + j) mod
kvol: at most 4 partners per row, every offset live in every 16-row block - the family of recipe D) | one_block (an offset is
populated in a single 16-row block of a tile) | last_row (the only partner of the last tile sits in row m - 1) | empty_tile (a
whole 64-row tile and, elsewhere, a whole wave's block without a partner) | single_offset (only offset kvol - 1 is live) |
empty (no partner at all)."""
import numpy as np
import pytest
import torch

import spconv_exact_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.5
N_X = 97                                     # rows of x of the small cases
OS_ENTRIES = [('os', 41), ('os', 42), ('os', 81), ('os', 82), ('os', 0)]
GG_ENTRIES = [('gg', 1), ('gg', 2)]
ROWS_ENTRIES = [('rows', 1), ('rows', 2), ('rows', 4), ('rows', 8)]
FIVE = [('A', 'x'), ('B', 'x'), ('B', 'w'), ('D', 'x'), ('D', 'w')]       # (recipe, the fine side)


def _entries(recipe, first_generation=True):
    """every contraction entry the recipe is exact for: D does not go to the two-way split of the x3 kernel"""
    e = OS_ENTRIES + ([] if recipe == 'D' else [('x3',)]) + [('x6',)] + ROWS_ENTRIES
    return e + (GG_ENTRIES if first_generation else [])


def _lib():
    from sst_amd import _lib as L
    return L, L.load()


def _nan_bytes(nbytes):
    """a workspace whose every word is NaN, as fp32 and as a pair of bf16: an unwritten slab or partial that gets read shows"""
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
# the contraction
# ------------------------------------------------------------------------------------------------------------------------------
class _Conv:
    """operands of one contraction on the device: x as [n_x, cin] and inside a [n_x, cin + 4] buffer of sentinels, w as
    [K, cin, cout] and as [K, cout, cin] (trans_w), the bias 16-byte aligned and offset by one float"""

    def __init__(self, recipe, fine, kvol, cin, cout, seed, n_x=N_X, nan_row0=False):
        gen = torch.Generator().manual_seed(seed)
        self.recipe, self.fine, self.kvol, self.cin, self.cout, self.n_x = recipe, fine, kvol, cin, cout, n_x
        x, w, bias = R.conv_operands(recipe, fine, n_x, kvol, cin, cout, gen)
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

    def want(self, mp, bias=True):
        """float64 reference, its exactness asserted from the operands, as fp32"""
        x = self.x.clone()
        x[0] = torch.nan_to_num(x[0])
        b = self.bias if bias else None
        R.assert_conv_exact(self.recipe, x, mp, self.w, b)
        y = R.conv_ref(x, mp, self.w, b)
        out = y.float()
        assert torch.equal(out.double(), y)
        return out


def _conv_call(entry, c, mp, m, y, ldy, trans_w=0, bias=None, x=None, ldx=None, order=None, expect_split=None):
    """one C entry on a NaN workspace of the queried size; `y`: the first element of the destination.  ('rows', s): the rows
    entry offered room for the partial tiles of s splits - what it really takes is confirmed through the plan query"""
    L, lib = _lib()
    x = c.x if x is None else x
    ldx = c.cin if ldx is None else ldx
    kvol, cin, cout = c.kvol, c.cin, c.cout
    head = (L.ptr(x), ldx, L.ptr(mp), m, kvol, L.ptr(c.w_stored[trans_w]), cin, cout, trans_w, L.ptr(bias), L.ptr(y), ldy)
    kind = entry[0]
    if kind == 'gg':
        return lib.sst_spconv_gather_gemm_f32(*head, entry[1], L.stream_ptr())
    if kind == 'os':
        ws = _nan_bytes(lib.sst_spconv_conv_os_workspace_bytes(kvol, cin, cout))
        return lib.sst_spconv_conv_os_f32(*head, entry[1], L.ptr(order), L.ptr(ws), L.stream_ptr())
    if kind == 'x3':
        ws = _nan_bytes(lib.sst_spconv_conv_os_workspace_bytes(kvol, cin, cout))
        return lib.sst_spconv_conv_os_f32x3(*head, 0, L.ptr(order), L.ptr(ws), L.stream_ptr())
    if kind == 'x6':
        ws = _nan_bytes(lib.sst_spconv_conv_os_f32x6_workspace_bytes(kvol, cin, cout))
        return lib.sst_spconv_conv_os_f32x6(*head, 0, L.ptr(order), L.ptr(ws), L.stream_ptr())
    assert kind == 'rows'
    nbytes = _rows_bytes(c, m, entry[1])
    if expect_split is not None:
        assert R.conv_plan(R.ROWS_F32X6, m, kvol, cin, cout, 0, nbytes)[3] == expect_split, (m, entry, expect_split)
    ws = _nan_bytes(nbytes)
    assert ws.data_ptr() % 256 == 0
    return lib.sst_spconv_conv_os_rows_f32x6(*head, 0, L.ptr(order), L.ptr(ws), nbytes, L.stream_ptr())


def _rows_bytes(c, m, splits):
    """the packed weights and room for the partial tiles of `splits` workgroups per unit (1: the packed weights alone)"""
    _, lib = _lib()
    pack = (lib.sst_spconv_conv_os_f32x6_workspace_bytes(c.kvol, c.cin, c.cout) + 255) // 256 * 256
    return pack if splits == 1 else pack + splits * m * ((c.cout + 3) // 4 * 4) * 4


def _natural_split(c, m):
    """the split the rows entry takes when it is offered all it asks for"""
    _, lib = _lib()
    full = lib.sst_spconv_conv_os_f32x6_workspace_bytes_rows(c.kvol, c.cin, c.cout, m)
    rc, _, _, split, _ = R.conv_plan(R.ROWS_F32X6, m, c.kvol, c.cin, c.cout, 0, full)
    assert rc == 0
    return split


def _run_layout(tally, entry, c, mp, m, want, what, trans_w=0, layout=0, order=None, bias=True):
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
    split = min(entry[1], _natural_split(c, m)) if entry[0] == 'rows' else None
    rc = _conv_call(entry, c, mp, m, y0, ldy, trans_w, b, x, ldx, order, split)
    assert rc == 0, (what, rc)
    expect = torch.full_like(buf, SENTINEL)
    off = 1 if layout == 2 else 0
    expect[off:off + (m + 2) * ldy].view(m + 2, ldy)[:m, :cout] = want[:m]
    tally.same(buf, expect, what)


M_SWEEP = 258


@pytest.mark.parametrize('recipe,fine', FIVE)
def test_row_sweep_every_m_from_1_to_258(recipe, fine):
    """every m of 1 .. 258 (twice the 128-row tile and a margin) on column prefixes of one map, kvol 27, 16 -> 32 channels:
    the ragged last tile with its `row >= m` returns in all of its 64 / 128 positions, waves without a row, one tile and
    several; every contraction entry (D: not the x3 one), the rows entry at each n_split of 1, 2, 4, 8 - steered by the
    workspace it is offered, confirmed by the plan query - equal to the reference and so to the unsplit call, bit for bit"""
    c = _Conv(recipe, fine, 27, 16, 32, seed=100 + ord(recipe) + (fine == 'w'))
    rng = np.random.default_rng(258)
    full = R.make_map('sparse4' if recipe == 'D' else 'random', 27, M_SWEEP, N_X, rng)
    R.check_map(full, N_X)
    mp_full = torch.from_numpy(full).to(DEV)
    want = c.want(mp_full)
    tally = _Tally()
    for m in range(1, M_SWEEP + 1):
        mp = mp_full[:, :m].contiguous()
        for entry in _entries(recipe):
            _run_layout(tally, entry, c, mp, m, want, 'm=%d (%%16=%d %%64=%d) %s' % (m, m % 16, m % 64, entry))
    tally.finish()


@pytest.mark.parametrize('kvol', [1, 8, 27, 32])
def test_map_shapes(kvol):
    """every map family at m = 64, 65 and 191 and kvol = 1, 8, 27, 32 (the most the index image holds), recipes A and B on all
    families and D on sparse4: a tile with no live offset at all (output = bias), a wave whose 16 rows have no partner, an
    offset that is live in one block only.  The rows entry with every workspace: at kvol = 27 it takes n_split = 8 and with a
    single_offset map seven of its eight workgroups per unit own no live offset and must write zeros (at kvol = 8 the library
    deals the 8 offsets out over fewer workgroups - whatever the plan query reports, all but one own nothing)."""
    rng = np.random.default_rng(kvol)
    tally = _Tally()
    convs = {rf: _Conv(rf[0], rf[1], kvol, 16, 32, seed=200 + kvol + 7 * i) for i, rf in enumerate(FIVE)}
    for m in (64, 65, 191):
        natural = _natural_split(convs[('A', 'x')], m)
        assert natural == {1: 1, 27: 8, 32: 8}.get(kvol, natural) and (kvol == 1 or natural > 1), (kvol, m, natural)
        for fam in R.MAP_FAMILIES + ('empty',):
            mp_np = R.make_map(fam, kvol, m, N_X, rng)
            R.check_map(mp_np, N_X)
            mp = torch.from_numpy(mp_np).to(DEV)
            for rf in FIVE[:2] + (FIVE[3:] if fam == 'sparse4' else []):
                c = convs[rf]
                want = c.want(mp)
                for entry in _entries(rf[0]):
                    _run_layout(tally, entry, c, mp, m, want, 'kvol=%d m=%d %s %s%s %s' % ((kvol, m, fam) + rf + (entry,)))
    tally.finish()


def _shape_cases(cin, cout, kvol, entries_of, ms):
    tally = _Tally()
    rng = np.random.default_rng(cin * 1000 + cout)
    for i, (recipe, fine) in enumerate(FIVE):
        c = _Conv(recipe, fine, kvol, cin, cout, seed=300 + cin + cout + 11 * i)
        # B: about half of the kvol * cin slots while that is within the condition, else 4 partners per row
        fam = 'sparse4' if recipe == 'D' or (recipe == 'B' and kvol * cin > 4096) else 'random'
        for m in ms:
            mp_np = R.make_map(fam, kvol, m, N_X, rng)
            R.check_map(mp_np, N_X)
            mp = torch.from_numpy(mp_np).to(DEV)
            wants = {True: c.want(mp, True), False: c.want(mp, False)}
            for trans_w in (0, 1):
                for entry in entries_of(recipe):
                    for layout, bias in ((0, True), (1, False), (2, True), (3, True), (0, False)):
                        _run_layout(tally, entry, c, mp, m, wants[bias], '%d->%d m=%d %s%s trans_w=%d %s layout %d bias %d'
                                    % (cin, cout, m, recipe, fine, trans_w, entry, layout, bias), trans_w, layout, None, bias)
    tally.finish()


@pytest.mark.parametrize('cin,cout', [(4, 4), (12, 20), (16, 7), (64, 64), (64, 66), (68, 132), (128, 160), (256, 256)])
def test_channel_shapes_output_stationary(cin, cout):
    """the output-stationary entries (fp32 at every tile_cfg, x3, x6, the rows entry split and unsplit) on channel counts that
    are one chunk, several, ragged in cin (68) and in cout (7, 66, 132: not a multiple of 4 reaches the scalar stores of the
    last column tile), both weight orientations, ragged m, and five operand layouts (_run_layout): row strides larger than the
    channel counts, y and the bias 16-byte aligned and offset by one float, with and without a bias"""
    def entries(recipe):
        return [e for e in _entries(recipe, first_generation=False) if e not in (('rows', 2), ('rows', 4))]
    _shape_cases(cin, cout, 27, entries, (1, 67, 150))


@pytest.mark.parametrize('cin,cout', [(5, 7), (6, 16), (67, 128)])
def test_channel_shapes_first_generation(cin, cout):
    """sst_spconv_gather_gemm_f32, which every layer with cin % 4 != 0 takes: forms 1 and 2 (with trans_w form 2 hands over
    to the tiled kernel), the same layouts and orientations; fp32 FMA / fp32 MFMA accumulation is exact under all recipes"""
    _shape_cases(cin, cout, 27, lambda recipe: GG_ENTRIES, (1, 67, 150))


def _first_m_with_128_columns(entry, kvol, cin, cout, limit=300000):
    """the smallest m at which the entry takes 128 columns per workgroup, by bisection in the plan query (the choice is
    monotone in m: more row tiles only add workgroups)"""
    cols = lambda m: R.conv_plan(entry, m, kvol, cin, cout)[2]     # noqa: E731
    assert cols(limit) == 128, 'the 128-column kernel of entry %d is out of reach below %d rows' % (entry, limit)
    lo, hi = 1, limit                                     # cols(lo) == 64 < cols(hi) == 128
    assert cols(lo) == 64
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if cols(mid) == 128 else (mid, hi)
    return hi


def test_128_column_kernels():
    """sp_conv_os_x3_k<8> and sp_conv_os_x6_k<8>, which no other test reaches: the smallest m at which the library picks them
    (found in the plan query), cout = 132 so that the second column group has 4 live columns, cin = 8, kvol = 27, x of 4 096
    rows; at that m, at m + 63, and at m - 1, which must still be the 64-column kernel.  Recipe A for both, recipe D (both ways
    round) for x6."""
    kvol, cin, cout, n_x = 27, 8, 132, 4096
    m0 = {e: _first_m_with_128_columns(e, kvol, cin, cout) for e in (R.F32X3, R.F32X6)}
    assert m0[R.F32X3] == m0[R.F32X6]
    m0 = m0[R.F32X6]
    tally = _Tally()
    rng = np.random.default_rng(128)
    for recipe, fine, entries in (('A', 'x', (('x3',), ('x6',))), ('D', 'x', (('x6',),)), ('D', 'w', (('x6',),))):
        c = _Conv(recipe, fine, kvol, cin, cout, seed=128 + ord(recipe), n_x=n_x)
        full = R.make_map('sparse4', kvol, m0 + 63, n_x, rng)
        R.check_map(full, n_x)
        mp_full = torch.from_numpy(full).to(DEV)
        want = c.want(mp_full)
        for m, cols in ((m0 - 1, 64), (m0, 128), (m0 + 63, 128)):
            mp = mp_full[:, :m].contiguous()
            for entry in entries:
                kind = R.F32X3 if entry == ('x3',) else R.F32X6
                assert R.conv_plan(kind, m, kvol, cin, cout)[2] == cols
                _run_layout(tally, entry, c, mp, m, want, 'm=%d %d columns %s%s %s' % (m, cols, recipe, fine, entry))
    tally.finish()


def test_launch_numbering_and_tile_order():
    """workgroup counts just below and just above the switch to XCD runs of 4 (250 and 261 row tiles; 31 and 33 row tiles at
    n_split = 8), none a multiple of 32: below it the grid is padded to a round of 8 at most, above it to whole rounds of
    runs, with idle workgroups behind the last unit (read off the plan query).  At the same sizes a random permutation and the
    reversed order as d_tile_order: the bits are those of the call without it."""
    kvol, cin, cout = 27, 16, 32
    c = _Conv('A', 'x', kvol, cin, cout, seed=400)
    rng = np.random.default_rng(400)
    tally = _Tally()
    plans = {R.F32: [('os', 0)], R.F32X3: [('x3',)], R.F32X6: [('x6',)]}
    cases = [(250 * 64 - 9, plans, False), (261 * 64 - 30, plans, True), (31 * 64 - 5, {R.ROWS_F32X6: [('rows', 8)]}, False),
             (33 * 64 - 7, {R.ROWS_F32X6: [('rows', 8)]}, True), (261 * 64 - 30, {R.F32: [('os', 42)]}, None)]
    for m, by_kind, above in cases:
        mp_np = R.make_map('random', kvol, m, N_X, rng)
        R.check_map(mp_np, N_X)
        mp = torch.from_numpy(mp_np).to(DEV)
        want = c.want(mp)
        for kind, entries in by_kind.items():
            for entry in entries:
                nbytes = _rows_bytes(c, m, 8) if entry[0] == 'rows' else 0
                rc, rows, cols, split, wgs = R.conv_plan(kind, m, kvol, cin, cout, entry[1] if entry[0] == 'os' else 0, nbytes)
                live = -(-m // rows) * -(-cout // cols) * split
                assert rc == 0 and split == (8 if entry[0] == 'rows' else 1) and live % 32 != 0
                if above is False:
                    assert wgs - live < 8, (entry, m, live, wgs)
                if above is True:
                    assert wgs % 32 == 0 and wgs - live >= 8, (entry, m, live, wgs)
                n_tiles = -(-m // rows)
                perm = torch.from_numpy(rng.permutation(n_tiles).astype(np.int32)).to(DEV)
                rev = torch.arange(n_tiles - 1, -1, -1, dtype=torch.int32, device=DEV)
                for name, order in (('row order', None), ('random order', perm), ('reversed order', rev)):
                    _run_layout(tally, entry, c, mp, m, want, 'm=%d %s %s (%d of %d workgroups live)' % (m, entry, name, live, wgs),
                                order=order)
    tally.finish()


def test_absent_partners_select_zero():
    """the kernels read row 0 of x for an absent partner and must SELECT zero, not multiply by it: with a map that never
    references row 0 and NaN in that row, every entry still equals the reference"""
    tally = _Tally()
    rng = np.random.default_rng(7)
    for i, (recipe, fine) in enumerate(FIVE):
        c = _Conv(recipe, fine, 27, 16, 32, seed=500 + i, nan_row0=True)
        assert bool(torch.isnan(c.x[0]).all())
        for fam in (('sparse4',) if recipe == 'D' else ('random', 'one_block', 'empty_tile', 'single_offset')):
            m = 191
            mp_np = R.make_map(fam, 27, m, N_X, rng, lo=1)
            R.check_map(mp_np, N_X)
            assert (mp_np != 0).all()
            mp = torch.from_numpy(mp_np).to(DEV)
            want = c.want(mp)
            for entry in _entries(recipe):
                _run_layout(tally, entry, c, mp, m, want, 'NaN in row 0: %s%s %s %s' % (recipe, fine, fam, entry))
    tally.finish()


def test_contraction_refusals_launch_nothing():
    """cin % 4 != 0, ldx % 4 != 0, x not 16-byte aligned, kvol = 33, a non-zero tile_cfg on the split entries and a workspace
    below the packed weights: each returns its error code, and neither the destination nor the workspace is touched"""
    L, lib = _lib()
    m = 70
    ws = _nan_bytes(1 << 20)
    y = torch.full((m, 32), SENTINEL, device=DEV)
    xbuf = torch.zeros(N_X * 24 + 4, device=DEV)
    w = torch.zeros(33 * 16 * 32, device=DEV)
    mp = torch.full((33, m), -1, dtype=torch.int32, device=DEV)
    UNS, ARG = L.SST_ERR_UNSUPPORTED, L.SST_ERR_ARG

    def call(kind, x=xbuf, ldx=16, kvol=27, cin=16, tile_cfg=0, nbytes=1 << 20):
        head = (L.ptr(x), ldx, L.ptr(mp), m, kvol, L.ptr(w), cin, 32, 0, None, L.ptr(y), 32, tile_cfg, None, L.ptr(ws))
        if kind == 'rows':
            return lib.sst_spconv_conv_os_rows_f32x6(*head, nbytes, L.stream_ptr())
        fn = {'os': lib.sst_spconv_conv_os_f32, 'x3': lib.sst_spconv_conv_os_f32x3, 'x6': lib.sst_spconv_conv_os_f32x6}[kind]
        return fn(*head, L.stream_ptr())

    for kind in ('os', 'x3', 'x6', 'rows'):
        assert call(kind, cin=6, ldx=8) == UNS, kind
        assert call(kind, ldx=18) == UNS, kind
        assert call(kind, x=xbuf[1:]) == UNS, kind
        assert call(kind, kvol=33) == UNS, kind
        if kind != 'os':
            assert call(kind, tile_cfg=41) == ARG, kind
    assert call('os', tile_cfg=43) == ARG
    pack = lib.sst_spconv_conv_os_f32x6_workspace_bytes(27, 16, 32)
    assert call('rows', nbytes=pack // 4) == ARG
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((ws == 0xFF).all())


# ------------------------------------------------------------------------------------------------------------------------------
# the filter gradient
# ------------------------------------------------------------------------------------------------------------------------------
WG_ENTRIES = ('sst_spconv_wgrad_os_f32', 'sst_spconv_wgrad_os_f32x6', 'sst_spconv_wgrad_f32')
WG_FIVE = [('A', 'x'), ('B', 'x'), ('B', 'dy'), ('D', 'x'), ('D', 'dy')]


class _Wgrad:
    """x [rows_x, cin] and dy [rows_dy, cout] of a recipe on the device, inside buffers with wider rows; D: the unit side
    has one-hot rows, every channel among them, and `cap` = 4 x its channels bounds the pairs of an offset"""

    def __init__(self, recipe, fine, cin, cout, seed, wide=False):
        gen = torch.Generator().manual_seed(seed)
        self.recipe, self.fine, self.cin, self.cout = recipe, fine, cin, cout
        ROWS_X, ROWS_DY = max(90, cin + 7), max(70, cout + 5)
        self.rows_x, self.rows_dy = ROWS_X, ROWS_DY
        if recipe == 'D':
            x = R.values('D', True, (ROWS_X, cin), gen) if fine == 'x' else R.one_hot_rows(ROWS_X, cin, gen)
            dy = R.values('D', True, (ROWS_DY, cout), gen) if fine == 'dy' else R.one_hot_rows(ROWS_DY, cout, gen)
            unit = dy if fine == 'x' else x
            self.channel = unit.abs().argmax(1).numpy()
            self.cap = 4 * unit.size(1)
        else:
            x, dy = R.values(recipe, fine == 'x', (ROWS_X, cin), gen), R.values(recipe, fine == 'dy', (ROWS_DY, cout), gen)
            self.channel, self.cap = None, 1 << 30
        self.ldx, self.lddy = (cin + 4, cout + 8) if wide else (cin, cout)
        bx = torch.full((ROWS_X, self.ldx), SENTINEL, device=DEV)
        bdy = torch.full((ROWS_DY, self.lddy), SENTINEL, device=DEV)
        bx[:, :cin], bdy[:, :cout] = x.to(DEV), dy.to(DEV)
        self.x, self.dy = bx[:, :cin], bdy[:, :cout]

    def pairs(self, num, pair_ld, x_side, rng):
        """[kvol, 2, pair_ld] on the device; side x_side indexes x"""
        rows = (self.rows_x, self.rows_dy) if x_side == 0 else (self.rows_dy, self.rows_x)
        hot = None
        if self.recipe == 'D':
            hot = ((1 - x_side) if self.fine == 'x' else x_side, self.channel, 4)
        p = R.make_pairs(num, pair_ld, rows[0], rows[1], rng, hot)
        for side in (0, 1):
            assert p[:, side].min() >= -1 and p[:, side].max() < rows[side]
        return torch.from_numpy(p).to(DEV)

    def want(self, pairs, num, x_side):
        R.assert_wgrad_exact(self.recipe, self.x, self.dy, pairs, num, x_side)
        dw = R.wgrad_ref(self.x, self.dy, pairs, num, x_side)
        out = dw.float()
        assert torch.equal(out.double(), dw)
        for k, n in enumerate(num):
            assert n or not bool(out[k].any())            # no pairs: exactly zero
        return out


def _wgrad_call(entry, g, pairs, num_dev, total, x_side):
    """one C entry on a NaN workspace of the queried size into a sentinel-filled dW"""
    L, lib = _lib()
    kvol, pair_ld = pairs.size(0), pairs.size(2)
    query = lib.sst_spconv_wgrad_workspace_bytes if entry == 'sst_spconv_wgrad_f32' else lib.sst_spconv_wgrad_os_workspace_bytes
    ws = _nan_bytes(query(kvol, pair_ld, total, g.cin, g.cout))
    dw = torch.full((kvol, g.cin, g.cout), SENTINEL, device=DEV)
    rc = getattr(lib, entry)(L.ptr(g.x), g.ldx, L.ptr(g.dy), g.lddy, L.ptr(pairs), pair_ld, total, x_side, L.ptr(num_dev), kvol,
                             g.cin, g.cout, L.ptr(dw), L.ptr(ws), L.stream_ptr())
    assert rc == 0, (entry, rc)
    return dw


def _wgrad_entries(g):
    return WG_ENTRIES if g.cin % 4 == 0 and g.cout % 4 == 0 else WG_ENTRIES[2:]


def _wgrad_run(tally, g, num, pair_ld, rng, what):
    """every entry, x_side 0 and 1, total_pairs exact and -1 (the upper-bound sizing of the Python side): all equal to the
    reference, hence to each other"""
    num = [int(v) for v in num]
    assert max(num) <= g.cap
    num_dev = torch.tensor(num, dtype=torch.int32, device=DEV)
    for x_side in (0, 1):
        pairs = g.pairs(num, pair_ld, x_side, rng)
        want = g.want(pairs, num, x_side)
        for entry in _wgrad_entries(g):
            for total in (sum(num), -1):
                got = _wgrad_call(entry, g, pairs, num_dev, total, x_side)
                tally.same(got, want, '%s %s%s %s x_side=%d total_pairs=%d' % (what, g.recipe, g.fine, entry, x_side, total))


@pytest.mark.parametrize('recipe,fine', WG_FIVE)
def test_filter_gradient_every_pair_count_from_0_to_161(recipe, fine):
    """num[k] = base + k over six launches: every count of 0 .. 161 (the 64-pair stage tail in all of its positions, one and
    several stages), then all offsets empty, and a single pair in one offset; the three entries, 16 -> 32 channels.  D: up to
    4 x the channels of its unit side per offset (the launches whose counts stay within that)"""
    g = _Wgrad(recipe, fine, 16, 32, seed=600 + ord(recipe) + (fine == 'x'))
    rng = np.random.default_rng(161)
    tally = _Tally()
    launches = [[base + k for k in range(27)] for base in range(0, 136, 27)]
    launches = [n for n in launches if max(n) <= g.cap] + [[min(v, g.cap) for v in launches[-1]]] * (recipe == 'D')
    launches += [[0] * 27, [0] * 13 + [1] + [0] * 13]
    assert recipe == 'D' or sorted(set(v for n in launches for v in n)) == list(range(162))
    for num in launches:
        _wgrad_run(tally, g, num, 192, rng, 'counts %d..%d' % (min(num), max(num)))
    tally.finish()


def _edge_counts(kvol, pair_ld, total, cin, cout, counts_of):
    """num [kvol] summing to `total`: the counts counts_of(c) around the chunk size c the library takes for this total, beside
    an empty offset, a single pair and three pairs, the rest dealt out over the remaining offsets"""
    rc, c, _ = R.wgrad_plan(kvol, pair_ld, total, cin, cout)
    assert rc == 0
    num = [0, 1, 3] + counts_of(c)
    rest, free = total - sum(num), kvol - len(num) - 1
    assert rest >= 0 and free > 0 and -(-rest // free) <= pair_ld and max(num) <= pair_ld
    num += [rest // free + (i < rest % free) for i in range(free)] + [0]
    assert len(num) == kvol and sum(num) == total
    return c, num


@pytest.mark.parametrize('cin,cout,total,pair_ld,chunk', [(16, 32, 5000, 1100, 512), (256, 256, 24000, 1800, None),
                                                          (256, 256, 35000, 4200, 2048)])
def test_filter_gradient_chunk_edges(cin, cout, total, pair_ld, chunk):
    """counts of c - 1, c, c + 1, 2 c and 2 c + 1 pairs, c the chunk size asked of the plan query, in three operand sets whose
    plan gives 512 pairs, an intermediate size and 2048: an exact multiple of the chunk (no tail chunk, and none too many),
    one pair in a chunk of its own, the slot lookup across empty and tiny offsets; recipes A and B; D where 4 x 256 pairs per
    offset reach (c - 1, c, c + 1 and 2 c of the 512-pair chunk at 256 channels)"""
    rng = np.random.default_rng(total)
    tally = _Tally()
    c, num = _edge_counts(27, pair_ld, total, cin, cout, lambda c: [c - 1, c, c + 1, 2 * c, 2 * c + 1])
    assert 512 <= c <= 2048 and (c == chunk if chunk else 512 < c < 2048), c
    _, c_bound, slots_bound = R.wgrad_plan(27, pair_ld, -1, cin, cout)
    assert slots_bound >= sum(-(-n // c_bound) for n in num)
    for i, (recipe, fine) in enumerate(WG_FIVE[:3]):
        g = _Wgrad(recipe, fine, cin, cout, seed=700 + i + cin)
        _wgrad_run(tally, g, num, pair_ld, rng, 'chunk %d' % c)
    if chunk == 512:
        cd, num_d = _edge_counts(27, 1024, 6000, 256, 256, lambda c: [c - 1, c, c + 1, 2 * c])
        assert cd == 512
        for i, (recipe, fine) in enumerate(WG_FIVE[3:]):
            g = _Wgrad(recipe, fine, 256, 256, seed=750 + i)
            _wgrad_run(tally, g, num_d, 1024, rng, 'chunk %d' % cd)
    tally.finish()


@pytest.mark.parametrize('cin,cout', [(4, 4), (16, 32), (64, 64), (68, 132), (256, 256), (5, 7)])
def test_filter_gradient_channel_shapes(cin, cout):
    """one 64 x 64 block of dW[k], a ragged one, several (68 x 132: six blocks, two of them 4 wide), 16 of them; row strides
    larger than the channel counts with sentinels between the rows; kvol 27 and 32; (5, 7): the first-generation entry alone"""
    rng = np.random.default_rng(cin + cout)
    tally = _Tally()
    for i, (recipe, fine) in enumerate(WG_FIVE):
        g = _Wgrad(recipe, fine, cin, cout, seed=800 + i + cin, wide=cin % 4 == 0)
        for kvol in (27, 32):
            num = np.minimum(rng.integers(0, 151, kvol) * (rng.random(kvol) < 0.8), g.cap)
            num[kvol // 2] = min(130, g.cap)
            _wgrad_run(tally, g, num, 160, rng, '%d->%d kvol=%d' % (cin, cout, kvol))
    tally.finish()


def test_filter_gradient_refusals_launch_nothing():
    """the output-stationary filter gradient refuses channel counts and strides that are no multiple of 4 and operands that
    are not 16-byte aligned; nothing is written"""
    L, lib = _lib()
    ws = _nan_bytes(1 << 20)
    dw = torch.full((27, 16, 32), SENTINEL, device=DEV)
    x, dy = torch.zeros(90 * 20 + 4, device=DEV), torch.zeros(70 * 36 + 4, device=DEV)
    pairs = torch.zeros((27, 2, 8), dtype=torch.int32, device=DEV)
    num = torch.full((27,), 8, dtype=torch.int32, device=DEV)

    def call(entry, x=x, ldx=16, dy=dy, lddy=32, cin=16, cout=32, x_side=0):
        return getattr(lib, entry)(L.ptr(x), ldx, L.ptr(dy), lddy, L.ptr(pairs), 8, 27 * 8, x_side, L.ptr(num), 27, cin, cout,
                                   L.ptr(dw), L.ptr(ws), L.stream_ptr())

    for entry in WG_ENTRIES[:2]:
        assert call(entry, cin=6) == L.SST_ERR_UNSUPPORTED
        assert call(entry, cout=30) == L.SST_ERR_UNSUPPORTED
        assert call(entry, ldx=18) == L.SST_ERR_UNSUPPORTED
        assert call(entry, lddy=34) == L.SST_ERR_UNSUPPORTED
        assert call(entry, x=x[1:]) == L.SST_ERR_UNSUPPORTED
        assert call(entry, dy=dy[1:]) == L.SST_ERR_UNSUPPORTED
        assert call(entry, x_side=2) == L.SST_ERR_ARG
        assert call(entry, ldx=12) == L.SST_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((ws == 0xFF).all())
