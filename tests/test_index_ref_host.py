"""CPU: the references and input builders of tests/index_ref.py, which the GPU edge tests of the integer front end
(tests/test_gpu_index_edges.py) rest on.

Three things are shown here, all without a GPU:
  1. the references are right: each against a brute-force definition at small sizes (unique against torch.unique, the
     voxel quotient against exact rational arithmetic);
  2. the inputs reach the edges they are meant to reach (asserted from the reference alone);
  3. the inputs discriminate: for every plausible kernel error a mutated reference gives a different answer on at least
     one of the inputs the GPU test runs.  The mutants live here only - nothing is mutated on the GPU.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import index_ref as R
from conftest import DROP_TEST, DROP_TRAIN, load_golden
from oracle import sst_oracle

TABLES = {'train': DROP_TRAIN, 'test': DROP_TEST, 'one': R.DROP_ONE, 'eight': R.DROP_EIGHT, 'overlap': R.DROP_OVERLAP,
          'gap': R.DROP_GAP}
VOXEL_CASES = ['sst', 'fsd', 'fsdv2']


# ------------------------------------------------------------------------------------------------------------------
# 1. the references are right
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 7, 8, 9, 65, 300])
def test_scan_ref_equals_the_running_sum_loop(n):
    x = R.scan_values(n, n)
    out, total = R.scan_ref(x)
    run = 0
    for i in range(n):
        assert out[i] == run
        run += int(x[i])
        assert -2 ** 31 <= run < 2 ** 31
    assert total == run
    if n > 8:
        assert np.abs(x.astype(np.int64)).max() > 2 ** 28 and (x < 0).any() and (x > 0).any()    # signed and large


@pytest.mark.parametrize('bits', [1, 8, 33, 64])
@pytest.mark.parametrize('n', [1, 2, 65, 200])
def test_sort_ref_equals_counting_ranks(n, bits):
    keys = R.full_width_keys(n, bits, n + bits)
    sk, perm = R.sort_ref(keys)
    u = [int(k) & (2 ** 64 - 1) for k in keys]
    for i in range(n):          # O(n^2): the place of row i = rows with a smaller key + equal keys in front of it
        place = sum(1 for j in range(n) if u[j] < u[i] or (u[j] == u[i] and j < i))
        assert perm[place] == i and sk[place] == keys[i]


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('ncols', [1, 2, 4, 8])
@pytest.mark.parametrize('kind', ['equal', 'distinct', 'random'])
def test_unique_ref_equals_torch_unique(kind, ncols, mode):
    n = 257
    rows = R.unique_rows_input(n, ncols, kind, 5 * ncols + mode, mode)
    ref = R.unique_ref(rows, mode)
    clean = torch.from_numpy(R._mask_invalid(rows, mode))
    # the batched form sample by sample == one lexicographic unique of the masked rows (column 0 leads the order)
    uniq, inv, cnt = torch.unique(clean, dim=0, return_inverse=True, return_counts=True)
    np.testing.assert_array_equal(ref['rows'], uniq.numpy())
    np.testing.assert_array_equal(ref['inverse'], inv.numpy())
    np.testing.assert_array_equal(ref['counts'], cnt.numpy())
    m = uniq.size(0)
    assert m == (1 if kind == 'equal' else m) and (kind != 'distinct' or mode != 0 or m == n)
    # perm: brute force - groups ascending, row indices ascending inside a group
    want = [i for g in range(m) for i in range(n) if ref['inverse'][i] == g]
    np.testing.assert_array_equal(ref['perm'], want)
    assert ref['offsets'][0] == 0 and ref['offsets'][m] == n
    if mode and kind == 'random' and ncols > (1 if mode == 2 else 0):
        assert (uniq < 0).any(), 'the input must contain invalid rows'


def _packed_unique(rows, mins, extents, mode):
    """the kernels' packed key (include/sst_amd.h: key = 1 + sum (c_j - mins[j]) * stride_j, last column fastest; 64-bit
    wrap-around; mode 1: invalid rows take key 0; mode 2: columns 1.. of an invalid row become -1) -> inverse"""
    rows = np.asarray(rows, dtype=np.int64)
    n, k = rows.shape
    strides, total = [0] * k, 1
    for j in range(k - 1, -1, -1):
        strides[j] = total
        total *= int(extents[j])
    keys = []
    for r in rows.tolist():
        j0 = 1 if mode == 2 else 0
        neg = any(c < 0 for c in r[j0:]) if mode else False
        key = 1
        for j, c in enumerate(r):
            if mode == 2 and neg and j >= 1:
                c = -1
            key += ((c - int(mins[j])) % 2 ** 64) * strides[j]
        key %= 2 ** 64
        if mode == 1 and neg:
            key = 0
        keys.append(key)
    order = {key: g for g, key in enumerate(sorted(set(keys)))}
    return np.asarray([order[key] for key in keys], dtype=np.int64), total


@pytest.mark.parametrize('total', sorted(R.keyspace_boxes()))
def test_packed_key_orders_rows_lexicographically_in_every_key_space(total):
    mins, extents = R.keyspace_boxes()[total]
    rows = R.keyspace_rows(129, mins, extents, 3)
    inv, tot = _packed_unique(rows, mins, extents, 0)
    assert tot == total
    ref = R.unique_ref(rows, 0)
    np.testing.assert_array_equal(inv, ref['inverse'])
    lo = [int(v) for v in mins]
    hi = [int(a) + int(b) - 1 for a, b in zip(mins, extents)]
    assert ref['rows'][0].tolist() == lo and ref['rows'][-1].tolist() == hi       # keys 1 and `total` are present
    assert ref['counts'][0] > 1 and ref['counts'][-1] > 1


@pytest.mark.parametrize('n', [1, 2, 64, 131])
def test_ingroup_rank_equals_the_counting_loop(n):
    rng = np.random.default_rng(n)
    ids = rng.integers(0, 5, size=n) * (1 << 60)
    got = sst_oracle.ingroup_rank(ids)
    for i in range(n):
        assert got[i] == sum(1 for j in range(i) if ids[j] == ids[i])


def _window_coors_loop(coors, sparse_shape, window_shape, do_shift, half=lambda w: w // 2):
    """get_window_coors voxel by voxel (mmdet3d/ops/sst/sst_ops.py:266-314)"""
    sx, sy, sz = sparse_shape
    wx, wy, wz = window_shape if len(window_shape) == 3 else (window_shape[0], window_shape[1], sz)
    nwx, nwy, nwz = -(-sx // wx) + 1, -(-sy // wy) + 1, -(-sz // wz) + 1
    shx, shy, shz = (half(wx), half(wy), half(wz)) if do_shift else (wx, wy, wz)
    if sz == wz:
        shz = 0
    win, ciw = [], []
    for b, z, y, x in np.asarray(coors).tolist():
        xs, ys, zs = x + shx, y + shy, z + shz
        win.append(b * nwx * nwy * nwz + (xs // wx) * nwy * nwz + (ys // wy) * nwz + zs // wz)
        ciw.append([zs % wz, ys % wy, xs % wx])
    return np.asarray(win, dtype=np.int64), np.asarray(ciw, dtype=np.int64)


@pytest.mark.parametrize('window_shape,sparse_shape', R.WINDOW_CASES)
def test_window_coors_oracle_equals_the_loop_and_the_corners_are_there(window_shape, sparse_shape):
    coors = R.window_corner_voxels(sparse_shape, window_shape, 3)
    assert set(coors[:, 0]) == {0, 2}
    w3 = window_shape if len(window_shape) == 3 else (window_shape[0], window_shape[1], sparse_shape[2])
    for col, s, w in ((3, sparse_shape[0], w3[0]), (2, sparse_shape[1], w3[1]), (1, sparse_shape[2], w3[2])):
        want = {min(max(v, 0), s - 1) for v in (0, w // 2 - 1, w // 2, w - 1, w, s - 1)}
        assert set(coors[:, col]) == want
    assert len(coors) == 2 * np.prod([len(set(coors[:, c])) for c in (1, 2, 3)])    # the full cross product
    for shift in (False, True):
        win, ciw = sst_oracle.window_coors(coors, sparse_shape, window_shape, shift)
        lw, lc = _window_coors_loop(coors, sparse_shape, window_shape, shift)
        np.testing.assert_array_equal(win, lw)
        np.testing.assert_array_equal(ciw, lc)
        assert win.max() < 2 ** 31


def _rb_loop(win0, win1, drop_info, hi_le=False, lo_gt=False, recompute_level0=False):
    """drop_voxel + get_flat2win_inds + the window CSR, window by window in plain Python
    (sst_input_layer_v2.py:128-226, sst_ops.py:26-64).  The keyword arguments switch on the mutations."""
    levels = R.levels_of(drop_info)

    def classify(c):
        lv, cap = -1, 0
        for l, (cp, lo, hi) in enumerate(levels):
            if (c > lo if lo_gt else c >= lo) and (c <= hi if hi_le else c < hi):
                lv, cap = l, cp
        return lv, cap

    def single(alive, win):
        groups = {}
        for i in alive:
            groups.setdefault(int(win[i]), []).append(i)
        keep, level = [], {}
        for members in groups.values():
            lv, cap = classify(len(members))
            keep += members[:cap]
            for i in members:
                level[i] = lv
        return sorted(keep), level

    m = len(win0)
    keep0, level0 = single(range(m), win0)
    keep, level1 = single(keep0, win1)
    if recompute_level0:
        _, level0 = single(keep, win0)
    out = dict(keep_idx=np.asarray(keep, dtype=np.int64))
    new = {i: k for k, i in enumerate(keep)}
    for s, (win, level) in enumerate(((win0, level0), (win1, level1))):
        groups = {}
        for i in keep:
            groups.setdefault(int(win[i]), []).append(i)
        ids = sorted(groups)
        seen = {}
        f2w, inner = {}, {}
        tok, winoff, winlevel = [], [0], []
        for w in ids:
            lv = level[groups[w][0]]
            cw = seen.get(lv, 0)
            seen[lv] = cw + 1
            cap = levels[lv][0] if lv >= 0 else 0
            for r, i in enumerate(groups[w]):
                inner[i] = r
                f2w[i] = cw * cap + r
                tok.append(new[i])
            winoff.append(len(tok))
            winlevel.append(lv)
        out[f'level{s}'] = np.asarray([level[i] for i in keep], dtype=np.int64)
        out[f'inner{s}'] = np.asarray([inner[i] for i in keep], dtype=np.int64)
        out[f'flat2win{s}'] = np.asarray([f2w[i] for i in keep], dtype=np.int64)
        out[f'tok{s}'] = np.asarray(tok, dtype=np.int64)
        out[f'winoff{s}'] = np.asarray(winoff, dtype=np.int64)
        out[f'winlevel{s}'] = np.asarray(winlevel, dtype=np.int64)
    return out


_RB_KEYS = ['keep_idx'] + [f'{k}{s}' for s in range(2) for k in ('level', 'inner', 'flat2win', 'tok', 'winoff', 'winlevel')]


def _rb_same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in _RB_KEYS)


_SCENES = {}


def _scene(table, n_win0=256, win_bits=13):
    key = (table, n_win0, win_bits)
    if key not in _SCENES:
        win0, win1, pops = R.rb_scene(TABLES[table], n_win0, win_bits, seed=n_win0 + win_bits)
        _SCENES[key] = (win0, win1, pops, R.region_ref(win0, win1, TABLES[table]))
    return _SCENES[key]


@pytest.mark.parametrize('table', sorted(TABLES))
def test_region_ref_equals_the_window_by_window_loop(table):
    win0, win1, _, ref = _scene(table)
    loop = _rb_loop(win0, win1, TABLES[table])
    for k in _RB_KEYS:
        np.testing.assert_array_equal(ref[k], loop[k], err_msg=k)
    keep = np.zeros(len(win0), dtype=bool)
    keep[loop['keep_idx']] = True
    np.testing.assert_array_equal(ref['keep'], keep)
    np.testing.assert_array_equal(ref['newidx'][keep], np.arange(keep.sum()))
    for s in range(2):
        assert ref[f'n_windows{s}'] == len(loop[f'winoff{s}']) - 1
        assert ref[f'max_tokens{s}'] == np.diff(loop[f'winoff{s}']).max()
        np.testing.assert_array_equal(ref[f'level{s}_all'][keep], loop[f'level{s}'])


@pytest.mark.parametrize('n', [1, 2, 17, 40])
def test_window_order_ref_equals_counting_ranks(n):
    sizes = R.window_order_sizes(n, 5, 'random', n)
    order = R.window_order_ref(sizes)
    for i in range(n):
        place = sum(1 for j in range(n) if sizes[j] < sizes[i] or (sizes[j] == sizes[i] and j < i))
        assert order[place] == i


def _round_to_f32(x):
    """exact rational -> nearest float32, ties to even, gradual underflow, overflow to inf"""
    if x == 0:
        return 0.0
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()        # 2^(e-1) < x < 2^(e+1)
    if Fraction(2) ** e > x:
        e -= 1                                                       # now 2^e <= x < 2^(e+1)
    q = max(e - 23, -149)                                            # the spacing of float32 at x is 2^q
    scaled = x / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rest = scaled - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    val = Fraction(n) * Fraction(2) ** q
    if val >= Fraction(2) ** 128:
        return sign * float('inf')
    return sign * float(val)


def test_round_to_f32_on_known_values():
    assert _round_to_f32(Fraction(1, 3)) == float(np.float32(1) / np.float32(3))
    assert _round_to_f32(Fraction(2 ** 24 + 1)) == 2.0 ** 24                       # tie -> even
    assert _round_to_f32(Fraction(2 ** 24 + 3)) == 2.0 ** 24 + 4
    assert _round_to_f32(Fraction(1, 2 ** 150)) == 0.0 and _round_to_f32(Fraction(3, 2 ** 150)) == 2.0 ** -148
    assert _round_to_f32(Fraction(2) ** 128) == float('inf') and _round_to_f32(-Fraction(10) ** 39) == -float('inf')


def _voxel_case(case):
    g = load_golden('voxelize.npz')
    return g[f'{case}::voxel_size'].tolist(), g[f'{case}::range'].tolist()


@pytest.mark.parametrize('case', VOXEL_CASES)
def test_voxel_quotient_is_the_correctly_rounded_quotient_on_the_whole_boundary_set(case):
    vs, rng = _voxel_case(case)
    pts = R.voxel_boundary_points(vs, rng)
    for a in range(3):
        lo, v = np.float32(rng[a]), np.float32(vs[a])
        col = np.unique(pts[:, a][np.isfinite(pts[:, a])])
        q = R.voxel_quotient(col, lo, v)
        for p, got in zip(col.tolist(), q.tolist()):
            d = _round_to_f32(Fraction(p) - Fraction(float(lo)))             # fp32 subtract: one rounding
            want = _round_to_f32(Fraction(d) / Fraction(float(v))) if np.isfinite(d) else d   # fp32 divide: one more
            assert got == want, (case, a, p)


@pytest.mark.parametrize('case', VOXEL_CASES)
def test_voxel_ref_equals_the_oracle_on_finite_points_and_states_the_rest(case):
    from oracle import voxel_oracle
    vs, rng = _voxel_case(case)
    pts = R.voxel_boundary_points(vs, rng)
    grid = voxel_oracle.dynamic_voxelize_grid(vs, rng)
    ref = R.voxel_ref(pts, vs, rng)
    fin = np.isfinite(pts).all(1) & (np.abs(pts) < 1e30).all(1)
    np.testing.assert_array_equal(ref[fin], voxel_oracle.dynamic_voxelize(pts[fin], vs, rng))
    for a in range(3):
        c = ref[:, 2 - a]
        assert c.min() >= 0 and c.max() <= grid[a] - 1
        assert (c[np.isnan(pts[:, a])] == 0).all() and np.isnan(pts[:, a]).any()
        assert (c[pts[:, a] == np.inf] == grid[a] - 1).all() and (pts[:, a] == np.inf).any()
        assert (c[pts[:, a] == -np.inf] == 0).all() and (pts[:, a] == -np.inf).any()
        assert (c[pts[:, a] == np.float32(3e38)] == grid[a] - 1).all() and (c[pts[:, a] == np.float32(-3e38)] == 0).all()


# ------------------------------------------------------------------------------------------------------------------
# 2. the inputs reach the edges
# ------------------------------------------------------------------------------------------------------------------
def test_edge_lengths_and_case_lists():
    assert R.edge_lengths(8, 64) == [7, 8, 9, 63, 64, 65]
    for u in (8, 64, 512, 2048, 524288):
        assert {u - 1, u, u + 1} <= set(R.SCAN_LENGTHS)
    assert {0, 1} <= set(R.SCAN_LENGTHS)
    assert sorted({(b + 7) // 8 for b in R.SORT_KEY_BITS}) == list(range(1, 9))
    assert {8 * k for k in range(1, 9)} | {8 * k - 7 for k in range(1, 9)} == set(R.SORT_KEY_BITS)
    assert -(-R.SORT_LARGE_N // 2048) * 256 > 524288          # the histogram scan's spine takes a second round
    assert set(R.UNIQUE_LENGTHS) == {63, 64, 65, 2047, 2048, 2049}


@pytest.mark.parametrize('bits', R.SORT_KEY_BITS)
def test_full_width_keys_show_every_digit_value_in_every_pass_and_repeat(bits):
    for b, n, seed in R.sort_cases():
        if b != bits:
            continue
        keys = R.full_width_keys(n, bits, seed).view(np.uint64)
        if bits < 64:
            assert int(keys.max()) < 2 ** bits
        if n >= 8:
            assert np.unique(keys).size < n, 'duplicates make stability observable'
        if n >= 1024:
            for p in range((bits + 7) // 8):
                width = min(8, bits - 8 * p)
                digits = (keys >> np.uint64(8 * p)) & np.uint64(0xFF)
                assert np.unique(digits).size == 2 ** width, (n, p)
            if bits == 64:
                frac = float((keys >> np.uint64(63)).mean())
                assert 0.4 < frac < 0.6, 'about half of the 64-bit keys carry the top bit'


@pytest.mark.parametrize('table', sorted(TABLES))
@pytest.mark.parametrize('n_win0', R.RB_WINDOW_COUNTS)
def test_scene_holds_every_edge_population_in_both_shifts(table, n_win0):
    drop = TABLES[table]
    win0, win1, pops, ref = _scene(table, n_win0)
    bounds = {b for lv in drop.values() for b in lv['drop_range'] if 1 < b < 10000} | {lv['max_tokens'] for lv in drop.values()}
    if table in ('train', 'test', 'gap'):
        assert {30, 60, 100} <= bounds
    want = {1, 99, 100, 101} | {b + d for b in bounds for d in (-1, 0, 1)}
    assert want == set(pops)
    assert np.unique(win0).size == n_win0
    pop0 = np.bincount(np.unique(win0, return_inverse=True)[1].reshape(-1))
    assert want <= set(pop0.tolist())
    k0 = ref['keep0']
    pop1 = np.bincount(np.unique(win1[k0], return_inverse=True)[1].reshape(-1))
    assert want <= set(pop1.tolist()), sorted(want - set(pop1.tolist()))
    # the voxels of a window are interleaved across the array, not stored in one run
    big = np.nonzero(win0 == np.unique(win0)[np.argmax(pop0)])[0]
    assert (np.diff(big) > 1).any()
    # a shift-0 window that changes its level class when the shift-1 drop thins it (level0 is not recomputed)
    after = {w: c for w, c in zip(*np.unique(ref['win0'], return_counts=True))}
    lv_of = dict(zip(ref['win0'].tolist(), ref['level0'].tolist()))

    def classify(c):
        lv = -1
        for l, (cap, lo, hi) in enumerate(R.levels_of(drop)):
            if lo <= c < hi:
                lv = l
        return lv
    if table != 'one':      # one level: there is no other class to fall into
        assert any(classify(c) != lv_of[w] for w, c in after.items()), 'no level0-quirk window'
    if table == 'gap':
        assert (ref['level0_all'] == -1).any() and (ref['level1_all'][k0] == -1).any(), 'no window in the level -1 gap'
        assert not ref['keep'][ref['level0_all'] == -1].any()
    assert ref['keep'].sum() < len(win0), 'the scene must lose voxels to the drop'


@pytest.mark.parametrize('win_bits', R.RB_WIN_BITS)
def test_scene_ids_use_the_top_bit(win_bits):
    win0, win1, _, ref = _scene('train', 100, win_bits)
    for w in (win0, win1):
        assert w.min() == 0 and w.max() == 2 ** win_bits - 1
        assert 0.3 < float((np.unique(w) >> (win_bits - 1)).mean()) < 0.7
    assert ref['n_windows0'] > 50


@pytest.mark.parametrize('table', ['train', 'test', 'gap'])
def test_twin_realises_the_populations_at_shift_0(table):
    drop = TABLES[table]
    vox, pops = R.twin_voxels(drop)
    if table == 'gap':     # windows whose population matches no level: dropped whole, in both shifts' drop tests
        w0, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, False)
        w1, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, True)
        ref = R.region_ref(w0, w1, drop)
        gap0 = ref['level0_all'] == -1
        assert gap0.any() and not ref['keep'][gap0].any()
        assert {100, 101} <= set(np.unique(w0[gap0], return_counts=True)[1].tolist())     # `hi` itself and hi + 1
        assert (ref['level1_all'][ref['keep0']] == -1).any(), 'no shift-1 window of the twin in the gap'
        assert 0 < ref['keep'].sum() < len(vox)
    assert pops == [p for p in R.edge_populations(drop) if p <= 144] and (table != 'test' or 144 in pops)
    assert len(np.unique(vox, axis=0)) == len(vox) and vox[:, 2:].max() <= 467 and vox.min() == 0
    assert np.array_equal(vox, np.unique(vox, axis=0))                 # sorted (b, z, y, x)
    for b in range(2):
        w0, _ = sst_oracle.window_coors(vox[vox[:, 0] == b], R.TWIN_SPARSE, R.TWIN_WINDOW, False)
        assert sorted(np.unique(w0, return_counts=True)[1].tolist()) == sorted(pops + [99] * 4)
        w1, _ = sst_oracle.window_coors(vox[vox[:, 0] == b], R.TWIN_SPARSE, R.TWIN_WINDOW, True)
        assert 100 in np.unique(w1, return_counts=True)[1]
    from conftest import PC_RANGE, VOXEL_SIZE
    for b, pts in enumerate(R.twin_points(vox, VOXEL_SIZE, PC_RANGE)):
        c = R.voxel_ref(pts, VOXEL_SIZE, PC_RANGE).astype(np.int64)
        got = np.unique(c, axis=0)
        assert got[0].tolist() == [0, 0, 0]                            # the voxel DynamicVFE discards
        np.testing.assert_array_equal(got[1:], vox[vox[:, 0] == b][:, 1:])


@pytest.mark.parametrize('case', VOXEL_CASES)
def test_boundary_set_has_points_on_both_sides_of_every_face(case):
    from oracle import voxel_oracle
    vs, rng = _voxel_case(case)
    pts = R.voxel_boundary_points(vs, rng)
    ref = R.voxel_ref(pts, vs, rng)
    grid = voxel_oracle.dynamic_voxelize_grid(vs, rng)
    for a in range(3):
        lo, v, g = np.float32(rng[a]), np.float32(vs[a]), int(grid[a])
        face = (np.float64(lo) + np.arange(g + 1) * np.float64(v)).astype(np.float32)
        col, c = pts[:, a], ref[:, 2 - a]
        for k in range(1, g):
            near = np.abs(col - face[k]) <= 4 * np.spacing(np.abs(face[k])) + 3 * np.spacing(np.float32(k)) * v
            assert {k - 1, k} <= set(c[near].tolist()), (case, a, k)
        assert (col < lo).any() and (col > np.float32(rng[a + 3])).any()      # outside both ends
        for s in R.VOXEL_SPECIALS[:-1]:
            assert ((col == s) & (np.signbit(col) == np.signbit(s))).any()


# ------------------------------------------------------------------------------------------------------------------
# 3. the inputs discriminate
# ------------------------------------------------------------------------------------------------------------------
def _lsd(keys, bits, skip=None, unstable_unit=None):
    """LSD radix sort, 8-bit digits.  skip: a pass that is left out.  unstable_unit: equal digits of different blocks of
    that many positions come out in descending block order."""
    u = np.asarray(keys, dtype=np.int64).view(np.uint64)
    order = np.arange(u.size)
    for p in range((bits + 7) // 8):
        if p == skip:
            continue
        d = ((u[order] >> np.uint64(8 * p)) & np.uint64(0xFF)).astype(np.int64)
        if unstable_unit is None:
            step = np.argsort(d, kind='stable')
        else:
            pos = np.arange(u.size)
            step = np.lexsort((pos, -(pos // unstable_unit), d))
        order = order[step]
    return order


def _sort_inputs(bits):
    for b, n, seed in R.sort_cases():
        if b == bits:
            yield R.full_width_keys(n, bits, seed)
    for n in R.SORT_PATTERN_LENGTHS:
        for keys in R.sort_patterns(n, bits).values():
            yield keys


@pytest.mark.parametrize('bits', R.SORT_KEY_BITS)
def test_sort_inputs_kill_the_skipped_pass_and_the_unstable_sort(bits):
    inputs = list(_sort_inputs(bits))
    for keys in inputs:
        np.testing.assert_array_equal(_lsd(keys, bits), R.sort_ref(keys)[1])          # the unmutated sort is the reference
    for k in range((bits + 7) // 8):
        assert any(not np.array_equal(_lsd(keys, bits, skip=k), R.sort_ref(keys)[1]) for keys in inputs), f'pass {k} survives'
    for unit in (64, 512, 2048):
        assert any(not np.array_equal(_lsd(keys, bits, unstable_unit=unit), R.sort_ref(keys)[1]) for keys in inputs), unit


def _scan_inputs():
    for n in R.SCAN_LENGTHS:
        yield R.scan_values(n, n)
        for pos in sorted({0, n - 2, n - 1} & set(range(n))):
            yield R.scan_single_one(n, pos)


@pytest.mark.parametrize('unit', [8, 64, 2048, 524288])
def test_scan_inputs_kill_the_lost_carry(unit):
    def mutant(x):
        out = R.scan_ref(x)[0].astype(np.int64)
        if x.size > unit:                      # positions [unit, 2 unit) do not receive the sum of the first `unit` values
            out[unit:2 * unit] -= int(x[:unit].astype(np.int64).sum())
        return out

    inputs = [x for x in _scan_inputs() if unit - 1 <= x.size <= unit + 1]
    assert any(not np.array_equal(mutant(x), R.scan_ref(x)[0]) for x in inputs)
    ones = [x for x in inputs if x.size == unit + 1 and np.abs(x).sum() == 1]
    assert any(not np.array_equal(mutant(x), R.scan_ref(x)[0]) for x in ones), 'the single 1 just below the edge must show it'


@pytest.mark.parametrize('table', sorted(TABLES))
def test_scene_kills_the_drop_test_mutants(table):
    win0, win1, _, ref = _scene(table)
    drop = TABLES[table]
    assert _rb_same(_rb_loop(win0, win1, drop), ref)
    hit = {name: not _rb_same(_rb_loop(win0, win1, drop, **{name: True}), ref) for name in ('hi_le', 'lo_gt', 'recompute_level0')}
    # `<=` at the upper end is masked wherever the next level starts there (the later level wins): only a table with a hole
    # or with a range that ends inside another one can show it
    if table in ('gap', 'overlap'):
        assert hit['hi_le'], hit
    if table != 'one':
        assert hit['lo_gt'], hit
    if table in ('train', 'test', 'gap'):
        assert hit['recompute_level0'], hit


def test_twin_on_the_table_with_a_hole_kills_the_upper_bound_mutant():
    """the fused planner has its own copy of the drop test and is reached through the twin only"""
    vox, _ = R.twin_voxels(R.DROP_GAP)
    w0, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, False)
    w1, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, True)
    ref = R.region_ref(w0, w1, R.DROP_GAP)
    assert _rb_same(_rb_loop(w0, w1, R.DROP_GAP), ref)
    for name in ('hi_le', 'lo_gt'):
        assert not _rb_same(_rb_loop(w0, w1, R.DROP_GAP, **{name: True}), ref), name
    # at shift 1 alone: the window of exactly 100 survivors is kept whole by `<=`
    mut = _rb_loop(w0, w1, R.DROP_GAP, hi_le=True)
    assert len(mut['keep_idx']) > len(ref['keep_idx'])


def test_odd_windows_kill_the_rounded_up_half_shift():
    killed = []
    for window_shape, sparse_shape in R.WINDOW_CASES:
        coors = R.window_corner_voxels(sparse_shape, window_shape, 3)
        ref = sst_oracle.window_coors(coors, sparse_shape, window_shape, True)
        mut = _window_coors_loop(coors, sparse_shape, window_shape, True, half=lambda w: (w + 1) // 2)
        wz = window_shape[2] if len(window_shape) == 3 else sparse_shape[2]
        odd = bool(window_shape[0] % 2 or window_shape[1] % 2 or (wz % 2 and wz != sparse_shape[2]))
        differs = not (np.array_equal(ref[0], mut[0]) and np.array_equal(ref[1], mut[1]))
        assert differs == odd
        killed.append(differs)
    assert sum(killed) >= 2


@pytest.mark.parametrize('case', VOXEL_CASES)
def test_boundary_set_kills_the_reciprocal_multiply_and_tells_truncation_apart(case):
    from oracle import voxel_oracle
    vs, rng = _voxel_case(case)
    pts = R.voxel_boundary_points(vs, rng)
    grid = voxel_oracle.dynamic_voxelize_grid(vs, rng)
    ref = R.voxel_ref(pts, vs, rng)
    diff_recip = 0
    for a in range(3):
        lo, v, g = np.float32(rng[a]), np.float32(vs[a]), int(grid[a])
        with np.errstate(all='ignore'):
            q_recip = ((pts[:, a] - lo) * (np.float32(1) / v)).astype(np.float32)
        diff_recip += int((R.voxel_coord_from_quotient(q_recip, g) != ref[:, 2 - a]).sum())
        # truncation towards zero instead of floor: differs from floor exactly for -1 < q < 0, where floor gives -1 and the
        # clamp then gives 0 as well - after the clamp the two are the same function, no input can tell them apart.  What
        # the set does guarantee is that such quotients are in it, so a kernel that truncated AND tagged instead of clamped
        # (the upstream behaviour: -1 for points below the range) would show.
        q = R.voxel_quotient(pts[:, a], lo, v)
        assert ((q > -1) & (q < 0)).any()
        with np.errstate(all='ignore'):
            trunc = np.where(np.isfinite(q), np.trunc(q), q)
        np.testing.assert_array_equal(R.voxel_coord_from_quotient(trunc.astype(np.float32), g), ref[:, 2 - a])
    # 0.25 is a power of two: its reciprocal is exact and the multiply IS the divide (fsd, x and y)
    assert diff_recip > 0, 'multiply-by-reciprocal survives'


def test_window_order_inputs_kill_the_order_that_is_unstable_across_the_slices():
    def mutant(sizes):
        n = len(sizes)
        per = -(-n // 16)
        i = np.arange(n)
        return np.lexsort((i, -(i // per), sizes))

    for n in R.WINDOW_ORDER_N:
        if n < 16:
            continue
        for cap in R.WINDOW_ORDER_CAPS:
            sizes = R.window_order_sizes(n, cap, 'equal', n + cap)
            assert not np.array_equal(mutant(sizes), R.window_order_ref(sizes)), (n, cap)
    sizes = R.window_order_sizes(1040, 511, 'random', 3)
    assert np.unique(sizes).size < sizes.size and not np.array_equal(mutant(sizes), R.window_order_ref(sizes))


@pytest.mark.parametrize('ncols', [3, 4, 8])     # two columns: the one coordinate column is the negative one itself
def test_mode2_inputs_kill_bounds_that_are_not_lowered_to_minus_one(ncols):
    rows = R.unique_rows_input(2049, ncols, 'random', ncols, mode=2)
    ref = R.unique_ref(rows, 2)
    raw_lo = rows.min(0)
    raw_ext = rows.max(0) - raw_lo + 1
    assert (rows[:, 1:] < 0).any() and (raw_lo[1:] >= 0).any()
    low_lo = np.concatenate([raw_lo[:1], np.minimum(raw_lo[1:], -1)])
    low_ext = rows.max(0) - low_lo + 1
    np.testing.assert_array_equal(_packed_unique(rows, low_lo, low_ext, 2)[0], ref['inverse'])
    assert not np.array_equal(_packed_unique(rows, raw_lo, raw_ext, 2)[0], ref['inverse'])
    lo, ext = R.unique_bounds(rows, 2)
    np.testing.assert_array_equal(_packed_unique(rows, lo, ext, 2)[0], ref['inverse'])
