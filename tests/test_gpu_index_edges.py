"""GPU: the integer front end (csrc/sort_scan.hip, window.hip, frame_plan.hip, voxelize.hip) at every tile, digit and
drop-level edge, bit-exact against the plain references of tests/index_ref.py.  The inputs are the ones whose reach and
discriminating power tests/test_index_ref_host.py proves on the CPU; nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import index_ref as R
from conftest import DROP_TEST, DROP_TRAIN, PC_RANGE, VOXEL_SIZE, load_golden
from oracle import sst_oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

TABLES = {'train': DROP_TRAIN, 'test': DROP_TEST, 'one': R.DROP_ONE, 'eight': R.DROP_EIGHT, 'overlap': R.DROP_OVERLAP,
          'gap': R.DROP_GAP}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------
# scan
# ------------------------------------------------------------------------------------------------------------------
def _scan_inputs(n):
    yield R.scan_values(n, n)
    for pos in sorted({0, n - 2, n - 1} & set(range(n))):
        yield R.scan_single_one(n, pos)


@pytest.mark.parametrize('n', R.SCAN_LENGTHS)
def test_scan_signed_values_and_single_ones(n):
    from sst_amd import kernels as K
    for x in _scan_inputs(n):
        want, total = R.scan_ref(x)
        out, tot = K.exclusive_scan_i32(_dev(x))
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert int(tot.item()) == total


@pytest.mark.parametrize('n', R.SCAN_LENGTHS)
def test_scan_in_place_and_without_a_total(n):
    """the C entry as the sort uses it: out == in, d_total == NULL"""
    from sst_amd import _lib
    lib = _lib.load()
    for x in _scan_inputs(n):
        want, total = R.scan_ref(x)
        buf = _dev(x)
        ws = _lib.workspace(lib.sst_scan_workspace_bytes(n), buf.device)
        rc = lib.sst_exclusive_scan_i32(_lib.ptr(buf), _lib.ptr(buf), n, None, _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, 'sst_exclusive_scan_i32')
        np.testing.assert_array_equal(buf.cpu().numpy(), want)
        # in place WITH a total
        buf = _dev(x)
        tot = torch.full((1,), -77, dtype=torch.int32, device=DEV)
        rc = lib.sst_exclusive_scan_i32(_lib.ptr(buf), _lib.ptr(buf), n, _lib.ptr(tot), _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, 'sst_exclusive_scan_i32')
        np.testing.assert_array_equal(buf.cpu().numpy(), want)
        assert int(tot.item()) == total


# ------------------------------------------------------------------------------------------------------------------
# sort
# ------------------------------------------------------------------------------------------------------------------
def _check_sort(keys, bits):
    from sst_amd import kernels as K
    sk, perm = K.sort_pairs_u64(_dev(keys), bits)
    want_keys, want_perm = R.sort_ref(keys)
    np.testing.assert_array_equal(sk.cpu().numpy(), want_keys)
    np.testing.assert_array_equal(_np(perm), want_perm)


@pytest.mark.parametrize('bits', R.SORT_KEY_BITS)
def test_sort_full_width_keys_every_pass_count(bits):
    for b, n, seed in R.sort_cases():
        if b == bits:
            _check_sort(R.full_width_keys(n, bits, seed), bits)


@pytest.mark.parametrize('bits', R.SORT_KEY_BITS)
def test_sort_fixed_patterns(bits):
    for n in R.SORT_PATTERN_LENGTHS:
        for name, keys in R.sort_patterns(n, bits).items():
            _check_sort(keys, bits)


def test_sort_whose_histogram_scan_needs_a_second_spine_round():
    """2049 sort tiles: 256 x 2049 digit counters = 257 scan tiles, one more than the spine handles in a round"""
    n = R.SORT_LARGE_N
    keys = np.random.default_rng(5).integers(0, 256, size=n, dtype=np.int64)
    _check_sort(keys, 8)


# ------------------------------------------------------------------------------------------------------------------
# unique rows
# ------------------------------------------------------------------------------------------------------------------
def _check_plan(plan, ref, n, dtype, K):
    m = len(ref['counts'])
    assert plan.m == m and int(plan.num.item()) == m
    np.testing.assert_array_equal(_np(plan.inverse), ref['inverse'])
    np.testing.assert_array_equal(_np(plan.counts()), ref['counts'])
    np.testing.assert_array_equal(_np(plan.perm), ref['perm'])
    off = _np(plan.offsets)[:m + 1]
    np.testing.assert_array_equal(off, ref['offsets'])
    assert off[m] == n
    rows = K.unpack_unique_rows(plan, dtype)
    assert rows.dtype == dtype
    np.testing.assert_array_equal(_np(rows), ref['rows'])


@pytest.mark.parametrize('ncols', range(1, 9))
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_unique_rows_modes_widths_lengths(mode, dtype, ncols):
    from sst_amd import kernels as K
    for n in R.UNIQUE_LENGTHS:
        for kind in ('equal', 'distinct', 'random'):
            rows = R.unique_rows_input(n, ncols, kind, 100 * n + ncols, mode)
            ref = R.unique_ref(rows, mode)
            if kind == 'equal':
                assert len(ref['counts']) == 1
            if kind == 'distinct' and mode == 0:
                assert len(ref['counts']) == n
            coors = _dev(rows, dtype)
            _check_plan(K.unique_rows(coors, invalid_if_negative=mode), ref, n, dtype, K)          # automatic bounds
            mins, extents = R.unique_bounds(rows, mode)
            _check_plan(K.unique_rows(coors, mins, extents, invalid_if_negative=mode), ref, n, dtype, K)
            if kind == 'random':
                late = K.unique_rows(coors, mins, extents, invalid_if_negative=mode, defer_count=True)
                assert late.m is None and int(late.num.item()) == len(ref['counts'])
                np.testing.assert_array_equal(_np(late.inverse), ref['inverse'])


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_unique_rows_of_a_column_sliced_view(mode, dtype):
    from sst_amd import kernels as K
    n, ncols = 2049, 4
    rows = R.unique_rows_input(n, ncols, 'random', 9, mode)
    wide = np.full((n, ncols + 3), -5, dtype=np.int64)
    wide[:, 1:1 + ncols] = rows
    view = _dev(wide, dtype)[:, 1:1 + ncols]
    assert view.stride(0) == ncols + 3 and view.stride(1) == 1 and not view.is_contiguous()
    _check_plan(K.unique_rows(view, invalid_if_negative=mode), R.unique_ref(rows, mode), n, dtype, K)


def test_unique_rows_rejects_a_transposed_view():
    from sst_amd import kernels as K
    rows = R.unique_rows_input(65, 3, 'random', 1, 0)
    t = _dev(rows.T.copy(), torch.int32).t()
    assert t.shape == (65, 3) and t.stride(1) != 1
    with pytest.raises(RuntimeError, match='inner stride'):
        K.unique_rows(t)
    _check_plan(K.unique_rows(t.contiguous()), R.unique_ref(rows, 0), 65, torch.int32, K)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('total', sorted(R.keyspace_boxes()))
def test_unique_rows_key_space_on_a_pass_boundary(total, dtype):
    """packed keys 1 .. total with `total` next to a digit boundary, the smallest and the largest key present"""
    from sst_amd import kernels as K
    mins, extents = R.keyspace_boxes()[total]
    assert int(np.prod([int(e) for e in extents], dtype=object)) == total
    for n in (65, 2049):
        rows = R.keyspace_rows(n, mins, extents, n)
        ref = R.unique_ref(rows, 0)
        assert ref['rows'][0].tolist() == mins and ref['rows'][-1].tolist() == [a + b - 1 for a, b in zip(mins, extents)]
        coors = _dev(rows, dtype)
        _check_plan(K.unique_rows(coors, mins, extents), ref, n, dtype, K)
        _check_plan(K.unique_rows(coors), ref, n, dtype, K)


def test_unique_rows_key_space_above_the_limit_raises():
    from sst_amd import _lib, kernels as K
    coors = _dev(np.zeros((5, 2), dtype=np.int64))
    with pytest.raises(_lib.SSTError, match='SST_ERR_KEYSPACE'):
        K.unique_rows(coors, [0, 0], [1 << 31, (1 << 31) + 1])
    with pytest.raises(_lib.SSTError, match='SST_ERR_KEYSPACE'):
        K.unique_rows(coors, [0, 0], [1 << 62, 2])
    assert K.unique_rows(coors, [0, 0], [1 << 31, 1 << 31]).m == 1          # exactly 2^62: allowed


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_unpack_unique_rows_window_of_groups_into_wider_rows(dtype):
    from sst_amd import kernels as K
    rows = R.unique_rows_input(2049, 3, 'random', 4, 0)
    ref = R.unique_ref(rows, 0)
    plan = K.unique_rows(_dev(rows, dtype))
    m = len(ref['counts'])
    first, count = 5, m - 9
    out = torch.full((count, 6), -7, dtype=dtype, device=DEV)
    got = K.unpack_unique_rows(plan, dtype, first=first, count=count, out_cols=6, col0=2, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = np.full((count, 6), -7, dtype=np.int64)
    want[:, 2:5] = ref['rows'][first:first + count]
    np.testing.assert_array_equal(_np(got), want)
    fresh = K.unpack_unique_rows(plan, dtype, first=first, out_cols=4, col0=1)
    assert fresh.shape == (m - first, 4)
    np.testing.assert_array_equal(_np(fresh)[:, 1:], ref['rows'][first:])


# ------------------------------------------------------------------------------------------------------------------
# in-group rank
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', R.UNIQUE_LENGTHS)
def test_ingroup_rank_one_group_singletons_wide_ids(n):
    from sst_amd import kernels as K
    rng = np.random.default_rng(n)
    big = (1 << 62) // max(n, 1)
    cases = {
        'one group': (np.full(n, 12345, dtype=np.int64), None),
        'one group at 2^62': (np.full(n, 1 << 62, dtype=np.int64), None),
        'singletons': (rng.permutation(n).astype(np.int64) * big + (1 << 62) - (n - 1) * big, None),
        'wide ids': (rng.integers(0, 7, size=n, dtype=np.int64) * ((1 << 62) // 6), None),
        'more key bits than needed': (rng.integers(0, 40, size=n, dtype=np.int64), 63),
        'odd key bits': (rng.integers(0, 300, size=n, dtype=np.int64), 17),
    }
    for name, (ids, bits) in cases.items():
        assert ids.min() >= 0 and ids.max() <= 1 << 62
        got = K.ingroup_rank(_dev(ids), bits)
        np.testing.assert_array_equal(_np(got), sst_oracle.ingroup_rank(ids), err_msg=name)
    assert cases['singletons'][0].max() == 1 << 62 and np.unique(cases['singletons'][0]).size == n


# ------------------------------------------------------------------------------------------------------------------
# window coordinates
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('window_shape,sparse_shape', R.WINDOW_CASES)
def test_window_coors_at_the_corners(window_shape, sparse_shape, dtype):
    import sst_amd
    coors = R.window_corner_voxels(sparse_shape, window_shape, 3)
    dev = _dev(coors, dtype)
    for shift in (False, True):
        win, ciw = sst_amd.get_window_coors(dev, sparse_shape, window_shape, shift)
        want_win, want_ciw = sst_oracle.window_coors(coors, sparse_shape, window_shape, shift)
        np.testing.assert_array_equal(_np(win), want_win)
        np.testing.assert_array_equal(_np(ciw), want_ciw)


# ------------------------------------------------------------------------------------------------------------------
# region batching
# ------------------------------------------------------------------------------------------------------------------
def _check_region_batching(win0, win1, win_bits, drop):
    from sst_amd import kernels as K
    ref = R.region_ref(win0, win1, drop)
    rb = K.region_batching(_dev(win0, torch.int32), _dev(win1, torch.int32), win_bits, R.levels_of(drop))
    counts = rb['counts'].cpu().tolist()
    keep = ref['keep']
    mk = int(keep.sum())
    np.testing.assert_array_equal(_np(rb['keep']), keep.astype(np.int64))
    np.testing.assert_array_equal(_np(rb['newidx']), ref['newidx'])
    assert counts[0] == mk
    for s in range(2):
        np.testing.assert_array_equal(_np(rb[f'level{s}']), ref[f'level{s}_all'], err_msg=f'level{s}')
        np.testing.assert_array_equal(_np(rb[f'inner{s}'])[keep], ref[f'inner{s}'], err_msg=f'inner{s}')
        np.testing.assert_array_equal(_np(rb[f'flat2win{s}']), ref[f'flat2win{s}_all'], err_msg=f'flat2win{s}')
        nw = ref[f'n_windows{s}']
        assert counts[1 + s] == nw
        assert counts[3 + s] == ref[f'max_tokens{s}']
        np.testing.assert_array_equal(_np(rb[f'tok{s}'])[:mk], ref[f'tok{s}'], err_msg=f'tok{s}')
        np.testing.assert_array_equal(_np(rb[f'winoff{s}'])[:nw + 1], ref[f'winoff{s}'], err_msg=f'winoff{s}')
        np.testing.assert_array_equal(_np(rb[f'winlevel{s}'])[:nw], ref[f'winlevel{s}'], err_msg=f'winlevel{s}')
    return ref


@pytest.mark.parametrize('n_win0', R.RB_WINDOW_COUNTS)
@pytest.mark.parametrize('table', sorted(TABLES))
def test_region_batching_scene_on_every_level_boundary(table, n_win0):
    win0, win1, _ = R.rb_scene(TABLES[table], n_win0, 13, seed=n_win0 + 13)
    ref = _check_region_batching(win0, win1, 13, TABLES[table])
    assert ref['keep'].sum() < len(win0)


@pytest.mark.parametrize('table', ['train', 'gap'])
@pytest.mark.parametrize('win_bits', R.RB_WIN_BITS)
def test_region_batching_ids_that_use_the_top_bit(win_bits, table):
    win0, win1, _ = R.rb_scene(TABLES[table], 100, win_bits, seed=100 + win_bits)
    assert win0.max() == 2 ** win_bits - 1 and win1.max() == 2 ** win_bits - 1
    _check_region_batching(win0, win1, win_bits, TABLES[table])


# the twin's drop tables: what the detector ships for training and for testing, and the table with a hole (a population of
# 100 and more matches no level): (tables handed to the layer, training mode, the table in force)
TWIN_TABLES = {'train': ((DROP_TRAIN, DROP_TEST), True, DROP_TRAIN), 'test': ((DROP_TRAIN, DROP_TEST), False, DROP_TEST),
               'gap': ((R.DROP_GAP, R.DROP_GAP), True, R.DROP_GAP)}


def _twin_layer(table, window_major):
    import sst_amd
    tables, train, _ = TWIN_TABLES[table]
    layer = sst_amd.SSTInputLayerV2(tables, R.TWIN_WINDOW, R.TWIN_SPARSE, shuffle_voxels=False, debug=False,
                                    mute=True, reference_outputs=False, window_major=window_major)
    layer.train(train)
    return layer


def _check_sra_plans(info, ref, tok, drop):
    cap = max(lv['max_tokens'] for lv in drop.values())
    mk = len(ref['keep_idx'])
    for s in range(2):
        plan = info[f'sra_plan_shift{s}']
        nw = ref[f'n_windows{s}']
        assert (plan.n_windows, plan.n_tokens) == (nw, mk)
        assert plan.max_tokens == min(cap, max(1, ref[f'max_tokens{s}']))
        np.testing.assert_array_equal(_np(plan.winoff)[:nw + 1], ref[f'winoff{s}'])
        np.testing.assert_array_equal(_np(plan.tok)[:mk], tok[s])


@pytest.mark.parametrize('window_major', [False, True])
@pytest.mark.parametrize('table', sorted(TWIN_TABLES))
def test_twin_through_the_input_layer_plan(table, window_major):
    drop = TWIN_TABLES[table][2]
    vox, _ = R.twin_voxels(drop)
    vox = vox[np.random.default_rng(3).permutation(len(vox))]            # the voxels of a window interleaved
    w0, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, False)
    w1, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, True)
    ref = R.region_ref(w0, w1, drop)
    # at test time a 12 x 12 window never exceeds the cap of 144: nothing is dropped there
    assert table == 'test' or 0 < len(ref['keep_idx']) < len(vox)
    assert table != 'gap' or ((ref['level0_all'] == -1).any() and (ref['level1_all'][ref['keep0']] == -1).any())
    info = _twin_layer(table, window_major).build_plan(_dev(vox, torch.int32), 2)
    if window_major:
        keep, tok0, tok1 = R.window_major(ref)
    else:
        keep, tok0, tok1 = ref['keep_idx'], ref['tok0'], ref['tok1']
    np.testing.assert_array_equal(_np(info['voxel_keep_inds']), keep)
    np.testing.assert_array_equal(_np(info['voxel_coors']), vox[keep])
    _check_sra_plans(info, ref, (tok0, tok1), drop)


@pytest.mark.parametrize('table', sorted(TWIN_TABLES))
def test_twin_through_the_fused_frame_plan(table):
    """csrc/frame_plan.hip repeats the drop test of window.hip in its own code: the same populations on every level
    boundary, and with the 'gap' table windows that match no level (dropped whole) in both partitions"""
    import sst_amd
    from sst_amd.frame_plan import FramePlanner
    drop = TWIN_TABLES[table][2]
    vox, _ = R.twin_voxels(drop)                                          # sorted (b, z, y, x): the planner's voxel table
    clouds = [_dev(p) for p in R.twin_points(vox, VOXEL_SIZE, PC_RANGE)]
    w0, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, False)
    w1, _ = sst_oracle.window_coors(vox, R.TWIN_SPARSE, R.TWIN_WINDOW, True)
    ref = R.region_ref(w0, w1, drop)
    assert table != 'gap' or ((ref['level0_all'] == -1).any() and (ref['level1_all'][ref['keep0']] == -1).any())
    keep, tok0, tok1 = R.window_major(ref)
    voxel_layer = sst_amd.Voxelization(VOXEL_SIZE, PC_RANGE, -1, (-1, -1))
    vfe = sst_amd.DynamicVFE(in_channels=3, feat_channels=[64, 128], voxel_size=VOXEL_SIZE, with_cluster_center=True,
                             with_voxel_center=True, point_cloud_range=PC_RANGE,
                             norm_cfg=dict(type='naiveSyncBN1d', eps=1e-3, momentum=0.01)).to(DEV)
    assert vfe.reference_compat, 'the twin carries one voxel per sample for the discarded first row'
    layer = _twin_layer(table, True)
    planner = FramePlanner(voxel_layer, vfe, layer)
    assert planner.supported(2)
    plan = planner.build(clouds)
    info = plan.finalize(torch.zeros(plan.n_upper, 128, device=DEV), layer)
    assert plan.num_voxels == len(vox)
    np.testing.assert_array_equal(_np(plan.vcoors)[:len(vox)], vox)
    np.testing.assert_array_equal(_np(info['voxel_keep_inds']), keep)
    np.testing.assert_array_equal(_np(info['voxel_coors']), vox[keep])
    _check_sra_plans(info, ref, (tok0, tok1), drop)


# ------------------------------------------------------------------------------------------------------------------
# window launch order
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', R.WINDOW_ORDER_CAPS)
@pytest.mark.parametrize('n', R.WINDOW_ORDER_N)
def test_window_order_at_the_slice_edges_and_the_bin_limit(n, cap, monkeypatch):
    from sst_amd import kernels as K
    monkeypatch.setattr(K, 'WINDOW_ORDER_MIN', 1)
    for kind in R.WINDOW_ORDER_KINDS:
        sizes = R.window_order_sizes(n, cap, kind, 7 * n + cap)
        winoff = _dev(np.concatenate([[0], np.cumsum(sizes)]), torch.int32)
        total = int(sizes.sum())
        plan = K.WindowPlan(torch.arange(max(total, 1), dtype=torch.int32, device=DEV), winoff, n, total, cap)
        order = plan.order
        assert order.dtype == torch.int32
        np.testing.assert_array_equal(_np(order), R.window_order_ref(sizes), err_msg=kind)


# ------------------------------------------------------------------------------------------------------------------
# voxelization
# ------------------------------------------------------------------------------------------------------------------
def _voxel_case(case):
    g = load_golden('voxelize.npz')
    return g[f'{case}::voxel_size'].tolist(), g[f'{case}::range'].tolist()


@pytest.mark.parametrize('ncol', [3, 9])
@pytest.mark.parametrize('case', ['sst', 'fsd', 'fsdv2'])
def test_voxelize_plain_kernel_on_the_boundary_set(case, ncol):
    import sst_amd
    vs, rng = _voxel_case(case)
    pts = R.voxel_boundary_points(vs, rng, ncol)
    ref = R.voxel_ref(pts, vs, rng)
    out = sst_amd.voxelization(_dev(pts), vs, rng, -1, -1)
    assert out.dtype == torch.int32 and out.shape == (len(pts), 3)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    if ncol == 9:      # rows wider than the streaming kernel takes: the plain kernel with the batch column
        _, coors = sst_amd.Voxelization(vs, rng, -1, (-1, -1)).voxelize_batch([_dev(pts), _dev(pts[::-1].copy())])
        want = np.concatenate([np.pad(ref, ((0, 0), (1, 0)), constant_values=0),
                               np.pad(ref[::-1], ((0, 0), (1, 0)), constant_values=1)])
        np.testing.assert_array_equal(coors.cpu().numpy(), want)


@pytest.mark.parametrize('ncol', [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize('case', ['sst', 'fsd', 'fsdv2'])
def test_voxelize_streaming_rows_kernel_on_the_boundary_set(case, ncol):
    """the LDS-staged kernel (n >= 4096, rows of up to 8 floats): 4096 / 4097 / 17 * 256 - 1 / 17 * 256 rows, and a second
    sample that starts at a row offset that is no multiple of the 256-row tile"""
    import sst_amd
    vs, rng = _voxel_case(case)
    pts = R.voxel_boundary_points(vs, rng, ncol)
    vox = sst_amd.Voxelization(vs, rng, -1, (-1, -1))
    second = R.pad_or_trim(pts[::-1], 4099)
    ref2 = np.pad(R.voxel_ref(second, vs, rng), ((0, 0), (1, 0)), constant_values=1)
    for n in (4096, 4097, 4351, 4352):
        first = R.pad_or_trim(pts, n)
        # a set longer than n loses its tail in the first sample (for x: the specials and the points outside the range);
        # the second sample is the set reversed, so the two together must hold every row
        assert min(n, len(pts)) + min(len(second), len(pts)) >= len(pts)
        _, coors = vox.voxelize_batch([_dev(first), _dev(second)])
        want = np.concatenate([np.pad(R.voxel_ref(first, vs, rng), ((0, 0), (1, 0)), constant_values=0), ref2])
        np.testing.assert_array_equal(coors.cpu().numpy(), want)
