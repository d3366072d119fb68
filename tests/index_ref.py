"""TEST INFRASTRUCTURE ONLY - plain numpy / Python references of the integer front end (scan, radix sort, sorted-unique,
in-group rank, window coordinates, region batching, window launch order, dynamic voxelization) and the builders of the
inputs that put every structural edge of the kernels on the table.  The host test (test_index_ref_host.py) proves the
references against brute force and the inputs against mutated references; the GPU test (test_gpu_index_edges.py) runs the
very same inputs through the kernels, bit for bit.

Where the oracle package already IS the definition (oracle.sst_oracle.ingroup_rank / window_coors / region_batching) it is
reused; what it lacks (keep mask over the input voxels, new numbering, per-window level, largest window) is added here.
"""
import itertools

import numpy as np

from oracle import sst_oracle
from oracle.voxel_oracle import dynamic_voxelize_grid

# structural units of csrc/sort_scan.hip
UNIT_IPT = 8          # kScanIpt: values per thread of the scan kernels
UNIT_WAVE = 64        # one wave / one ballot round of radix_scatter_k
UNIT_WAVE_SHARE = 512  # kSortIpt * 64: the keys one wave of the sort owns; kScanIpt * 64: one wave of the scan
UNIT_TILE = 2048      # kScanTile == kSortTile: one workgroup
UNIT_SPINE = 524288   # kScanTile * kScanThreads: the scan's spine takes a second round beyond 256 tiles


def edge_lengths(*units):
    """u - 1, u, u + 1 for every structural unit, ascending and without repeats"""
    out = set()
    for u in units:
        out.update((u - 1, u, u + 1))
    return sorted(v for v in out if v >= 0)


# ------------------------------------------------------------------------------------------------------------------
# scan / sort / unique
# ------------------------------------------------------------------------------------------------------------------
def scan_ref(x):
    """exclusive prefix sum of int32 values -> (out int32 [n], total); every prefix must fit int32"""
    x = np.asarray(x, dtype=np.int64)
    inc = np.cumsum(x)
    if x.size:
        assert np.abs(inc).max() < 2 ** 31, 'the input builder must keep every prefix inside int32'
    out = np.concatenate([[0], inc[:-1]]) if x.size else inc
    return out.astype(np.int32), int(inc[-1]) if x.size else 0


def scan_values(n, seed):
    """signed, large int32 values whose every prefix stays inside int32: the prefix sums themselves are drawn uniformly
    from (-2^30, 2^30), the values are their differences (|x| < 2^31)"""
    rng = np.random.default_rng(seed)
    prefix = rng.integers(-(1 << 30) + 1, 1 << 30, size=n, dtype=np.int64)      # inclusive prefix sums
    x = np.diff(prefix, prepend=0)
    assert np.abs(x).max(initial=0) < 2 ** 31
    return x.astype(np.int32)


def scan_single_one(n, pos):
    x = np.zeros(n, dtype=np.int32)
    x[pos] = 1
    return x


def sort_ref(keys):
    """keys: int64 bit patterns.  Stable ascending order of the uint64 view -> (sorted keys int64, perm int64)"""
    keys = np.ascontiguousarray(np.asarray(keys, dtype=np.int64))
    order = np.argsort(keys.view(np.uint64), kind='stable')
    return keys[order], order.astype(np.int64)


def _u64_to_i64(a):
    return np.asarray(a, dtype=np.uint64).view(np.int64)


def full_width_keys(n, key_bits, seed):
    """n keys drawn (with repeats) from a pool of ~n/4 distinct values spread uniformly over all key_bits bits: every digit
    of every pass varies, duplicates exist (stability is observable), and for key_bits == 64 half the keys have the top
    bit set.  For n >= 1024 the pool is completed so that every pass sees all 256 digit values."""
    rng = np.random.default_rng(seed)
    npool = max(1, n // 4)
    raw = rng.integers(0, 1 << 63, size=npool, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=npool, dtype=np.uint64)
    if npool >= 256:
        # digit p of pool entry i (i < 256) := a permutation of 0..255, one permutation per pass
        passes = (key_bits + 7) // 8
        for p in range(passes):
            perm = rng.permutation(256).astype(np.uint64)
            sh = np.uint64(8 * p)
            raw[:256] = (raw[:256] & ~(np.uint64(0xFF) << sh)) | (perm << sh)
    if key_bits < 64:
        raw &= np.uint64((1 << key_bits) - 1)
    idx = rng.integers(0, npool, size=n)
    idx[:min(n, npool)] = rng.permutation(npool)[:min(n, npool)]     # every pool value is used when n allows
    keys = raw[idx]
    if n >= 2 * npool and n >= 2:
        assert np.unique(keys).size < n
    return _u64_to_i64(keys)


def sort_patterns(n, key_bits):
    """the fixed patterns: name -> int64 keys"""
    top = (1 << key_bits) - 1
    i = np.arange(n, dtype=np.uint64)
    pats = {
        'zeros': np.zeros(n, dtype=np.uint64),
        'ones': np.full(n, top, dtype=np.uint64),
        'alternating': np.where(i % np.uint64(2) == 0, np.uint64(top), np.uint64(top >> 1 if key_bits > 1 else 0)),
        'ascending': i & np.uint64(top),
        'descending': (np.uint64(n - 1) - i) & np.uint64(top),
    }
    passes = (key_bits + 7) // 8
    for d in range(passes):
        width = min(8, key_bits - 8 * d)
        # keys equal everywhere but in digit d, which runs through its values in a scrambled order; the other digits are
        # non-zero so that a pass that moves them shows
        base = np.uint64(0x5A5A5A5A5A5A5A5A & top & ~(0xFF << (8 * d)))
        dig = (i * np.uint64(167) + np.uint64(13)) % np.uint64(1 << width)
        pats['digit%d' % d] = base | (dig << np.uint64(8 * d))
    return {k: _u64_to_i64(v) for k, v in pats.items()}


def _mask_invalid(rows, mode):
    rows = np.array(rows, dtype=np.int64, copy=True)
    if mode == 1:
        bad = (rows < 0).any(1)
        rows[bad] = -1
    elif mode == 2:
        bad = (rows[:, 1:] < 0).any(1)
        rows[bad, 1:] = -1
    return rows


def unique_ref(rows, mode=0):
    """sorted-unique of integer rows the way the reference states it: masked_fill(any(< 0), -1) (mode 1: the whole row;
    mode 2: columns 1.. of the row, per sample = per value of column 0), then the lexicographic unique - for mode 2 of
    every sample on its own, samples in ascending order.
    -> dict(inverse [n], counts [m], rows [m, k], perm [n] = lexsort by (group, row index), offsets [m + 1])"""
    rows = np.asarray(rows, dtype=np.int64)
    n, k = rows.shape
    clean = _mask_invalid(rows, mode)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return dict(inverse=z, counts=z, rows=np.zeros((0, k), dtype=np.int64), perm=z, offsets=np.zeros(1, dtype=np.int64))
    if mode == 2 and k > 1:
        inverse = np.empty(n, dtype=np.int64)
        uniq, counts = [], []
        base = 0
        for b in np.unique(clean[:, 0]):
            sel = np.nonzero(clean[:, 0] == b)[0]
            u, inv, cnt = np.unique(clean[sel][:, 1:], axis=0, return_inverse=True, return_counts=True)
            inverse[sel] = inv.reshape(-1) + base
            uniq.append(np.concatenate([np.full((u.shape[0], 1), b, dtype=np.int64), u], 1))
            counts.append(cnt)
            base += u.shape[0]
        uniq, counts = np.concatenate(uniq), np.concatenate(counts)
    else:
        uniq, inverse, counts = np.unique(clean, axis=0, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
    perm = np.lexsort((np.arange(n), inverse))
    offsets = np.concatenate([[0], np.cumsum(counts)])
    return dict(inverse=inverse.astype(np.int64), counts=counts.astype(np.int64), rows=uniq.astype(np.int64),
                perm=perm.astype(np.int64), offsets=offsets.astype(np.int64))


def unique_rows_input(n, ncols, kind, seed, mode=0):
    """[n, ncols] int64 rows.  kind: 'equal' (m == 1), 'distinct' (m == n), 'random' (many repeats).
    mode 0: values of both signs (negative mins).  modes 1 / 2: valid values are >= 0 and about one row in twelve holds a
    negative entry in ONE column (for mode 2 never in column 0, the sample index) while the minimum of every other column
    stays above zero - the case in which bounds taken from the data must be lowered to -1."""
    rng = np.random.default_rng(seed)
    if kind == 'equal':
        return np.tile(np.arange(ncols, dtype=np.int64) * 3 + (-4 if mode == 0 else 2), (n, 1))
    if mode == 0:
        rows = rng.integers(-4, 5, size=(n, ncols), dtype=np.int64)
    else:
        rows = rng.integers(0, 6, size=(n, ncols), dtype=np.int64) + np.arange(ncols, dtype=np.int64)[None, :] + 1
        rows[:, 0] = rng.integers(0, 3, size=n)
        j0 = 1 if mode == 2 else 0
        if ncols > j0:
            bad = np.nonzero(rng.integers(0, 12, size=n) == 0)[0]
            rows[bad, j0 + seed % (ncols - j0)] = -1 - rng.integers(0, 3, size=bad.size)
    if kind == 'distinct':
        rows[:, ncols - 1] = rng.permutation(n) + (-(n // 2) if mode == 0 else 0)
    return rows


def unique_bounds(rows, mode):
    """per-column (mins, extents) the packed key needs: data bounds of the masked rows"""
    clean = _mask_invalid(rows, mode)
    if mode == 1:
        clean = np.maximum(clean, 0)       # the invalid group takes key 0, not a coordinate
    lo = clean.min(0)
    hi = clean.max(0)
    return [int(v) for v in lo], [int(h - l + 1) for l, h in zip(lo, hi)]


def keyspace_rows(n, mins, extents, seed):
    """n rows inside the box [mins, mins + extents) with the all-minimum and the all-maximum row present (the smallest
    and the largest packed key: 1 and total) and duplicates of both"""
    rng = np.random.default_rng(seed)
    k = len(mins)
    cols = []
    for j in range(k):
        # python ints: extents reach 2^62
        span = int(extents[j])
        draw = rng.integers(0, min(span, 1 << 62), size=n, dtype=np.int64) if span > 1 else np.zeros(n, dtype=np.int64)
        cols.append(draw + int(mins[j]))
    rows = np.stack(cols, 1)
    lo = np.asarray([int(m) for m in mins], dtype=np.int64)
    hi = np.asarray([int(m) + int(e) - 1 for m, e in zip(mins, extents)], dtype=np.int64)
    if n >= 1:
        rows[n // 2] = hi
    if n >= 2:
        rows[0] = lo
    if n >= 4:
        rows[n - 1] = lo
        rows[1] = hi
    if n >= 8:                                  # some more repeats
        rows[n // 3] = rows[n // 3 + 1]
    return rows


# key spaces whose size sits on a pass boundary (total + 1 values incl. the invalid key 0): total -> [(mins, extents)]
def keyspace_boxes():
    return {
        255: ([0, -3], [5, 51]),
        256: ([-7, 0, 2], [4, 8, 8]),
        257: ([3], [257]),
        65535: ([0, -1, 0], [3, 5, 4369]),
        65536: ([-100, 0], [256, 256]),
        65537: ([0], [65537]),
        (1 << 32) - 1: ([0, -2, 5], [65535, 1, 65537]),
        1 << 32: ([-(1 << 20), 0, 0], [1 << 16, 1 << 8, 1 << 8]),
        1 << 62: ([-(1 << 30), -5, 0], [1 << 31, 1 << 20, 1 << 11]),
    }


# ------------------------------------------------------------------------------------------------------------------
# window order, region batching
# ------------------------------------------------------------------------------------------------------------------
def window_order_ref(sizes):
    """launch order of the windows: ids by ascending token count, ties in id order"""
    return np.argsort(np.asarray(sizes, dtype=np.int64), kind='stable').astype(np.int64)


def window_order_sizes(n, cap, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == 'equal':
        return np.full(n, cap, dtype=np.int64)
    if kind == 'zero_or_cap':
        return rng.integers(0, 2, size=n, dtype=np.int64) * cap
    sizes = rng.integers(0, cap + 1, size=n, dtype=np.int64)
    sizes[rng.integers(0, n, size=max(1, n // 3))] = cap          # ties at the cap, as after the drop
    sizes[rng.integers(0, n, size=max(1, n // 5))] = cap // 2
    return sizes


def levels_of(drop_info):
    """drop_info dict -> the kernels' list of (max_tokens, lo, hi)"""
    return [(drop_info[k]['max_tokens'], drop_info[k]['drop_range'][0], drop_info[k]['drop_range'][1]) for k in drop_info]


def drop_table(levels):
    return {i: {'max_tokens': c, 'drop_range': (lo, hi)} for i, (c, lo, hi) in enumerate(levels)}


# further tables: one level; eight levels; overlapping ranges (the later level wins); a table with a hole at >= 100
# (a population there matches no level: the whole window is dropped with level -1)
DROP_ONE = drop_table([(50, 0, 100000)])
DROP_EIGHT = drop_table([(8, 0, 10), (15, 10, 20), (25, 20, 30), (35, 30, 40), (45, 40, 50), (55, 50, 60), (65, 60, 70),
                         (75, 70, 100000)])
DROP_OVERLAP = drop_table([(20, 0, 50), (40, 30, 100000), (10, 40, 45)])
DROP_GAP = drop_table([(30, 0, 30), (60, 30, 60), (100, 60, 100)])


def edge_populations(drop_info):
    """b - 1, b, b + 1 for every level boundary and every cap of the table, plus 1 and 99 / 100 / 101"""
    pops = {1, 99, 100, 101}
    for lv in drop_info.values():
        lo, hi = lv['drop_range']
        for b in (lo, hi, lv['max_tokens']):
            if 1 < b < 10000:
                pops.update((b - 1, b, b + 1))
    return sorted(p for p in pops if p >= 1)


def region_ref(win0, win1, drop_info):
    """oracle.sst_oracle.region_batching plus what the kernels also return: the keep mask and the new numbering over the
    INPUT voxels, level / flat2win over the input voxels (-1 where undefined), the level of every surviving window,
    window counts and the largest surviving window of each shift"""
    # window identity and order are all the drop depends on: the oracle counts with np.bincount, one counter per id up to the
    # largest, so ids that use the top bit of a 31-bit id space go in as their ranks and come out as themselves
    ids0, win0 = np.unique(np.asarray(win0, dtype=np.int64), return_inverse=True)
    ids1, win1 = np.unique(np.asarray(win1, dtype=np.int64), return_inverse=True)
    win0, win1 = win0.reshape(-1), win1.reshape(-1)
    m = win0.shape[0]
    out = sst_oracle.region_batching(win0, win1, drop_info)
    out['win0'], out['win1'] = ids0[out['win0']], ids1[out['win1']]
    keep = np.zeros(m, dtype=bool)
    keep[out['keep_idx']] = True
    out['keep'] = keep
    out['newidx'] = (np.cumsum(keep) - keep).astype(np.int64)
    k0, l0_all = sst_oracle.drop_single_shift(win0, drop_info)
    out['keep0'] = k0
    out['level0_all'] = l0_all.astype(np.int64)                       # not recomputed after the shift-1 filter
    l1_all = -np.ones(m, dtype=np.int64)
    if k0.any():
        l1_all[k0] = sst_oracle.drop_single_shift(win1[k0], drop_info)[1]
    out['level1_all'] = l1_all
    for s in range(2):
        f2w = -np.ones(m, dtype=np.int64)
        f2w[out['keep_idx']] = out[f'flat2win{s}']
        out[f'flat2win{s}_all'] = f2w
        off = out[f'winoff{s}']
        nw = len(off) - 1
        out[f'n_windows{s}'] = nw
        out[f'max_tokens{s}'] = int(np.diff(off).max()) if nw else 0
        w, lv = out[f'win{s}'], out[f'level{s}']
        first = out[f'tok{s}'][off[:-1]] if nw else np.zeros(0, dtype=np.int64)
        out[f'winlevel{s}'] = lv[first].astype(np.int64)
        # every voxel of a surviving window carries the window's level
        if nw:
            assert (np.repeat(out[f'winlevel{s}'], np.diff(off)) == lv[out[f'tok{s}']]).all()
    return out


def window_major(ref):
    """the plan of SSTInputLayerV2(window_major=True) / FramePlanner from the oracle's: kept voxels listed by their
    shift-0 window slot -> (voxel_keep_inds, tok0, tok1)"""
    tok0, tok1 = ref['tok0'], ref['tok1']
    mk = tok0.size
    keep = ref['keep_idx'][tok0]
    inv = np.empty(mk, dtype=np.int64)
    inv[tok0] = np.arange(mk)
    return keep, np.arange(mk), inv[tok1]


def _spread_ids(n, win_bits, rng):
    """n distinct ids below 2^win_bits in scrambled order; 0 and 2^win_bits - 1 are among them and every second one
    uses the top bit"""
    top = 1 << win_bits
    assert n <= top
    half = top >> 1
    n_hi = min((n + 1) // 2, half)
    n_lo = n - n_hi
    assert n_lo <= half

    def pick(count, lo, hi, must):
        if count == 0:
            return np.zeros(0, dtype=np.int64)
        if hi - lo <= 4 * count + 8:
            ids = rng.permutation(np.arange(lo, hi, dtype=np.int64))[:count]
        else:
            ids = np.unique(rng.integers(lo, hi, size=4 * count + 8, dtype=np.int64))
            ids = rng.permutation(ids)[:count]
        if must not in ids:
            ids[0] = must
        return ids

    ids = np.concatenate([pick(n_hi, half, top, top - 1), pick(n_lo, 0, half, 0)])
    assert np.unique(ids).size == n
    return rng.permutation(ids)


_FILLER = (1, 2, 3, 5, 8, 13)


def rb_scene(drop_info, n_win0=256, win_bits=13, seed=0):
    """Region-batching scene given directly as (win0, win1) id arrays, the voxels of every window interleaved across the
    array.  Shift 0: one window for every population of edge_populations(drop_info), small filler windows up to n_win0
    distinct ids.  Shift 1: among the voxels that survive the shift-0 drop (reference semantics) windows of the same
    populations are formed from a random selection of survivors, so the shift-1 drop thins shift-0 windows (some of
    them across a level boundary: the "level0 is not recomputed" quirk); the rest goes to filler windows.
    ids: n distinct values below 2^win_bits, top bit in use, 0 and 2^win_bits - 1 present, order scrambled.
    -> (win0 int64 [m], win1 int64 [m], populations list)"""
    rng = np.random.default_rng(seed)
    pops = edge_populations(drop_info)
    sizes0 = list(pops)
    i = 0
    while len(sizes0) < n_win0:
        sizes0.append(_FILLER[i % len(_FILLER)])
        i += 1
    assert len(sizes0) == n_win0, 'n_win0 must hold one window per edge population'
    ids0 = _spread_ids(n_win0, win_bits, rng)
    win0 = np.repeat(ids0, sizes0)
    win0 = win0[rng.permutation(win0.size)]                           # interleave
    keep0, _ = sst_oracle.drop_single_shift(np.unique(win0, return_inverse=True)[1].reshape(-1), drop_info)   # dense ids
    surv = rng.permutation(np.nonzero(keep0)[0])
    sizes1, left = [], surv.size
    for p in sorted(pops, reverse=True):                              # the large ones first: they must fit
        if p <= left:
            sizes1.append(p)
            left -= p
    i = 0
    while left > 0:
        s = min(left, _FILLER[i % len(_FILLER)])
        sizes1.append(s)
        left -= s
        i += 1
    # the level0 quirk, by construction: the LAST voxel (in array order) of a shift-0 window whose population sits exactly on
    # a lower level bound becomes the last voxel of the largest shift-1 window, which is over its cap (or in a hole of the
    # table) - the shift-1 drop takes it, and the shift-0 window falls below the bound while keeping its level
    quirk = [b for b in pops if any(lv['drop_range'][0] == b for lv in drop_info.values()) and b > 1]
    if quirk and sizes1 and sizes1[0] > 1:
        victim = int(np.nonzero(win0 == ids0[sizes0.index(quirk[0])])[0].max())
        if keep0[victim]:
            smaller = [int(v) for v in surv if v < victim]
            if len(smaller) >= sizes1[0] - 1:
                first = smaller[:sizes1[0] - 1] + [victim]
                taken = set(first)
                surv = np.asarray(first + [int(v) for v in surv if int(v) not in taken], dtype=np.int64)
    limit = 1 << win_bits
    while len(sizes1) + 1 > limit:                                    # few ids: merge filler windows
        a = sizes1.pop()
        sizes1[-1] += a
    ids1 = _spread_ids(len(sizes1) + 1, win_bits, rng)
    win1 = np.full(win0.size, ids1[-1], dtype=np.int64)               # voxels dropped by shift 0: one window of their own
    win1[surv] = np.repeat(ids1[:-1], sizes1)
    return win0.astype(np.int64), win1.astype(np.int64), pops


# ------------------------------------------------------------------------------------------------------------------
# geometric twin: voxels in the 468 x 468 grid, 12 x 12 windows
# ------------------------------------------------------------------------------------------------------------------
TWIN_SPARSE = (468, 468, 1)
TWIN_WINDOW = (12, 12, 1)


def twin_voxels(drop_info, seed=0):
    """(b, z, y, x) voxel rows, two samples, whose shift-0 windows hold the edge populations (those that fit a 12 x 12
    window: <= 144).  The windows sit side by side in a block, so the shifted partition mixes quadrants of neighbours,
    plus one window in each far corner of the grid, plus four windows of 99 that give the shifted partition a window of 100.  Rows are returned sorted (b, z, y, x) - the order of a sorted-unique."""
    rng = np.random.default_rng(seed)
    pops = [p for p in edge_populations(drop_info) if p <= 144]
    rows = []
    for b in range(2):
        order = pops if b == 0 else pops[::-1]
        slots = [(38, 38), (0, 38), (0, 0)] + [(10 + i % 4, 20 + i // 4) for i in range(len(order))]
        for (wi, wj), p in zip(slots, order):
            # voxel (y, x) = (0, 0) stays free: twin_points puts the voxel there that DynamicVFE discards
            cells = rng.permutation(np.arange(1, 144) if (wi, wj) == (0, 0) else 144)[:p]
            assert cells.size == p
            x = wi * 12 + cells % 12
            y = wj * 12 + cells // 12
            rows.append(np.stack([np.full(p, b), np.zeros(p, dtype=np.int64), y, x], 1))
        # four more windows of 99 voxels around one corner, 25 voxels of each in the quadrant at the corner: the shifted
        # window centred there holds exactly 100 - a level boundary (a hole, in a table that has one) at shift 1 as well
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            cx, cy = np.meshgrid(np.arange(12), np.arange(12))
            cx, cy = cx.reshape(-1), cy.reshape(-1)
            inner = ((cx >= 6) if dx == 0 else (cx < 6)) & ((cy >= 6) if dy == 0 else (cy < 6))
            cells = np.concatenate([rng.permutation(np.nonzero(inner)[0])[:25], rng.permutation(np.nonzero(~inner)[0])[:74]])
            x = (20 + dx) * 12 + cx[cells]
            y = (30 + dy) * 12 + cy[cells]
            rows.append(np.stack([np.full(99, b), np.zeros(99, dtype=np.int64), y, x], 1))
    rows = np.concatenate(rows).astype(np.int64)
    order = np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))
    return rows[order], pops


def twin_points(voxels, voxel_size, pc_range, seed=0):
    """the twin as point clouds at voxel centres, one [n, 3] float32 array per sample (points in scrambled order, some
    voxels hit twice), with one extra point per sample in voxel (0, 0, 0), which sorts before all others: DynamicVFE
    discards the first sorted voxel of every sample (the reference's DynamicScatter quirk)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(voxel_size, dtype=np.float64)
    lo = np.asarray(pc_range[:3], dtype=np.float64)
    out = []
    for b in range(2):
        c = voxels[voxels[:, 0] == b][:, 1:]                              # (z, y, x)
        assert not ((c[:, 1] == 0) & (c[:, 2] == 0)).any()
        c = np.concatenate([c, c[rng.integers(0, len(c), size=len(c) // 5)], np.zeros((1, 3), dtype=np.int64)])
        xyz = (c[:, ::-1] + 0.5) * v[None, :] + lo[None, :]
        out.append(xyz[rng.permutation(len(xyz))].astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------------------------
# voxelization
# ------------------------------------------------------------------------------------------------------------------
def voxel_quotient(p, lo, v):
    """fp32 subtract, correctly rounded fp32 divide (numpy float32 arithmetic is IEEE)"""
    with np.errstate(all='ignore'):
        return ((np.asarray(p, dtype=np.float32) - np.float32(lo)) / np.float32(v)).astype(np.float32)


def voxel_coord_from_quotient(q, g):
    """(int)floor(q) clamped to [0, g - 1], stated without a float-to-int cast of anything out of range:
    NaN -> 0, q >= g (incl. +inf) -> g - 1, q < 0 (incl. -inf) -> 0"""
    q = np.asarray(q, dtype=np.float32)
    c = np.zeros(q.shape, dtype=np.int64)
    hi = q >= np.float32(g)           # g <= 2^24 is exact in float32
    mid = (q >= 0) & ~hi              # False for NaN
    with np.errstate(all='ignore'):
        c[mid] = np.floor(q[mid]).astype(np.int64)
    c[hi] = g - 1
    return c


def voxel_ref(points, voxel_size, coors_range):
    """points [N, >= 3] float32 -> int32 [N, 3] (z, y, x)"""
    p = np.asarray(points, dtype=np.float32)
    grid = dynamic_voxelize_grid(voxel_size, coors_range)             # (gx, gy, gz)
    cols = [voxel_coord_from_quotient(voxel_quotient(p[:, a], coors_range[a], voxel_size[a]), int(grid[a])) for a in range(3)]
    return np.stack(cols[::-1], 1).astype(np.int32)


VOXEL_SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 3e38, -3e38, np.inf, -np.inf, np.nan],
                          dtype=np.float32)


def voxel_axis_probes(lo, v, g, hi):
    """probes of one axis: fl(lo + k v) and its +-1, +-2 ulp neighbours for k = 0..g, the same face moved by 1 and 2 ulps of
    the QUOTIENT k (where |p| is small next to k v, ulps of p do not reach the next quotient), the specials, and points
    just outside both ends of the range"""
    lo32, v32 = np.float32(lo), np.float32(v)
    k = np.arange(g + 1, dtype=np.float64)
    face = (np.float64(lo32) + k * np.float64(v32)).astype(np.float32)
    down1 = np.nextafter(face, np.float32(-np.inf))
    down2 = np.nextafter(down1, np.float32(-np.inf))
    up1 = np.nextafter(face, np.float32(np.inf))
    up2 = np.nextafter(up1, np.float32(np.inf))
    qstep = (np.spacing(np.maximum(k, 1).astype(np.float32)).astype(np.float64) * np.float64(v32))
    moved = [(np.float64(lo32) + k * np.float64(v32) + j * qstep).astype(np.float32) for j in (-2, -1, 1, 2)]
    hi32 = np.float32(hi)
    outside = np.array([lo32 - v32, lo32 - np.float32(0.5) * v32, np.nextafter(lo32, np.float32(-np.inf)), lo32 - np.float32(1e-3),
                        hi32, np.nextafter(hi32, np.float32(np.inf)), hi32 + np.float32(0.5) * v32, hi32 + v32,
                        hi32 + np.float32(1e-3), np.float32(1e6), np.float32(-1e6)], dtype=np.float32)
    return np.concatenate([np.stack([down2, down1, face, up1, up2] + moved, 1).reshape(-1), VOXEL_SPECIALS, outside]).astype(np.float32)


def voxel_boundary_points(voxel_size, coors_range, ncol=3, seed=0):
    """[N, ncol] float32: column a holds the probes of axis a (the shorter lists repeat), further columns are noise"""
    grid = dynamic_voxelize_grid(voxel_size, coors_range)
    probes = [voxel_axis_probes(coors_range[a], voxel_size[a], int(grid[a]), coors_range[a + 3]) for a in range(3)]
    n = max(len(p) for p in probes)
    rng = np.random.default_rng(seed)
    cols = []
    for a in range(3):
        col = np.resize(probes[a], n)
        if a:                                   # decouple the axes: every axis in its own scrambled order
            col = col[rng.permutation(n)]
        cols.append(col)
    for _ in range(ncol - 3):
        cols.append(rng.standard_normal(n).astype(np.float32))
    return np.stack(cols, 1).astype(np.float32)


def pad_or_trim(points, n):
    """first n rows; a shorter set repeats"""
    idx = np.arange(n) % points.shape[0]
    return np.ascontiguousarray(points[idx])


# ------------------------------------------------------------------------------------------------------------------
# window coordinates
# ------------------------------------------------------------------------------------------------------------------
def window_corner_voxels(sparse_shape, window_shape, batch):
    """(b, z, y, x) rows on the full cross product of {0, w//2 - 1, w//2, w - 1, w, s - 1} per axis (clipped to the
    grid), in samples 0 and batch - 1"""
    sx, sy, sz = sparse_shape
    wx, wy, wz = window_shape if len(window_shape) == 3 else (window_shape[0], window_shape[1], sparse_shape[2])

    def axis(s, w):
        return sorted({min(max(v, 0), s - 1) for v in (0, w // 2 - 1, w // 2, w - 1, w, s - 1)})

    rows = [(b, z, y, x) for b in sorted({0, batch - 1}) for z, y, x in itertools.product(axis(sz, wz), axis(sy, wy), axis(sx, wx))]
    return np.asarray(rows, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------
# the cases both test files walk through
# ------------------------------------------------------------------------------------------------------------------
SCAN_LENGTHS = sorted(set([0, 1] + edge_lengths(UNIT_IPT, UNIT_WAVE, UNIT_WAVE_SHARE, UNIT_TILE, UNIT_SPINE)))
SORT_KEY_BITS = sorted(set(b for k in range(1, 9) for b in (8 * k - 7, 8 * k)))
SORT_LENGTHS = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4097, 16383, 16384, 16385]
SORT_PATTERN_LENGTHS = [2049, 4097]
SORT_LARGE_N = 2048 * 2048 + 1     # 2049 sort tiles: the histogram (256 x 2049 counters) needs 257 scan tiles
UNIQUE_LENGTHS = edge_lengths(UNIT_WAVE, UNIT_TILE)
WINDOW_ORDER_N = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1040]
WINDOW_ORDER_CAPS = [0, 1, 510, 511, 512]
WINDOW_ORDER_KINDS = ['equal', 'zero_or_cap', 'random']
# (window shape, sparse shape): even and odd windows, sparse shapes that are no multiple of the window, one with sz == wz
WINDOW_CASES = [((12, 12, 1), (468, 468, 1)), ((12, 12), (470, 461, 1)), ((10, 10, 4), (512, 507, 41)),
                ((7, 5, 3), (100, 99, 10)), ((9, 11, 2), (50, 64, 2)), ((7, 5, 3), (30, 31, 3))]
RB_WIN_BITS = [8, 9, 16, 17, 24, 25, 31]
RB_WINDOW_COUNTS = [255, 256, 257]


def sort_cases():
    """(key_bits, n, seed) of the full-width runs"""
    return [(b, n, 1000 * b + i) for b in SORT_KEY_BITS for i, n in enumerate(SORT_LENGTHS)]
