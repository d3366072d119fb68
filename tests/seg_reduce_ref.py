"""Plain numpy restatement of the segmented reduction (csrc/scatter.hip, csrc/seg_tiles.h) and the groupings that put a
group on every length edge of its five forward kernel classes (tests/test_gpu_seg_reduce_edges.py; pinned on the CPU by
tests/test_seg_reduce_ref_host.py).

The operation: output row g reduces the rows i of ``feats`` with ``ids[i] == g`` (ids outside [0, m) belong to no row).
  SUM   starts from +0.0, so a sum that is zero is +0.0 whatever the signs of the zeros that went in;
  MEAN  is fl32(fl32(sum) / fl32(len)), one fp32 division;
  MAX   records the smallest row whose value compares equal to the maximum (+0.0 == -0.0: the smaller row wins, and the
        value is that row's value, sign included); an empty group gives the value 0 and the row n.
NaN is outside the contract (and with it inf - inf in a sum)."""
import numpy as np

SPAN = 8            # kSegSpan: sorted rows per row lane of a tile
CHUNK = 512         # kSegChunk: rows per work-list entry
WORK_LIMIT = 32     # kWorkGroupLen: longer groups go to the work list
BLOCK_LIMIT = 16    # kLongGroup: longer groups go to seg_reduce_fwd_block_k (no work list, n >= 8 m)
WORK_HEADER = 8     # kSegWorkHdr


def grouping(lens, seed):
    """ids [n] (group k has lens[k] rows, scattered by a seeded shuffle) and coordinate rows [n, 3] whose sorted-unique
    order is the id order (kernels.unique_rows)"""
    lens = np.asarray(lens, np.int64)
    ids = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    np.random.default_rng(seed).shuffle(ids)
    coors = np.stack([np.zeros_like(ids), ids // 251, ids % 251], 1)
    return ids, coors


def exact_feats(n, c, seed):
    """small integers in [-3, 3] with +0.0 / -0.0 sprinkled in: every sum is exact in fp32 in any order, ties everywhere"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(n, c)).astype(np.float32)
    x[rng.random((n, c)) < 0.05] = 0.0
    x[rng.random((n, c)) < 0.05] = -0.0
    return x


def _csr(ids, m):
    ids = np.asarray(ids, np.int64)
    rows = np.flatnonzero((ids >= 0) & (ids < m))
    order = rows[np.argsort(ids[rows], kind='stable')]      # ascending rows inside a group
    lens = np.bincount(ids[rows], minlength=m).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return order, lens, starts


def group_lens(ids, m):
    return _csr(ids, m)[1]


def reduce_ref(feats, ids, m, mode):
    """'sum' / 'mean': values [m, c] (int64 for integer input, else float64; mean always float64); 'max': (values, rows) with
    rows int64 = the smallest row attaining the maximum, n for an empty group.  Empty groups have the value 0."""
    feats = np.asarray(feats)
    n, c = feats.shape
    acc_t = np.int64 if feats.dtype.kind in 'iu' else np.float64
    order, lens, starts = _csr(ids, m)
    full = lens > 0
    at = starts[full]
    fs = feats[order].astype(acc_t)
    if mode in ('sum', 'mean'):
        out = np.zeros((m, c), acc_t)
        if at.size:
            out[full] = np.add.reduceat(fs, at, axis=0)
        if acc_t is np.float64:
            out = out + 0.0                                  # the accumulators start from +0.0
        if mode == 'mean':
            out = np.where(full[:, None], out / np.maximum(lens, 1)[:, None].astype(np.float64), 0.0)
        return out
    assert mode == 'max'
    vals = np.zeros((m, c), acc_t)
    arg = np.full((m, c), n, np.int64)
    if at.size:
        mx = np.maximum.reduceat(fs, at, axis=0)
        gid = np.repeat(np.arange(int(full.sum())), lens[full])
        hit = np.where(fs == mx[gid], order[:, None], n)
        arg[full] = np.minimum.reduceat(hit, at, axis=0)
        vals[full] = np.take_along_axis(feats.astype(acc_t), arg[full], axis=0)
    return vals, arg


def expect_f32(feats, ids, m, mode):
    """what a kernel must give bit for bit on exact operands: fp32 [m, c] (and the rows for 'max')"""
    feats = np.asarray(feats, np.float32)
    if mode == 'max':
        vals, arg = reduce_ref(feats, ids, m, 'max')
        return vals.astype(np.float32), arg
    s = reduce_ref(feats, ids, m, 'sum').astype(np.float32)
    if mode == 'sum':
        return s
    lens = group_lens(ids, m)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = s / lens.astype(np.float32)[:, None]             # one correctly rounded fp32 division
    return np.where(lens[:, None] > 0, q, np.float32(0.0)).astype(np.float32)


def grad_ref(gout, rows_of_point, n, mode, arg=None, lens=None, limit=None):
    """gradient of the rows [n, c] (fp32).  rows_of_point [n]: output row of every point (outside [0, limit): none).
    'max': gout[g, ch] goes to row arg[g, ch] (>= n: nowhere); 'sum': gout[row]; 'mean': fl32(gout[row] / fl32(len[row]))"""
    gout = np.asarray(gout, np.float32)
    m, c = gout.shape
    limit = m if limit is None else min(int(limit), m)
    g = np.zeros((n, c), np.float32)
    if mode == 'max':
        arg = np.asarray(arg)[:limit]
        gi, ch = np.nonzero((arg >= 0) & (arg < n))
        g[arg[gi, ch], ch] = gout[gi, ch]
        return g
    r = np.asarray(rows_of_point, np.int64)
    ok = (r >= 0) & (r < limit)
    g[ok] = gout[r[ok]]
    if mode == 'mean':
        g[ok] = g[ok] / np.asarray(lens)[r[ok]].astype(np.float32)[:, None]
    return g


def sum_bound(feats, ids, m):
    """|fl(sum) - sum| <= gamma_len * sum |x_i| for fp32 sums in ANY association, gamma_k = k u / (1 - k u), u = 2^-24; and
    the bound of the mean: that divided by len, plus u |mean| for the division"""
    u = 2.0 ** -24
    lens = group_lens(ids, m).astype(np.float64)[:, None]
    gamma = lens * u / (1.0 - lens * u)
    mag = reduce_ref(np.abs(np.asarray(feats, np.float64)), ids, m, 'sum')
    mean = np.abs(reduce_ref(np.asarray(feats, np.float64), ids, m, 'mean'))
    b_sum = gamma * mag
    return b_sum, b_sum / np.maximum(lens, 1.0) + u * mean


# ---- geometry of the kernels, restated ---------------------------------------------------------------------------------
def tile_shape(c, n):
    """seg_tiles_shape: (channel vector width, channel vectors, row lanes, rows of a tile)"""
    v = 4 if c % 4 == 0 else 1
    cv = c // v
    lanes = min(256 // cv, 32)
    while lanes > 8 and n // (lanes * SPAN) < 256:
        lanes >>= 1
    return v, cv, lanes, lanes * SPAN


def _align(x, a):
    return (x + a - 1) // a * a


def long_scratch_bytes(c, n, m):
    """sst_segment_long_scratch_bytes: one int32 ticket counter per group, two records of 32 bytes per tile and channel vector"""
    _, cv, _, rows = tile_shape(c, n)
    tiles = (n + rows - 1) // rows
    return _align(4 * m, 256) + _align(tiles * 2 * cv * 32, 256)


def work_capacities(n, m, c):
    """seg_work_shape: (entries, cut groups, partial slots, padded width)"""
    chunks = n // CHUNK + 1
    return _align(m + chunks, 4), _align(chunks, 4), 2 * chunks, _align(c, 4)


def work_words(n, m, c):
    cap_e, cap_m, cap_p, cpad = work_capacities(n, m, c)
    return WORK_HEADER + 3 * cap_e + 3 * cap_m + 2 * cap_p * cpad


def work_demand(lens, limit=WORK_LIMIT):
    """(entries, cut groups, partial slots) a grouping asks of its work list"""
    lens = np.asarray(lens, np.int64)
    lens = lens[lens > limit]
    chunks = (lens + CHUNK - 1) // CHUNK
    return int(chunks.sum()), int((chunks > 1).sum()), int(chunks[chunks > 1].sum())


# ---- the groupings of the GPU test --------------------------------------------------------------------------------------
W_LENS = [1, 2, 3, 4, 5, WORK_LIMIT - 1, WORK_LIMIT, WORK_LIMIT + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK,
          2 * CHUNK + 1, 3 * CHUNK + 1]
B_LENS = [1, 4, 5, BLOCK_LIMIT - 1, BLOCK_LIMIT, BLOCK_LIMIT + 1, 255, 256, 257, 1000]
W4_WIDTHS = [4, 36, 68, 132, 256]
W1_WIDTHS = [1, 3, 5, 130, 257, 258]
B_WIDTHS = [4, 36, 132]
S_WIDTHS = [3, 64]
# (width, least number of rows): tile rows 64, 64, 64, 56 (7 lanes), 32 (4 lanes), 8 (1 lane), 128 (16 lanes), 256 (32 lanes)
T_CASES = [(4, 0), (3, 0), (64, 0), (132, 0), (256, 0), (255, 0), (64, 32768), (4, 65536)]
T_TAILS = ['0', '1', 'T-1']


def work_lens(first, singles=1100):
    """W_LENS among `singles` 1-row groups (n < 8 m); first = 1: group 0, which is discarded, is long"""
    return ([700] if first else []) + W_LENS[:8] + [1] * (singles // 2) + W_LENS[8:] + [1] * (singles - singles // 2)


def block_lens(first, singles=0):
    return ([300] if first else []) + B_LENS[:5] + [1] * singles + B_LENS[5:]


def tile_lens(c, n_min, first, tail):
    """group lengths that put a group on every edge of a tile of T rows / Ln row lanes (T_CASES, T_TAILS); first = 1: group 0,
    which is discarded, is long and crosses a tile.  n >= max(n_min, 8 m)."""
    guess = max(n_min, 1)
    for _ in range(3):
        T, Ln = tile_shape(c, guess)[3], tile_shape(c, guess)[2]
        lens = []

        def pos():
            return sum(lens)

        def pad_to(r):
            d = (r - pos()) % T
            if d:
                lens.append(d)

        if first:
            lens.append(T + 5)
        lens.append(3)
        lens.extend([1] * 17)                     # whole groups inside a span, runs of 1-row groups across lanes
        e = min(5, T - 1)
        pad_to(T - e)
        lens.append(e)                            # ends on the last row of a tile
        lens.append(3)                            # starts on the first row of the next
        pad_to(0)
        lens.append(T)                            # exactly one tile
        lens.append(3)
        lens.append(T)                            # a tile's worth of rows from the middle of a tile
        lens.append(2 * T + 1)
        lens.append((Ln + 3) * T)                 # more tiles than the finishing workgroup has row lanes
        filler = [9, 40, 1, 300, 17, 64, 8, 129, 2, 33]
        i = 0
        while pos() < n_min or pos() < 8 * (len(lens) + 2 - first) + T:
            lens.append(filler[i % len(filler)])
            i += 1
        want = {'0': 0, '1': 1, 'T-1': T - 1}[tail]
        pad_to(want)
        n = pos()
        if tile_shape(c, n)[3] == T:
            assert n % T == want and n >= 8 * (len(lens) - first) and n >= n_min
            return lens
        guess = n
    raise AssertionError('tile shape does not settle')
