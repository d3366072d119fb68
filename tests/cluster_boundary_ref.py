"""Inputs that sit ON the decision boundary of the clustering kernels, with the decision each of them must get.
Test helper: numpy only, no GPU.

The kernels (csrc/cluster.hip cc_pairs_k, csrc/fps.hip ssg_dist) decide `sqrt_rn(fl(fl(dx*dx) + fl(dy*dy))) < t` in float32:
separately rounded products and sum, the correctly rounded root.  sqrt_rn is monotone, so for a threshold t there is one
float32 s* = the smallest s with sqrt_rn(s) >= t, and a pair is an edge iff s < s*.  boundary_pairs() makes offsets (dx, dy)
whose s lies within +-3 ulps of s*, and tags each with
  u    the ulp offset of s_sep = fl(fl(dx*dx) + fl(dy*dy)) from s*   (the contract: edge iff u < 0)
  uf   the same for s_fma = fl(dx*dx + fl(dy*dy)), what a contracted multiply-add would give
One end of a pair sits at the origin (or the offsets are multiples of a power of two that the far end's coordinates can
hold), so the kernel's own subtraction is exact and dx, dy reach its multiplies as they stand here.

decide() restates the edge test four ways: the contract and three near misses (a fused multiply-add, a root one ulp low,
a root one ulp high).  The tests compare the kernels with the contract; tests/test_cluster_boundary_host.py shows that
every near miss changes the answer on these inputs, which random points never do.

voxel_face_points() does the same for the voxelization's floor((p - lo) / v): points whose float32 quotient is an integer
or its neighbour one ulp to either side.
"""
import collections

import numpy as np

F32 = np.float32
VARIANTS = ('separate_rn', 'fused_rn', 'separate_root_low', 'separate_root_high')
CONTRACT = 'separate_rn'
SHIPPED_DISTS = (0.6, 0.4, 0.1)           # connected_dist of the shipped configurations
U_RANGE = tuple(range(-3, 4))
MIN_PER_U = 8                             # every launch holds at least this many pairs of every u in U_RANGE ...
MIN_SENSITIVE = 8                         # ... and this many pairs whose decision a contraction flips

Pairs = collections.namedtuple('Pairs', 't s_star dx dy u uf')


def sqrt_rn(s):
    """the correctly rounded float32 root: the float64 root of a float32 number rounded once more is the exact rounding
    (53 >= 2 * 24 + 2 bits)"""
    return np.sqrt(np.asarray(s, F32).astype(np.float64)).astype(F32)


def _bits(x):
    return np.asarray(x, F32).view(np.int32).astype(np.int64)


def _step(x, k):
    """positive float32 x moved by k ulps"""
    return (np.asarray(x, F32).view(np.int32) + np.asarray(k, np.int32)).view(F32)


def s_star(t):
    """the smallest float32 s with sqrt_rn(s) >= t, t > 0"""
    t = F32(t)
    assert t > 0 and np.isfinite(t)
    s = F32(np.float64(t) * np.float64(t))
    while sqrt_rn(s) >= t:
        s = _step(s, -1)
    while sqrt_rn(s) < t:
        s = _step(s, 1)
    assert sqrt_rn(s) >= t > sqrt_rn(_step(s, -1))
    return F32(s)


def sums(dx, dy):
    """(s_sep, s_fma) of float32 offsets.  s_fma is computed exactly and rounded once: dx * dx is exact in float64 and so
    is its sum with the float32 fl(dy * dy) while the two exponents are close, which is asserted (two-sum error term)."""
    dx, dy = np.asarray(dx, F32), np.asarray(dy, F32)
    yy = dy * dy                                   # float32: rounded
    s_sep = dx * dx + yy                           # float32: product rounded, sum rounded
    a, b = dx.astype(np.float64) * dx.astype(np.float64), yy.astype(np.float64)
    s = a + b
    bb = s - a
    assert ((a - (s - bb)) + (b - bb) == 0).all(), 'dx * dx + fl(dy * dy) is not exact in float64'
    return s_sep, s.astype(F32)


def decide(dx, dy, t, variant=CONTRACT):
    """bool per pair: is it an edge under the named restatement of the test"""
    s_sep, s_fma = sums(dx, dy)
    t = F32(t)
    if variant == 'separate_rn':
        return sqrt_rn(s_sep) < t
    if variant == 'fused_rn':
        return sqrt_rn(s_fma) < t
    if variant == 'separate_root_low':
        return _step(sqrt_rn(s_sep), -1) < t
    if variant == 'separate_root_high':
        return _step(sqrt_rn(s_sep), 1) < t
    raise KeyError(variant)


def sensitive(p):
    """pairs whose decision a contraction of dx * dx + fl(dy * dy) flips"""
    return (p.u < 0) != (p.uf < 0)


def boundary_pairs(t, seed, quantum=None, per_u=16, n_sensitive=40, n_theta=None):
    """about 7 * per_u + n_sensitive offsets (dx, dy) > 0 around the circle of radius t, |u| <= 3, in a seeded random
    order.  quantum: make dx and dy multiples of this power of two (for pairs that do not start at the origin).
    Asserts the conditions every launch relies on: >= MIN_PER_U pairs of every u, >= MIN_SENSITIVE sensitive ones."""
    t = F32(t)
    ss = s_star(t)
    rng = np.random.default_rng(seed)
    if n_theta is None:
        n_theta = 1024 if quantum is None else 1 << 16
    # 0.3 rad off the axes: dx * dx and dy * dy stay within a factor 16 of each other (sums() needs close exponents)
    theta = rng.uniform(0.3, np.pi / 2 - 0.3, n_theta)
    dx = (np.float64(t) * np.cos(theta)).astype(F32)
    if quantum is not None:
        dx = (np.round(dx.astype(np.float64) / quantum) * quantum).astype(F32)
    dy0 = np.sqrt(np.float64(ss) - dx.astype(np.float64) ** 2)
    if quantum is None:
        steps = np.arange(-6, 7)
        dx = np.repeat(dx, len(steps))
        dy = _step(np.repeat(dy0.astype(F32), len(steps)), np.tile(steps, n_theta))
    else:
        dy = (np.round(dy0 / quantum) * quantum).astype(F32)
        assert (dx.astype(np.float64) / quantum % 1 == 0).all() and (dy.astype(np.float64) / quantum % 1 == 0).all()
    s_sep, s_fma = sums(dx, dy)
    u, uf = _bits(s_sep) - _bits(ss), _bits(s_fma) - _bits(ss)
    near = np.abs(u) <= 3
    dx, dy, u, uf = dx[near], dy[near], u[near], uf[near]
    flips = (u < 0) != (uf < 0)
    keep = np.zeros(len(dx), bool)
    for k in U_RANGE:                              # flipping pairs first inside each u, so that they are well mixed in
        idx = np.flatnonzero(u == k)
        idx = np.concatenate([idx[flips[idx]], idx[~flips[idx]]])
        half = np.concatenate([idx[:per_u // 2], idx[::-1][:per_u - per_u // 2]])
        keep[half] = True
    keep[np.flatnonzero(flips & ~keep)[:n_sensitive]] = True
    order = rng.permutation(np.flatnonzero(keep))
    p = Pairs(t, ss, dx[order], dy[order], u[order], uf[order])
    check_conditions(p)
    return p


def check_conditions(p):
    for k in U_RANGE:
        assert int((p.u == k).sum()) >= MIN_PER_U, f't = {p.t!r}: only {int((p.u == k).sum())} pairs with u = {k}'
    assert int(sensitive(p).sum()) >= MIN_SENSITIVE, f't = {p.t!r}: only {int(sensitive(p).sum())} contraction-sensitive pairs'
    assert (p.dx > 0).all() and (p.dy > 0).all() and np.isfinite(p.dx).all() and np.isfinite(p.dy).all()
    # the tags are the decision: u < 0 <=> the contract's test, uf < 0 <=> the fused one
    assert ((p.u < 0) == decide(p.dx, p.dy, p.t)).all() and ((p.uf < 0) == decide(p.dx, p.dy, p.t, 'fused_rn')).all()


def sweep_thresholds(n=256, seed=2024):
    """the shipped connected_dist values and n seeded float32 thresholds in [0.05, 4.0]"""
    rng = np.random.default_rng(seed)
    return [F32(d) for d in SHIPPED_DISTS] + list(rng.uniform(0.05, 4.0, n).astype(F32))


def expected_labels(edges, batch=None):
    """labels of isolated pairs stored pair after pair (points 2k and 2k + 1): components numbered by first appearance,
    which for samples stored one after the other is also the per-sample numbering with a running base.
    batch (per point), if given, must put the two points of a pair in one sample and the samples in ascending order."""
    edges = np.asarray(edges, bool)
    if batch is not None:
        batch = np.asarray(batch)
        assert len(batch) == 2 * len(edges) and (batch[0::2] == batch[1::2]).all() and (np.diff(batch) >= 0).all()
    first = np.concatenate([[0], np.cumsum(np.where(edges, 1, 2))[:-1]])
    return np.stack([first, first + np.where(edges, 0, 1)], 1).reshape(-1).astype(np.int32)


def pair_points(p, origins=None):
    """float32 [2n, 3] points, pair after pair: the near end at the origin (or at origins[k]), the far end dx, dy away.
    With origins the far end must be exactly representable, so that the kernel's subtraction gives dx, dy back: asserted."""
    n = len(p.dx)
    pts = np.zeros((2 * n, 3), F32)
    if origins is not None:
        pts[0::2, :2] = pts[1::2, :2] = np.asarray(origins, F32)
    pts[1::2, 0] += p.dx
    pts[1::2, 1] += p.dy
    assert (pts[1::2, 0] - pts[0::2, 0] == p.dx).all() and (pts[1::2, 1] - pts[0::2, 1] == p.dy).all()
    assert (pts[1::2, 0].astype(np.float64) - pts[0::2, 0].astype(np.float64) == p.dx.astype(np.float64)).all()
    assert (pts[1::2, 1].astype(np.float64) - pts[0::2, 1].astype(np.float64) == p.dy.astype(np.float64)).all()
    return pts


def grid_origins(n, spacing=2.0, first=2.0):
    """n pair origins on a square grid of small even coordinates"""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return np.stack([first + spacing * (k % side), first + spacing * (k // side)], 1).astype(F32)


_SWEEP = {}


def sweep():
    """[Pairs] for sweep_thresholds(), made once per process and shared by the tests (read only)"""
    if 'pairs' not in _SWEEP:
        _SWEEP['pairs'] = [boundary_pairs(t, seed=1000 + i) for i, t in enumerate(sweep_thresholds())]
    return _SWEEP['pairs']


# ----------------------------------------------------------------------------------------------------------------------
# the SSG forms of the same decision (sst_ssg_assign_f32: `< radius` in the ball, `< thr2` in the pruning)
# ----------------------------------------------------------------------------------------------------------------------
SSG_RADII = (2.0, 0.6, 1.0)               # the radii of tests/fps_ref.py FAMILIES; tests/golden/configs ship none
SSG_THR2 = (4.01, 1.21, 2.01)             # radius * 2 + 0.01 of the same, ssg_single_sample's rule


def ssg_ball_case(p):
    """one segment, its keypoint at the origin (point 0), every boundary offset an ordinary point; radius = p.t.
    -> (points, offsets, key_idx, key_count, thr2, radius), and the ids by construction"""
    n = len(p.dx)
    pts = np.zeros((n + 1, 3), F32)
    pts[1:, 0], pts[1:, 1] = p.dx, p.dy
    ids = np.concatenate([[0], np.where(p.u < 0, 0, -1)]).astype(np.int32)    # in the only ball, or in none
    return (pts, np.array([0, n + 1], np.int32), np.zeros((1, 1), np.int32), np.ones(1, np.int32),
            F32(2 * p.t + F32(0.01)), p.t), (ids, 1, 0)


def ssg_prune_case(p):
    """one segment per pair, both ends keypoints [0, 1]; thr2 = p.t, radius = thr2 / 4: keypoint 1 falls iff d < thr2.
    Then it gets no id (it lies in no ball) and the numbering moves on by one instead of two."""
    n = len(p.dx)
    edges = p.u < 0
    lab = expected_labels(edges)
    ids = lab.copy()
    ids[1::2] = np.where(edges, -1, lab[1::2])
    key_idx = np.tile(np.array([[0, 1]], np.int32), (n, 1))
    return (pair_points(p), np.arange(0, 2 * n + 1, 2).astype(np.int32), key_idx, np.full(n, 2, np.int32), p.t,
            F32(p.t / F32(4))), (ids.astype(np.int32), int(np.where(edges, 1, 2).sum()), 0)


# ----------------------------------------------------------------------------------------------------------------------
# voxel faces
# ----------------------------------------------------------------------------------------------------------------------
VOXEL_FACE_SIZE = (0.32, 0.32, 0.25)       # the SST grid in x and y; 24 cells in z, so that z has interior faces too
VOXEL_FACE_RANGE = [-74.88, -74.88, -2, 74.88, 74.88, 4]


def voxel_face_points(voxel_size, pc_range, seed, per_class=64):
    """float32 [n, 3] points whose quotient q = fl(fl(p - lo) / v) is, on every axis, an integer k, or k one ulp down, or
    k one ulp up - the three classes in equal numbers per axis (asserted).  floor(q) changes between the first two, so a
    divide that is one ulp off moves the point into the neighbouring voxel.  Returns (points, cls [n, 3] in {-1, 0, 1})."""
    rng = np.random.default_rng(seed)
    v, lo, hi = np.asarray(voxel_size, F32), np.asarray(pc_range[:3], F32), np.asarray(pc_range[3:], F32)
    cols, classes = [], []
    for a in range(3):
        grid = int(np.ceil((hi[a] - lo[a]) / v[a]))
        found = {-1: [], 0: [], 1: []}
        assert grid >= 4
        ks = rng.integers(1, grid, 40 * per_class)     # interior faces: the clamp to [0, grid - 1] hides nothing
        base = (lo[a].astype(np.float64) + ks * v[a].astype(np.float64)).astype(F32)
        for step in range(-4, 5):
            p = base.copy()
            for _ in range(abs(step)):
                p = np.nextafter(p, F32(np.inf if step > 0 else -np.inf))
            q = (p - lo[a]) / v[a]                 # float32 subtract, float32 divide
            kf = ks.astype(F32)
            for c, target in ((-1, np.nextafter(kf, F32(-np.inf))), (0, kf), (1, np.nextafter(kf, F32(np.inf)))):
                found[c].append(p[q == target])
        for c in found:
            found[c] = np.unique(np.concatenate(found[c]))
            assert len(found[c]) >= 8, f'axis {a}: only {len(found[c])} distinct coordinates of class {c}'
            found[c] = rng.choice(found[c], per_class, replace=len(found[c]) < per_class)   # a short axis repeats faces
        col = np.concatenate([found[-1], found[0], found[1]])
        cls = np.repeat([-1, 0, 1], per_class)
        perm = rng.permutation(len(col))
        cols.append(col[perm])
        classes.append(cls[perm])
    return np.stack(cols, 1).astype(F32), np.stack(classes, 1)
