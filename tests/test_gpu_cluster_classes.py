"""GPU: ``cluster.cluster_assign_classes`` (csrc/cluster_classes.hip: all classes of ClusterAssigner.forward in one pass, one
host read) against the per-class loop it replaces, ``ClusterAssigner.forward_single_class`` class after class.  Every tensor
of both lists and the ``_sst_keep`` index lists must be equal, and two runs bit-equal.

Why equality is a theorem here and not a tolerance: the two paths group the same integer cells, so they can differ only in
the float centroid of a voxel with three or more votes (the segmented mean's walk depends on the shape of the whole call).
Every coordinate below is a multiple of 2^-6 (or, for the +-1 ulp pairs, a voxel holds one vote), so every sum is exact in
float32 whatever its order and the centroids are the same bits on both paths."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_boundary_ref as B  # noqa: E402
import fps_ref as R  # noqa: E402
from test_gpu_cluster_shapes import star_case, xy  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RANGE = [-64.0, -64.0, -4.0, 64.0, 64.0, 4.0]
CELL = (0.5, 0.5, 6.0)           # a tuple is ONE size for every class; a list is read per class, as in the reference
NAMES32 = [f'c{i}' for i in range(32)]
COUNTS = (0, 1, 2, 255, 256, 257, 600)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assigner(g, cells, dists, min_points, training):
    import sst_amd
    a = sst_amd.ClusterAssigner(cells, min_points, RANGE, dists, class_names=NAMES32[:g])
    a.train(training)
    return a


def tables(a, g):
    return ([a._per_class(a.cluster_voxel_size, c) for c in a.class_names[:g]],
            [a._per_class(a.connected_dist, c) for c in a.class_names[:g]])


def check(points, batches, cells, dists, min_points, training):
    """per-class loop == cluster_assign_classes == forward with class_batched, twice; -> the per-class loop's result"""
    import sst_amd
    from sst_amd import cluster
    g = len(points)
    pts, bat = [dev(p) for p in points], [dev(b) for b in batches]
    a = assigner(g, cells, dists, min_points, training)
    want = [a.forward_single_class(p, b, c, None) for p, b, c in zip(pts, bat, a.class_names)]
    cell_list, dist_list = tables(a, g)
    runs = [cluster.cluster_assign_classes(pts, bat, cell_list, dist_list, min_points, RANGE[:3], training) for _ in range(2)]
    for got in runs:
        assert len(got) == g
        for c, ((wi, wm), (gi, gm)) in enumerate(zip(want, got)):
            assert gi.dtype == wi.dtype and gi.shape == wi.shape, (c, gi.shape, wi.shape)
            assert torch.equal(gi, wi), f'class {c}: (sample, component) rows differ'
            assert gm.dtype == torch.bool and torch.equal(gm, wm), f'class {c}: valid masks differ'
            wk = getattr(wm, '_sst_keep', None)                # the per-class path attaches none to an empty class
            assert gm._sst_keep.dtype == torch.int64
            assert torch.equal(gm._sst_keep, wk) if wk is not None else gm._sst_keep.numel() == 0
    for (ai, am), (bi, bm) in zip(*runs):
        assert torch.equal(ai, bi) and torch.equal(am, bm) and torch.equal(am._sst_keep, bm._sst_keep)
    loop = a(pts, bat)
    assert sst_amd.enable_class_batched(a) == 1 and a.class_batched
    fused = a(pts, bat)
    for x, y in zip(loop[0] + loop[1], fused[0] + fused[1]):
        assert x.dtype == y.dtype and torch.equal(x, y)
    return want


def lattice_class(per_sample_counts, seed, origin=(-20.0, -20.0)):
    """n distinct positions of a 48 x 48 unit lattice per sample: with a cell of 0.5 and min_points = 1 every vote is its own
    centroid, so the counts ARE the centroid counts and the class / sample boundaries sit where the counts put them"""
    rng = np.random.default_rng(seed)
    pts, bat = [], []
    for s, n in enumerate(per_sample_counts):
        k = rng.permutation(48 * 48)[:n]
        p = np.stack([origin[0] + (k % 48), origin[1] + (k // 48), rng.integers(-2, 2, n)], 1).astype(np.float32)
        pts.append(p)
        bat.append(np.full(n, s, np.int32))
    return np.concatenate(pts).reshape(-1, 3), np.concatenate(bat)


# per class the votes per sample; the centroid rows of the concatenation put class and sample boundaries inside a
# 256-centroid tile, on its edge and one row after it (running totals in the comments)
LATTICE_CASES = {
    'g1_b1': [[600]],
    'g1_b3_edges': [[255, 1, 1]],                                   # sample boundaries at 255 (inside), 256 (edge)
    'g3_b2_edges': [[256, 1], [255, 2], [0, 257]],                  # 256 edge | 257 one after | 512 edge, 514, 771
    'g3_empty_first': [[0, 0], [257, 255], [2, 600]],
    'g3_empty_middle': [[600, 1], [0, 0], [256, 256]],
    'g3_empty_last': [[1, 0], [255, 257], [0, 0]],
    'g6_b3': [[0, 0, 0], [256, 0, 1], [2, 255, 0], [0, 0, 0], [1, 1, 600], [257, 2, 256]],
    'g3_sample_missing': [[100, 0, 100], [50, 60, 70], [0, 0, 257]],
}


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('case', sorted(LATTICE_CASES))
def test_lattice_counts_at_the_tile_edges(case, training):
    counts = LATTICE_CASES[case]
    data = [lattice_class(c, seed=31 * i + len(case)) for i, c in enumerate(counts)]
    g = len(counts)
    dists = [1.2, 1.5, 2.1, 1.2, 1.5, 2.1][:g]                       # 4-, 8- and 12-neighbourhoods of the unit lattice
    want = check([d[0] for d in data], [d[1] for d in data], CELL, dists, 1, training)
    for (inds, mask), c in zip(want, counts):
        assert inds.size(0) == mask.numel() == sum(c)                # every vote survives: min_points = 1


def test_32_classes_over_every_count():
    counts = [[COUNTS[(i + s) % len(COUNTS)] for s in range(2)] for i in range(32)]
    assert {n for c in counts for n in c} == set(COUNTS)
    data = [lattice_class(c, seed=900 + i) for i, c in enumerate(counts)]
    cells = [[0.5, 0.5, 6.0] if i % 2 else [0.25, 0.5, 3.0] for i in range(32)]
    dists = [1.2 + 0.3 * (i % 4) for i in range(32)]
    for training in (True, False):
        check([d[0] for d in data], [d[1] for d in data], cells, dists, 1, training)


def test_refusals_by_name():
    from sst_amd import cluster
    p, b = dev(np.zeros((4, 3), np.float32)), dev(np.zeros(4, np.int32))
    with pytest.raises(NotImplementedError, match='at most 32'):
        cluster.cluster_assign_classes([p] * 33, [b] * 33, [[1, 1, 1]] * 33, [1.0] * 33, 1, RANGE[:3], True)
    with pytest.raises(ValueError, match='cell size'):
        cluster.cluster_assign_classes([p], [b], [[1, 0, 1]], [1.0], 1, RANGE[:3], True)
    with pytest.raises(ValueError, match='2 cell sizes'):
        cluster.cluster_assign_classes([p], [b], [[1, 1, 1]] * 2, [1.0], 1, RANGE[:3], True)
    with pytest.raises(RuntimeError, match='float32'):
        cluster.cluster_assign_classes([p.double()], [b], [[1, 1, 1]], [1.0], 1, RANGE[:3], True)
    with pytest.raises(RuntimeError, match='sample index'):
        cluster.cluster_assign_classes([p], [b + 256], [[1, 1, 1]], [1.0], 1, RANGE[:3], True)
    with pytest.raises(RuntimeError, match='key layout'):
        cluster.cluster_assign_classes([p + 1e6], [b], [[1, 1, 1]], [1.0], 1, RANGE[:3], True)


@pytest.mark.parametrize('training', [True, False])
def test_all_classes_empty(training):
    empty = (np.zeros((0, 3), np.float32), np.zeros(0, np.int32))
    check([empty[0]] * 3, [empty[1]] * 3, CELL, 0.6, 2, training)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('form', ['list', 'dict', 'scalar'])
def test_clustered_votes_with_the_occupancy_filter(form, training):
    """votes around random centres (multiples of 1/64), min_points = 2: voxels of one vote fall, the centroids are means of
    several votes; class 1 holds only single-vote voxels (a lattice), so there nothing survives and everything is kept,
    next to classes in which some voxels survive; the tables in the three forms the configurations use"""
    g, names = 4, NAMES32[:4]
    pts0, b0 = R.quantised_clusters(1500, 40, 0.4, 3, seed=5)
    pts1, b1 = lattice_class([70, 0, 90], seed=6)
    pts2, b2 = R.quantised_clusters(700, 25, 0.2, 3, seed=7)
    pts3, b3 = R.quantised_clusters(257, 9, 0.3, 2, seed=8)
    cells = [[0.5, 0.5, 6.0], [0.5, 0.5, 6.0], [0.25, 0.25, 6.0], [1.0, 1.0, 8.0]]
    dists = [0.6, 1.2, 0.4, 1.1]
    if form == 'dict':
        cells, dists = dict(zip(names, cells)), dict(zip(names, dists))
    elif form == 'scalar':
        cells, dists = tuple(cells[0]), dists[0]
    want = check([pts0, pts1, pts2, pts3], [b0.astype(np.int32), b1, b2.astype(np.int64), b3.astype(np.int32)], cells, dists,
                 2, training)
    assert 0 < want[0][0].size(0) < 1500 and 0 < want[2][0].size(0)              # the filter drops some votes, keeps some
    assert want[1][0].size(0) == 160 and bool(want[1][1].all())                  # the rule: nothing survived, all kept


@pytest.mark.parametrize('training', [True, False])
def test_identical_coordinates_in_two_classes_and_two_samples_are_not_linked(training):
    one, _ = lattice_class([300], seed=11)
    pts = np.concatenate([one, one])
    bat = np.repeat([0, 1], 300).astype(np.int32)
    want = check([pts, pts, one], [bat, bat, np.zeros(300, np.int32)], CELL, 1.2, 1, training)
    lab0, lab1, lab2 = (w[0][:, 1].cpu().numpy() for w in want)
    np.testing.assert_array_equal(lab0, lab1)                                     # every class numbers from 0 again
    k = int(lab2.max()) + 1
    if training:                                                                  # the samples stay apart: running base
        np.testing.assert_array_equal(lab0[300:], lab0[:300] + k)
        np.testing.assert_array_equal(lab0[:300], lab2)
    else:                                                                         # one graph: coincident votes share a voxel
        np.testing.assert_array_equal(lab0[300:], lab0[:300])


def test_pairs_one_ulp_either_side_of_a_distance_per_class():
    """isolated pairs whose fl(fl(dx*dx) + fl(dy*dy)) lies within 3 ulps of the value at which the root reaches the class's
    own distance (tests/cluster_boundary_ref.py): a cell of 2^-9 gives every vote its own voxel (and keeps the 96 m from the
    origin inside the 65536 cells of the key layout), so the centroids are the votes; the decision of every pair is the
    construction's, for three different distances in one pass"""
    from sst_amd import cluster
    pairs = [B.boundary_pairs(t, 40 + i, quantum=2.0 ** -18) for i, t in enumerate(B.SHIPPED_DISTS)]
    pts = [B.pair_points(p, B.grid_origins(len(p.dx))) for p in pairs]
    assert all(float(np.abs(x).max()) < 32 for x in pts)
    bat = [np.zeros(len(x), np.int32) for x in pts]
    cell = (2.0 ** -9,) * 3
    for training in (True, False):
        check(pts, bat, cell, [float(p.t) for p in pairs], 1, training)
    got = cluster.cluster_assign_classes([dev(x) for x in pts], [dev(b) for b in bat], [list(cell)] * 3, [float(p.t) for p in pairs],
                                         1, RANGE[:3], True)
    for p, (inds, mask) in zip(pairs, got):
        lab = inds[:, 1].cpu().numpy()
        assert len(lab) == 2 * len(p.dx) and bool(mask.all())
        wrong = np.flatnonzero((lab[0::2] == lab[1::2]) != (p.u < 0))
        assert wrong.size == 0, f'dist {p.t!r}: pairs {wrong[:10]} decided wrongly (u = {p.u[wrong[:10]]})'
        assert int(lab.max()) + 1 == int(np.where(p.u < 0, 1, 2).sum())


@pytest.mark.parametrize('training', [True, False])
def test_chain_of_513_and_a_star_beside_other_classes(training):
    """a chain of 513 centroids 19/32 = 0.59375 apart (dist 0.6: just under) that crosses three tiles and the tile of the
    class before it, and the star of tests/test_gpu_cluster_shapes.py (five chains and their hub) in the next class"""
    chain = xy(np.arange(513) * (19.0 / 32.0) - 60.0)
    chains, hub = star_case()
    star = np.concatenate([chains, hub])
    filler, fb = lattice_class([100], seed=3)
    want = check([filler, chain[::-1].copy(), star, chain], [fb, np.zeros(513, np.int32), np.zeros(len(star), np.int32),
                                                             np.zeros(513, np.int32)],
                 (0.25, 0.25, 6.0), [1.2, 0.6, 0.6, 0.59375], 1, training)
    assert (want[1][0][:, 1] == 0).all() and (want[2][0][:, 1] == 0).all()       # one component each
    np.testing.assert_array_equal(want[3][0][:, 1].cpu().numpy(), np.arange(513)[np.argsort(np.argsort(chain[:, 0]))])


def test_tile_pairs_of_other_partitions_leave_early():
    """six classes of 300 centroids: 8 tiles, 36 tile pairs; a pair is staged only where the partitions of its tiles meet"""
    from sst_amd import cluster
    data = [lattice_class([300], seed=70 + i) for i in range(6)]
    _, _, stats = cluster._assign_classes([dev(d[0]) for d in data], [dev(d[1]) for d in data], [[0.5, 0.5, 6.0]] * 6,
                                          [1.2] * 6, 1, RANGE[:3], per_sample=True, count_tiles=True)
    assert stats['host_reads'] == 1 and stats['centroids'] == 1800
    assert stats['tiles_run'] + stats['tiles_skipped'] == 36
    # tile t holds rows 256 t .. 256 t + 255, class c rows 300 c .. 300 c + 299: tiles meet iff they share a class
    cls = [set(range(256 * t // 300, (256 * t + 255) // 300 + 1)) for t in range(8)]
    meet = sum(1 for i in range(8) for j in range(i + 1) if i == j or max(cls[j]) >= min(cls[i]))
    assert stats['tiles_run'] == meet and stats['tiles_skipped'] == 36 - meet > 0
