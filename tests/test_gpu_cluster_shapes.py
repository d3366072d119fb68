"""GPU: the lock-free union-find of csrc/cluster.hip under shapes that random points never make: sizes at the edges of the
256-point tiles, long chains whose index order runs against or across their geometry, many components joined at once by
late (or early) points, coincident points, non-finite coordinates, strided and int64 inputs.  Neighbours are 0.5 apart
(or much farther) and dist is 0.6, so no distance is near the threshold: the expected labels follow from the construction,
components numbered by first appearance; the oracle is compared as well where n <= 3000 (it builds dense N x N x 2 arrays)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DIST = 0.6
STEP = 0.5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(pts, batch=None, dist=DIST):
    import sst_amd
    pts = np.asarray(pts, np.float32)
    batch = np.zeros(len(pts), np.int32) if batch is None else np.asarray(batch, np.int32)
    lab, count = sst_amd.connected_components_xy(dev(pts), dev(batch), dist, return_count=True)
    lab = lab.cpu().numpy()
    assert int(count) == len(np.unique(lab)) == int(lab.max()) + 1
    return lab


def oracle(pts, batch=None, dist=DIST):
    from oracle import cluster_oracle
    assert len(pts) <= 3000
    batch = np.zeros(len(pts), np.int32) if batch is None else batch
    with np.errstate(invalid='ignore'):             # the non-finite case subtracts inf from inf on the diagonal
        return cluster_oracle.find_connected_components(np.asarray(pts, np.float32), batch, dist)


def xy(x, y=0.0):
    x = np.asarray(x, np.float64)
    return np.stack([x, np.broadcast_to(np.asarray(y, np.float64), x.shape), np.zeros_like(x)], 1).astype(np.float32)


def margin_ok(pts, dist=DIST, rel=0.03):
    """no pair distance within 3 % of dist (float64): the construction, not the rounding, decides every edge"""
    p = np.asarray(pts, np.float64)[:, :2]
    for i in range(0, len(p), 512):
        d = np.hypot(p[i:i + 512, None, 0] - p[None, :, 0], p[i:i + 512, None, 1] - p[None, :, 1])
        if (np.abs(d - dist) <= rel * dist).any():
            return False
    return True


@pytest.mark.parametrize('n', [255, 256, 257, 511, 512, 513, 4099])
def test_tile_edges(n):
    """point i at x = r * 0.5 + (r // 7) * 1.0 with r = n - 1 - i: runs of seven against the index order with gaps of 1.5
    between them, two such samples.  The last points sit alone in the last tile and join a run of the tile before."""
    r = n - 1 - np.arange(n)
    one = xy(r * STEP + (r // 7) * 1.0)
    lab_one = ((n - 1) // 7 - r // 7).astype(np.int32)              # the run of point 0 appears first
    pts = np.concatenate([one, one])
    batch = np.repeat([0, 1], n).astype(np.int32)
    want = np.concatenate([lab_one, lab_one + lab_one.max() + 1])
    got = run(pts, batch)
    np.testing.assert_array_equal(got, want)
    if 2 * n <= 3000:
        np.testing.assert_array_equal(oracle(pts, batch), want)


def test_chains_against_and_across_the_index_order():
    n = 2000
    rev = xy((n - 1 - np.arange(n)) * STEP)
    np.testing.assert_array_equal(run(rev), np.zeros(n, np.int32))
    np.testing.assert_array_equal(oracle(rev), np.zeros(n, np.int32))
    shuffled = xy(np.random.default_rng(17).permutation(n) * STEP)
    np.testing.assert_array_equal(run(shuffled), np.zeros(n, np.int32))
    np.testing.assert_array_equal(oracle(shuffled), np.zeros(n, np.int32))


def test_interleaved_chains():
    n = 2000
    i = np.arange(n)
    pts = xy((i // 2) * STEP, np.where(i % 2 == 0, 0.0, 10.0))
    want = (i % 2).astype(np.int32)
    np.testing.assert_array_equal(run(pts), want)
    np.testing.assert_array_equal(oracle(pts), want)


# ----------------------------------------------------------------------------------------------------------------------
# bridges: many components joined at once
# ----------------------------------------------------------------------------------------------------------------------
def radial_chains(k, length, r0):
    """k chains of `length` points leaving the origin radially, the first point of each at radius r0, chain after chain"""
    ang = 2 * np.pi * np.arange(k) / k
    rad = r0 + STEP * np.arange(length)
    return np.stack([(rad[None, :] * np.cos(ang)[:, None]).reshape(-1), (rad[None, :] * np.sin(ang)[:, None]).reshape(-1),
                     np.zeros(k * length)], 1).astype(np.float32)


def star_case():
    """ONE bridge point touching every chain.  Points within dist of a common point and more than dist from each other
    number at most five in the plane (six on a circle of radius < dist are at most dist apart), so a single bridge point
    joins five chains: starts at radius 0.55 (0.55 < 0.6 from the hub, 2 * 0.55 * sin(36 deg) = 0.647 > 0.6 from each other)"""
    chains = radial_chains(5, 64, 0.55)
    hub = np.zeros((1, 3), np.float32)
    assert margin_ok(np.concatenate([chains, hub]))
    return chains, hub


def ring_case():
    """K = 64 chains of 64 points: starts at radius 6.4 (neighbouring starts 2 * 6.4 * sin(pi / 64) = 0.628 > 0.6 apart, farther
    out more).  No single point can touch 64 chains (star_case), so the bridge is a ring of 64 points at radius 5.9, one
    under each chain (0.5 from its start, 0.78 from the neighbouring starts) and 0.579 < 0.6 from its ring neighbours: 64
    components and the ring meet at once."""
    chains = radial_chains(64, 64, 6.4)
    ring = radial_chains(64, 1, 5.9)
    assert margin_ok(np.concatenate([chains, ring]))
    return chains, ring


@pytest.mark.parametrize('case', [star_case, ring_case])
def test_bridge_joins_every_chain(case):
    chains, bridge = case()
    k = len(chains) // 64
    apart = np.repeat(np.arange(k), 64).astype(np.int32)
    np.testing.assert_array_equal(run(chains), apart)                               # labels 0 .. k - 1 by first appearance
    last = np.concatenate([chains, bridge])
    first = np.concatenate([bridge, chains])
    for pts in (last, first):                                                        # bridge at the largest / smallest indices
        np.testing.assert_array_equal(run(pts), np.zeros(len(pts), np.int32))
    if len(last) <= 3000:
        np.testing.assert_array_equal(oracle(chains), apart)
        np.testing.assert_array_equal(oracle(last), np.zeros(len(last), np.int32))
    if case is ring_case:
        # ring points 0 and 1 missing: chains 0 and 1 hang free, the open ring still holds the other 62 together
        cut = np.concatenate([chains, bridge[2:]])
        want = np.full(len(cut), 2, np.int32)
        want[:64], want[64:128] = 0, 1
        np.testing.assert_array_equal(run(cut), want)


def test_coincident_points_and_the_strict_comparison():
    pts = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (1000, 1))
    np.testing.assert_array_equal(run(pts, dist=DIST), np.zeros(1000, np.int32))       # every pair is an edge
    np.testing.assert_array_equal(run(pts, dist=0.0), np.arange(1000, dtype=np.int32))  # 0 < 0 is false: no edge at all
    np.testing.assert_array_equal(oracle(pts, dist=0.0), np.arange(1000, dtype=np.int32))


def test_non_finite_points_are_singletons_and_break_the_chain():
    """a NaN and a +inf coordinate inside a chain of 600 (three tiles): such a point is no link (NaN and inf compare false
    with `< dist`), so it is a singleton with its own first-appearance label and the chain falls into three pieces"""
    n = 600
    pts = xy(np.arange(n) * STEP)
    pts[200, 0] = np.nan
    pts[400, 1] = np.inf
    want = np.zeros(n, np.int32)
    want[200], want[201:400], want[400], want[401:] = 1, 2, 3, 4
    np.testing.assert_array_equal(oracle(pts), want)
    np.testing.assert_array_equal(run(pts), want)


def test_storage_forms():
    """a strided view (row stride 7), int64 sample indices, interleaved samples"""
    import sst_amd
    from oracle import cluster_oracle
    pts, batch = R.quantised_clusters(1500, 40, 0.4, 3, seed=71)       # multiples of 1/64: no distance within 1e-4 of 0.6
    want = cluster_oracle.find_connected_components(pts, batch, DIST)
    big = torch.full((1500, 7), float('nan'))
    big[:, 2:5] = torch.from_numpy(pts)
    view = big.to(DEV)[:, 2:5]
    assert view.stride(0) == 7 and not view.is_contiguous()
    got = sst_amd.connected_components_xy(view, dev(batch.astype(np.int64)), DIST)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    got = sst_amd.find_connected_componets(view, dev(batch.astype(np.int64)), DIST)
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    perm = np.random.default_rng(3).permutation(1500)                   # interleaved: labelled per sample, in stored order
    got = sst_amd.find_connected_componets(dev(pts[perm]), dev(batch[perm].astype(np.int64)), DIST)
    np.testing.assert_array_equal(got.cpu().numpy(), cluster_oracle.find_connected_components(pts[perm], batch[perm], DIST))


def test_properties_on_a_clustered_input():
    pts, batch = R.quantised_clusters(3000, 60, 0.4, 3, seed=72)
    lab = run(pts, batch)                                                # asserts count == number of distinct labels
    d = pts[:, None, :2] - pts[None, :, :2]
    adj = (np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < np.float32(DIST)) & (batch[:, None] == batch[None, :])
    i, j = np.nonzero(adj)
    assert len(i) > 3000 and (lab[i] == lab[j]).all()                    # every edge joins equal labels
    _, first = np.unique(lab, return_index=True)
    assert (np.diff(first) > 0).all() and first[0] == 0                  # labels 0, 1, 2, ... appear in index order
    np.testing.assert_array_equal(lab, oracle(pts, batch))               # and no two components share a label


def test_contended_cases_repeat_bit_for_bit():
    """determinism of the lock-free hooking where most threads meet: ten launches each, all equal"""
    chains, ring = ring_case()
    for pts, dist in ((np.concatenate([chains, ring]), DIST), (np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (1000, 1)), DIST)):
        first = run(pts, dist=dist)
        assert (first == 0).all()
        for _ in range(9):
            np.testing.assert_array_equal(run(pts, dist=dist), first)
