"""CPU: the boundary inputs of tests/cluster_boundary_ref.py decide what the project's restatements decide
(oracle/cluster_oracle.py, tests/fps_ref.py, oracle/voxel_oracle.py), hold the promised number of pairs of every kind at
every threshold of the sweep, and tell the contract from its three near misses (fused multiply-add, root one ulp low,
root one ulp high).  tests/test_gpu_cluster_boundary.py runs the same inputs through the kernels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_boundary_ref as B  # noqa: E402
import fps_ref as R  # noqa: E402


def test_conditions_hold_at_every_threshold_of_the_sweep():
    ths = B.sweep_thresholds()
    assert len(ths) == 259 and [float(t) for t in ths[:3]] == [float(np.float32(d)) for d in B.SHIPPED_DISTS]
    assert all(np.float32(0.05) <= t <= np.float32(4.0) for t in ths[3:])
    for p, t in zip(B.sweep(), ths):
        assert p.t == t
        B.check_conditions(p)                       # >= 8 pairs of every u in -3 .. 3, >= 8 contraction-sensitive ones
        assert 7 * B.MIN_PER_U <= len(p.dx) <= 160   # "about 150": one launch
        assert np.abs(p.u).max() <= 3
        # s* is the boundary of the correctly rounded root, whichever way the root is computed on this host
        below, at = np.nextafter(p.s_star, np.float32(0)), p.s_star
        assert np.sqrt(below) < t <= np.sqrt(at) and B.sqrt_rn(below) < t <= B.sqrt_rn(at)
    for t in B.SHIPPED_DISTS:
        B.check_conditions(B.boundary_pairs(t, 7, quantum=2.0 ** -18))


def test_decisions_equal_the_cluster_oracle():
    """one sample per pair: the generator's labels are the oracle's (scipy's numbering, running base per sample)"""
    from oracle import cluster_oracle
    for p in B.sweep():
        n = len(p.dx)
        batch = np.repeat(np.arange(n), 2)
        want = cluster_oracle.find_connected_components(B.pair_points(p), batch, p.t)
        np.testing.assert_array_equal(B.expected_labels(p.u < 0, batch), want)


def test_single_batch_pairs_are_isolated_exact_and_equal_the_oracle():
    from oracle import cluster_oracle
    for t in B.SHIPPED_DISTS:
        p = B.boundary_pairs(t, 7, quantum=2.0 ** -18)
        pts = B.pair_points(p, B.grid_origins(len(p.dx)))       # asserts that the kernel's subtraction gives dx, dy back
        d = np.hypot(*(pts[:, None, :2].astype(np.float64) - pts[None, :, :2].astype(np.float64)).transpose(2, 0, 1))
        cross = np.ones_like(d, bool)
        k = np.arange(len(pts))
        cross[k, k] = cross[k, k ^ 1] = False
        assert d[cross].min() > 2 * float(t)                    # no cross pair anywhere near the threshold
        want = cluster_oracle.find_connected_components_single_batch(pts, p.t)
        np.testing.assert_array_equal(B.expected_labels(p.u < 0), want)


def test_decisions_equal_the_ssg_restatement():
    ball = [B.boundary_pairs(t, 50 + i) for i, t in enumerate(B.SSG_RADII)] + B.sweep()[::8]
    for p in ball:
        args, want = B.ssg_ball_case(p)
        ids, n_clusters, status = R.ssg_assign(*args)
        np.testing.assert_array_equal(ids, want[0])
        assert (n_clusters, status) == want[1:]
    prune = [B.boundary_pairs(t, 60 + i) for i, t in enumerate(B.SSG_THR2)] + B.sweep()[::8]
    for p in prune:
        args, want = B.ssg_prune_case(p)
        ids, n_clusters, status = R.ssg_assign(*args)
        np.testing.assert_array_equal(ids, want[0])
        assert (n_clusters, status) == want[1:]


def test_every_wrong_variant_changes_the_labels_at_most_thresholds():
    """the tests have teeth: a kernel that computed any of the three near misses would be told apart from the contract"""
    pairs = B.sweep()
    for variant in B.VARIANTS[1:]:
        caught = 0
        for p in pairs:
            right = B.expected_labels(B.decide(p.dx, p.dy, p.t))
            wrong = B.expected_labels(B.decide(p.dx, p.dy, p.t, variant))
            caught += bool((right != wrong).any())
        share = caught / len(pairs)
        print(f'{variant}: labels differ from the contract at {caught} of {len(pairs)} thresholds ({100 * share:.1f} %)')
        assert share > 0.5
    # by construction for the two root variants: u = -1 (an edge; a root one ulp high reaches t) and u = 0 (no edge; a root
    # one ulp low falls below t) are present at every threshold
    for p in pairs:
        high = B.decide(p.dx, p.dy, p.t, 'separate_root_high')
        low = B.decide(p.dx, p.dy, p.t, 'separate_root_low')
        assert not high[p.u == -1].any() and low[p.u == 0].all()


def test_voxel_face_points_equal_the_voxel_oracle():
    from oracle import voxel_oracle
    vs, rng = B.VOXEL_FACE_SIZE, B.VOXEL_FACE_RANGE
    pts, cls = B.voxel_face_points(vs, rng, seed=3)
    got = voxel_oracle.dynamic_voxelize(pts, vs, rng)[:, ::-1]                    # (x, y, z)
    face = np.rint((pts.astype(np.float64) - np.asarray(rng[:3], np.float32)) / np.asarray(vs, np.float32)).astype(np.int64)
    np.testing.assert_array_equal(got, face - (cls == -1))                         # one ulp below the face: the voxel before
    for c in (-1, 0, 1):
        assert ((cls == c).sum(0) >= 64).all()
