"""GPU: the clustering kernels on inputs that sit on their decision boundary (tests/cluster_boundary_ref.py): pairs whose
fl(fl(dx*dx) + fl(dy*dy)) lies within +-3 ulps of the value at which the correctly rounded root reaches the threshold, many of
them decided differently by a fused multiply-add.  Every comparison is bit-exact, nothing is masked out; a kernel with an
approximate root or a contracted sum fails here (tests/test_cluster_boundary_host.py shows that on the CPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_boundary_ref as B  # noqa: E402
import fps_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def failures(p, got_edge, want_edge):
    """(threshold, u, uf, dx, dy) of every pair whose decision is wrong.  Labels and ids run on from pair to pair, so one
    wrong decision shifts every later value: the decisions are compared pair by pair for the report, and the values
    themselves wherever the decisions are right (check_values), so that no difference of any kind passes."""
    bad = np.flatnonzero(np.asarray(got_edge) != np.asarray(want_edge))
    return [(float(p.t), int(p.u[k]), int(p.uf[k]), float(p.dx[k]), float(p.dy[k])) for k in bad]


def check_values(wrong, got, want):
    if not wrong:
        np.testing.assert_array_equal(got, want)


def report(failed, n_thresholds):
    by_u = {}
    for f in failed:
        by_u[f[1]] = by_u.get(f[1], 0) + 1
    return (f'{len(failed)} pairs at {len({f[0] for f in failed})} of {n_thresholds} thresholds decided wrongly; by u: '
            f'{sorted(by_u.items())}; the first ten (t, u, uf, dx, dy): {failed[:10]}; the thresholds: {sorted({f[0] for f in failed})}')


def test_connected_components_on_the_boundary_over_the_sweep():
    """the three shipped connected_dist values and 256 seeded thresholds in [0.05, 4]: about 150 isolated pairs per call,
    one sample per pair, samples stored one after the other"""
    import sst_amd
    failed = []
    pairs = B.sweep()
    for p in pairs:
        n = len(p.dx)
        pts, batch = dev(B.pair_points(p)), dev(np.repeat(np.arange(n, dtype=np.int32), 2))
        want = B.expected_labels(p.u < 0, host(batch))
        got = sst_amd.find_connected_componets(pts, batch, float(p.t))
        assert got.dtype == torch.int32
        lab, count = sst_amd.connected_components_xy(pts, batch, float(p.t), return_count=True)
        assert torch.equal(lab, got) and int(count) == int(lab.max()) + 1
        got = host(got)
        wrong = failures(p, got[0::2] == got[1::2], p.u < 0)
        check_values(wrong, np.append(got, int(count)), np.append(want, want.max() + 1))
        failed += wrong
    assert not failed, report(failed, len(pairs))


@pytest.mark.parametrize('dist', B.SHIPPED_DISTS)
def test_single_batch_form_on_the_boundary(dist):
    """the same kind of pairs in ONE graph: pair origins on a grid of even integers 2 apart, offsets multiples of 2^-18, so
    every coordinate is exact, the kernel's subtraction gives dx and dy back and no cross pair is closer than 2 * dist
    (all asserted on the CPU here and in tests/test_cluster_boundary_host.py)"""
    import sst_amd
    from oracle import cluster_oracle
    p = B.boundary_pairs(dist, 7, quantum=2.0 ** -18)
    pts = B.pair_points(p, B.grid_origins(len(p.dx)))
    assert float(np.abs(pts).max()) < 32                            # 2^-18 is a multiple of the ulp of every coordinate
    want = B.expected_labels(p.u < 0)
    np.testing.assert_array_equal(want, cluster_oracle.find_connected_components_single_batch(pts, p.t))
    got = host(sst_amd.find_connected_componets_single_batch(dev(pts), dev(np.arange(len(pts), dtype=np.int32) % 3), float(p.t)))
    failed = failures(p, got[0::2] == got[1::2], p.u < 0)
    assert not failed, report(failed, 1)
    np.testing.assert_array_equal(got, want)


def test_ssg_ball_on_the_boundary_over_the_sweep():
    """radius = 2.0, 0.6, 1.0 (the radii of fps_ref.FAMILIES; the shipped configurations name none) and the sweep: one
    segment, its keypoint at the origin, every boundary offset an ordinary point: id 0 inside the open ball, -1 outside"""
    import sst_amd
    failed = []
    pairs = [B.boundary_pairs(t, 50 + i) for i, t in enumerate(B.SSG_RADII)] + B.sweep()
    for p in pairs:
        (pts, offsets, key_idx, key_count, thr2, radius), by_construction = B.ssg_ball_case(p)
        want = R.ssg_assign(pts, offsets, key_idx, key_count, thr2, radius)
        np.testing.assert_array_equal(want[0], by_construction[0])
        ids, n_clusters, status = sst_amd.ssg_assign(dev(pts), dev(offsets), dev(key_idx), dev(key_count), float(thr2), float(radius))
        ids = host(ids)
        assert ids[0] == 0 and (int(n_clusters), int(status)) == want[1:] == (1, 0)
        assert np.isin(ids, (0, -1)).all()
        failed += failures(p, ids[1:] == 0, p.u < 0)
    assert not failed, report(failed, len(pairs))


def test_ssg_prune_on_the_boundary_over_the_sweep():
    """thr2 = 4.01, 1.21, 2.01 (radius * 2 + 0.01 of the same radii) and the sweep: one segment per pair, both ends
    keypoints, radius = thr2 / 4: keypoint 1 falls iff d < thr2, which shows in the ids, the cluster count and the status"""
    import sst_amd
    failed = []
    pairs = [B.boundary_pairs(t, 60 + i) for i, t in enumerate(B.SSG_THR2)] + B.sweep()
    for p in pairs:
        (pts, offsets, key_idx, key_count, thr2, radius), by_construction = B.ssg_prune_case(p)
        want = R.ssg_assign(pts, offsets, key_idx, key_count, thr2, radius)
        np.testing.assert_array_equal(want[0], by_construction[0])
        assert want[1:] == by_construction[1:]
        ids, n_clusters, status = sst_amd.ssg_assign(dev(pts), dev(offsets), dev(key_idx), dev(key_count), float(thr2), float(radius))
        ids = host(ids)
        wrong = failures(p, ids[1::2] == -1, p.u < 0)
        check_values(wrong, np.concatenate([ids, [int(n_clusters), int(status)]]), np.concatenate([want[0], want[1:]]))
        failed += wrong
    assert not failed, report(failed, len(pairs))


def test_voxelize_points_on_voxel_faces():
    """floor(fl(fl(p - lo) / v)) with the quotient an integer, or one ulp to either side of one, on every axis: a divide that
    is one ulp off puts the point into the neighbouring voxel.  Both kernels (plain, and the row kernel of voxelize_batch)."""
    import sst_amd
    from oracle import voxel_oracle
    vs, rng = B.VOXEL_FACE_SIZE, B.VOXEL_FACE_RANGE
    pts, cls = B.voxel_face_points(vs, rng, seed=3, per_class=1400)             # 4200 points: the row kernel needs >= 4096
    want = voxel_oracle.dynamic_voxelize(pts, vs, rng)
    got = host(sst_amd.voxelization(dev(pts), list(vs), rng, -1, -1))
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, f'{len(bad)} of {len(pts)} points in the wrong voxel; first: {pts[bad[:5]]}, classes {cls[bad[:5]]}'
    wide = np.concatenate([pts, np.zeros((len(pts), 2), np.float32)], 1)
    _, coors = sst_amd.Voxelization(vs, rng, -1, (-1, -1)).voxelize_batch([dev(wide)])
    np.testing.assert_array_equal(host(coors)[:, 1:], want)
